"""GPU: every GroupNorm-conv form and its backward on ill-conditioned inputs (tests/conditioning.py: truncation-saturated, near-constant, exactly
constant, large-mean, spike, dead-group and 2^+-40 scaled samples mixed into one launch) against FLOAT64 torch, sample by sample.

The other kernel tests draw relu(randn), on which a kernel that folds the centre of  (x - fl32(mean)) * scale + shift  into its shift, or sums
its statistics in fp32, passes everything; on near-constant, constant and large-mean samples such a kernel misses the bars below by 10x .. 100x
(tests/test_conditioning_cpu.py asserts that).  fp32 torch is no reference on these inputs for the same reason.  Bars are the forms' existing ones:
2e-5 for the direct and the fp32-MFMA kernels, 1e-5 for the fp32 decoder form and every split-operand form, 2e-4 for gradients -- applied per
sample (cnd.per_sample_close), so a loud sample cannot hide a quiet one.  The worst error per (form, family) is printed at the end of the module
(profiles/conditioning_errors.txt holds that table from an MI355X)."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conditioning as cnd
from oracle import refpath

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NF = len(cnd.FAMILIES)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU visible')
    from rfuse import ops as _ops
    return _ops


@pytest.fixture(scope='module', autouse=True)
def error_table():
    yield
    if cnd.TABLE:
        print('\n' + cnd.format_table())


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).float()


def dev(t):
    return t.to(DEV) if t is not None else None


def layer_params(gen, cin, cout, fan=27):
    """drawn as the kernel tests draw them"""
    return 1 + 0.2 * rnd(gen, cin), 0.2 * rnd(gen, cin), rnd(gen, cout, cin, 3, 3, 3, scale=1.0 / np.sqrt(fan * cin))


def ref_gcr64(src0, src1, gamma, beta, groups, w, idx=None):
    """float64 ReLU(conv3(GroupNorm(cat(src0, up2(src1))))) of the samples ``idx`` (CPU tensors in, float64 out)"""
    pick = lambda t: None if t is None else (t if idx is None else t[idx]).detach().cpu().double()
    s0, s1 = pick(src0), pick(src1)
    x = torch.cat([t for t in (s0, F.interpolate(s1, scale_factor=2, mode='nearest') if s1 is not None else None) if t is not None], 1)
    x = F.group_norm(x, cnd.gn_groups(x.shape[1], groups), gamma.detach().cpu().double(), beta.detach().cpu().double(), eps=1e-5)
    return F.relu(F.conv3d(x, w.detach().cpu().double(), None, padding=1))


def two_layers64(x64, convs):
    for sc in convs:
        gn = sc.groupnorm
        g = cnd.gn_groups(gn.num_channels, gn.num_groups)
        x64 = F.relu(F.conv3d(F.group_norm(x64, g, gn.weight.detach().double().cpu(), gn.bias.detach().double().cpu(), gn.eps),
                              sc.conv.weight.detach().double().cpu(), padding=1))
    return x64


def subset(n, fams, nfam=NF):
    idx = cnd.reference_subset(n, nfam)
    return idx, [fams[i] for i in idx]


def check_affine_triple(aff, src0, src1, gamma, beta, groups, fams, what):
    """the folded GroupNorm as tests/test_kernels_gpu.py:test_conv3d_gn_relu pins it, per sample: centre == fl32(float64 mean), scale to 1e-6, the
    two-term shift to 1e-6 and the shift itself -- which carries what fl32(mean) loses -- to 1e-7"""
    x = torch.cat([t for t in (src0, F.interpolate(src1, scale_factor=2, mode='nearest') if src1 is not None else None) if t is not None], 1)
    n, cin = x.shape[0], x.shape[1]
    mean_c, rstd_c = cnd.group_stats64(x, cnd.gn_groups(cin, groups))
    sc_ref = gamma.double()[None] * rstd_c
    a64 = aff.cpu().double()
    assert torch.equal(aff[..., 0].cpu(), mean_c.float()), what + ': centre = fp32-rounded float64 mean'
    cnd.per_sample_close(a64[..., 1], sc_ref, 1e-6, fams, what + ': gn scale')
    cnd.per_sample_close(a64[..., 2] - a64[..., 0] * a64[..., 1], beta.double()[None] - mean_c * sc_ref, 1e-6, fams, what + ': gn two-term shift')
    cnd.per_sample_close(a64[..., 2], beta.double()[None] - (mean_c - mean_c.float().double()) * sc_ref, 1e-7, fams, what + ': gn shift')


def same_affine(a, b, what):
    """two affine triples [n, C, 4] describe the same map to 1e-6, sample by sample (test_kernels_gpu.py:same_affine with a bound per sample)"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    fams = ['all'] * a.shape[0]
    cnd.per_sample_close(a[..., 1], b[..., 1], 1e-6, fams, what + ' (scale)')
    cnd.per_sample_close(a[..., 2] - a[..., 0] * a[..., 1], b[..., 2] - b[..., 0] * b[..., 1], 1e-6, fams, what + ' (shift)')


def fused_stats_agree(ops, gen, t, cout, groups, what):
    g = groups if cout % groups == 0 else 1
    g2, b2 = dev(1 + 0.2 * rnd(gen, cout)), dev(0.2 * rnd(gen, cout))
    assert getattr(t, '_rf_stats', None) is not None, what + ': no fused statistics'
    same_affine(ops.gn_affine(t, None, g2, b2, g), ops.gn_affine(t.clone(), None, g2, b2, g), 'fused statistics, ' + what)


def no_further_than_fp32(got, fp32, ref, idx, case):
    """a split form is no further from float64 than the fp32 kernel on the same affine: rms <= 1.05x, max <= 1.25x (as the existing split tests)"""
    e_s, e_f = (got[idx].cpu().double() - ref).flatten(), (fp32[idx].cpu().double() - ref).flatten()
    rms_s, rms_f = e_s.pow(2).mean().sqrt().item(), e_f.pow(2).mean().sqrt().item()
    print(f'\n{case}: error vs float64  split rms {rms_s:.3e} max {e_s.abs().max().item():.3e} | fp32 rms {rms_f:.3e} max {e_f.abs().max().item():.3e}')
    assert rms_s <= 1.05 * rms_f and e_s.abs().max().item() <= 1.25 * e_f.abs().max().item()


# ------------------------------------------------------------------------------------------------------------------ forward forms

DIRECT_CASES = [
    # (n, c0, c1, edge, cout, groups)
    (18, 8, 0, 8, 16, 8),
    (18, 1, 0, 8, 8, 8),        # one group
    (18, 16, 0, 4, 32, 8),
    (70, 64, 0, 2, 128, 8),
    (18, 64, 0, 1, 128, 8),
    (18, 32, 64, 8, 56, 8),     # groups straddle the two sources
    (9, 6, 0, 8, 12, 6),
]


@pytest.mark.parametrize('case', DIRECT_CASES)
def test_direct_and_fp32_mfma_forms(ops, case):
    n, c0, c1, edge, cout, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 1)
    if edge == 1:                                                       # a 1^3 volume has no low-resolution source
        assert c1 == 0
    src0, src1, fams = cnd.mixed_pair(gen, n, c0, c1, edge, groups)
    gamma, beta, w = layer_params(gen, c0 + c1, cout)
    d0, d1 = dev(src0), dev(src1)
    aff = ops.gn_affine(d0, d1, dev(gamma), dev(beta), groups)
    check_affine_triple(aff, src0, src1, gamma, beta, groups, fams, 'gn_affine')
    ref = ref_gcr64(src0, src1, gamma, beta, groups, w)
    wd = dev(w)
    direct = ops.conv3d_gn_relu(d0, d1, aff, None, cout, direct_weight=wd)
    cnd.per_sample_close(direct, ref, 2e-5, fams, 'direct conv')
    if edge >= 2:
        mfma = ops.conv3d_gn_relu(d0, d1, aff, ops.pack_conv3_weight(wd), cout)
        cnd.per_sample_close(mfma, ref, 2e-5, fams, 'fp32 MFMA conv')
        cnd.per_sample_close(mfma, direct, 2e-5, fams, 'fp32 MFMA conv vs direct conv')
        if getattr(mfma, '_rf_stats', None) is not None:
            fused_stats_agree(ops, gen, mfma, cout, groups, 'fp32 MFMA conv')


def test_fused_maxpool_epilogue(ops):
    case = (300, 8, 16, 16, 8)
    n, cin, edge, cout, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 2)
    src, fams = cnd.mixed(gen, n, cin, edge, groups)
    gamma, beta, w = layer_params(gen, cin, cout)
    x = dev(src)
    aff = ops.gn_affine(x, None, dev(gamma), dev(beta), groups)
    wp = ops.pack_conv3_weight(dev(w))
    assert ops.conv_pool_supported(x, None, cout)
    plain = ops.conv3d_gn_relu(x, None, aff, wp, cout)
    want_pool = ops.maxpool2(plain)
    full, pooled = ops.conv3d_gn_relu_pool(x, None, aff, wp, cout, keep_full=True)
    assert torch.equal(full, plain) and torch.equal(pooled, want_pool)
    none, pooled_only = ops.conv3d_gn_relu_pool(x, None, aff, wp, cout, keep_full=False)
    assert none is None and torch.equal(pooled_only, want_pool)
    idx, sub = subset(n, fams)
    ref = ref_gcr64(src, None, gamma, beta, groups, w, idx)
    cnd.per_sample_close(full[idx], ref, 2e-5, sub, 'fp32 MFMA conv + pool: full')
    cnd.per_sample_close(pooled_only[idx], F.max_pool3d(ref, 2), 2e-5, sub, 'fp32 MFMA conv + pool: pooled')
    for t, nm in ((pooled, 'pooled'), (pooled_only, 'pooled only'), (full, 'full')):
        fused_stats_agree(ops, gen, t, cout, groups, 'fp32 MFMA conv + pool: ' + nm)


@pytest.mark.parametrize('case', [(4099, 16, 0, 4, 16, 8), (32770, 64, 0, 2, 16, 8)])
def test_position_major_small_volume_form(ops, case):
    """conv3d_small.hip, reached by many samples; the generic kernel, reached by few samples at a time, must give the same bits and the same
    statistics (as test_conv_small_volume_position_major_kernel demands), and both the float64 value.  No predicate names the position-major
    kernel: the sample count alone selects it inside rf_conv3d_k3_gn_relu (from 128 workgroups on), which is why the few-sample launches below
    reach the other one."""
    n, cin, _, edge, cout, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 3)
    src, fams = cnd.mixed(gen, n, cin, edge, groups)
    gamma, beta, w = layer_params(gen, cin, cout)
    x = dev(src)
    wp = ops.pack_conv3_weight(dev(w))
    aff = ops.gn_affine(x, None, dev(gamma), dev(beta), groups)
    got = ops.conv3d_gn_relu(x, None, aff, wp, cout)
    step = {4: 500, 2: 3000}[edge]
    parts = [ops.conv3d_gn_relu(x[i:i + step].contiguous(), None, aff[i:i + step].contiguous(), wp, cout) for i in range(0, n, step)]
    assert torch.equal(got, torch.cat(parts))
    cnd.tensor_close(got._rf_stats[0].sum(dim=2), torch.cat([y._rf_stats[0] for y in parts]).sum(dim=2), 1e-12, 'position-major conv: fused sums vs generic kernel', floor=1.0)
    idx, sub = subset(n, fams)
    cnd.per_sample_close(got[idx], ref_gcr64(src, None, gamma, beta, groups, w, idx), 2e-5, sub, 'position-major conv')
    fused_stats_agree(ops, gen, got, cout, groups, 'position-major conv')


@pytest.mark.parametrize('case', [(256, 32, 64, 8, 56, 8), (1027, 64, 128, 4, 64, 8), (300, 0, 16, 8, 16, 8)])
def test_fp32_decoder_form(ops, case):
    n, c0, c1, edge, cout, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 4)
    src0, src1, fams = cnd.mixed_pair(gen, n, c0, c1, edge, groups)
    gamma, beta, w = layer_params(gen, c0 + c1, cout)
    d0, d1 = dev(src0), dev(src1)
    assert ops.conv_up_supported(d0, d1, cout)
    aff = ops.gn_affine(d0, d1, dev(gamma), dev(beta), groups)
    wd = dev(w)
    got = ops.conv3d_up_gn_relu(d0, d1, aff, ops.pack_conv3_up_weight(wd, c0), cout)
    generic = ops.conv3d_gn_relu(d0, d1, aff, ops.pack_conv3_weight(wd), cout)
    cnd.per_sample_close(got, generic, 1e-5, fams, 'fp32 decoder form vs generic kernel')
    idx, sub = subset(n, fams)
    cnd.per_sample_close(got[idx], ref_gcr64(src0, src1, gamma, beta, groups, w, idx), 1e-5, sub, 'fp32 decoder form')
    fused_stats_agree(ops, gen, got, cout, groups, 'fp32 decoder form')


SPLIT_BOX_CASES = [
    # (n, cin, edge, cout, groups)
    (1030, 8, 8, 16, 8),
    (130, 8, 16, 16, 8),
    (1025, 56, 8, 16, 8),       # cpg 7
    (1030, 32, 4, 64, 8),       # s4
    (2049, 16, 8, 16, 8),       # z-column
    (16, 24, 32, 48, 6),
    (3, 16, 64, 16, 8),         # three 64^3 samples: near_constant, big_mean, saturated -- statistics per box
]


@pytest.mark.parametrize('case', SPLIT_BOX_CASES)
def test_split_box_form(ops, case):
    n, cin, edge, cout, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 5)
    families = ('near_constant', 'big_mean', 'saturated') if edge == 64 else cnd.FAMILIES
    src, fams = cnd.mixed(gen, n, cin, edge, groups, families)
    gamma, beta, w = layer_params(gen, cin, cout)
    x = dev(src)
    assert ops.conv_split_supported(x, None, cout)
    aff = ops.gn_affine(x, None, dev(gamma), dev(beta), groups)
    wd = dev(w)
    ws = ops.pack_conv3_split_weight(wd)
    got = ops.conv3d_split_gn_relu(x, aff, ws, cout)
    fp32 = ops.conv3d_gn_relu(x, None, aff, ops.pack_conv3_weight(wd), cout)
    idx, sub = subset(n, fams, len(families))
    ref = ref_gcr64(src, None, gamma, beta, groups, w, idx)
    cnd.per_sample_close(fp32[idx], ref, 2e-5, sub, 'fp32 MFMA conv (beside the split box form)')
    cnd.per_sample_close(got[idx], ref, 1e-5, sub, 'split box form')
    cnd.per_sample_close(got, fp32, 1e-5, fams, 'split box form vs fp32 MFMA')
    no_further_than_fp32(got, fp32, ref, idx, case)
    want_pool = ops.maxpool2(got)
    full, pooled = ops.conv3d_split_gn_relu(x, aff, ws, cout, pool='also')
    assert torch.equal(full, got) and torch.equal(pooled, want_pool)
    none, pooled_only = ops.conv3d_split_gn_relu(x, aff, ws, cout, pool='only')
    assert none is None and torch.equal(pooled_only, want_pool)
    cnd.per_sample_close(pooled_only[idx], F.max_pool3d(ref, 2), 1e-5, sub, 'split box form: fused pool')
    for t, nm in ((got, 'full'), (pooled, 'pooled'), (pooled_only, 'pooled only'), (full, 'full beside pooled')):
        fused_stats_agree(ops, gen, t, cout, groups, 'split box form: ' + nm)


@pytest.mark.parametrize('case', [(260, 8, 6, 4, 2), (513, 20, 40, 4, 2), (300, 72, 40, 8, 1)])
def test_e2_gemm_form(ops, case):
    n, cin, cout, groups, edge = case
    gen = torch.Generator().manual_seed(sum(case) + 6)
    src, fams = cnd.mixed(gen, n, cin, edge, groups)
    gamma, beta, w = layer_params(gen, cin, cout, fan=edge ** 3)
    x = dev(src)
    assert ops.conv_e2_split_supported(x, cout)
    aff = ops.gn_affine(x, None, dev(gamma), dev(beta), groups)
    wd = dev(w)
    got = ops.conv3d_e2_split_gn_relu(x, aff, ops.pack_conv3_e2_split_weight(wd, edge), cout)
    fp32 = ops.conv3d_gn_relu(x, None, aff, ops.pack_conv3_weight(wd) if edge > 1 else None, cout, direct_weight=wd if edge == 1 else None)
    ref = ref_gcr64(src, None, gamma, beta, groups, w)
    cnd.per_sample_close(got, ref, 1e-5, fams, 'e2 GEMM form')
    cnd.per_sample_close(got, fp32, 1e-5, fams, 'e2 GEMM form vs fp32 kernel')
    no_further_than_fp32(got, fp32, ref, slice(None), case)
    fused_stats_agree(ops, gen, got, cout, groups, 'e2 GEMM form')


@pytest.mark.parametrize('case', [(260, 8, 8, 8, 33, 4), (257, 0, 16, 8, 64, 8)])           # the two smallest of test_kernels_gpu.py:SPLIT_UP_CASES
def test_decoder_split_form(ops, case):
    n, c0, c1, edge, cout, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 7)
    src0, src1, fams = cnd.mixed_pair(gen, n, c0, c1, edge, groups)
    gamma, beta, w = layer_params(gen, c0 + c1, cout)
    d0, d1 = dev(src0), dev(src1)
    assert ops.conv_up_split_supported(d0, d1, cout)
    aff = ops.gn_affine(d0, d1, dev(gamma), dev(beta), groups)
    wd = dev(w)
    got = ops.conv3d_up_split_gn_relu(d0, d1, aff, ops.pack_conv3_up_split_weight(wd, c0), cout)
    if ops.conv_up_supported(d0, d1, cout):
        fp32 = ops.conv3d_up_gn_relu(d0, d1, aff, ops.pack_conv3_up_weight(wd, c0), cout)
    else:                                                               # no fp32 decoder-form instance for this shape: the generic fp32 kernel
        fp32 = ops.conv3d_gn_relu(d0, d1, aff, ops.pack_conv3_weight(wd), cout)
    idx, sub = subset(n, fams)
    ref = ref_gcr64(src0, src1, gamma, beta, groups, w, idx)
    cnd.per_sample_close(got[idx], ref, 1e-5, sub, 'decoder split form')
    cnd.per_sample_close(got, fp32, 1e-5, fams, 'decoder split form vs fp32 decoder form')
    no_further_than_fp32(got, fp32, ref, idx, case)
    fused_stats_agree(ops, gen, got, cout, groups, 'decoder split form')


@pytest.mark.parametrize('case', [(300, 8, 16, 8), (37, 16, 32, 8)])                       # the two smallest of test_kernels_gpu.py:UP_CH8_CASES
def test_decoder_split_form_channel_interleaved(ops, case):
    n, c1, edge, cout = case
    gen = torch.Generator().manual_seed(sum(case) + 8)
    groups = 8 if c1 % 8 == 0 else 1
    _, src1, fams = cnd.mixed_pair(gen, n, 0, c1, edge, groups)
    gamma, beta, w = layer_params(gen, c1, cout)
    d1 = dev(src1)
    aff = ops.gn_affine(None, d1, dev(gamma), dev(beta), groups)
    wp = ops.pack_conv3_up_split_weight(dev(w), 0)
    from rfuse import _lib
    assert _lib.load().rf_conv3d_up_split_ch8_supported(0, c1, n, edge, cout)
    plain = ops.conv3d_up_split_gn_relu(None, d1, aff, wp, cout)
    got, stats, tiles = ops.conv3d_up_split_gn_relu_ch8(d1, aff, wp, cout)
    back = got.permute(0, 1, 5, 2, 3, 4).reshape(n, cout, edge, edge, edge)
    assert torch.equal(back, plain), 'ch8 output differs from the NCDHW output: max %.3e' % (back - plain).abs().max().item()
    pst, ptiles = plain._rf_stats[:2]
    assert tiles == ptiles and torch.equal(stats, pst), 'per-box statistics differ'
    fused_stats_agree(ops, gen, plain, cout, 8, 'decoder split form beside ch8 (the same per-box sums)')
    idx, sub = subset(n, fams)
    cnd.per_sample_close(back[idx], ref_gcr64(None, src1, gamma, beta, groups, w, idx), 1e-5, sub, 'decoder split form, ch8')


@pytest.mark.parametrize('case', [(18, 16, 0, 8, 8), (18, 1, 0, 16, 8), (9, 56, 0, 4, 8), (18, 32, 64, 8, 8)])
def test_gn_affine_against_float64(ops, case):
    """rf_gn_stats directly: (n, c0, c1, edge, groups), every family in the batch"""
    n, c0, c1, edge, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 9)
    src0, src1, fams = cnd.mixed_pair(gen, n, c0, c1, edge, groups)
    gamma, beta = 1 + 0.2 * rnd(gen, c0 + c1), 0.2 * rnd(gen, c0 + c1)
    aff = ops.gn_affine(dev(src0), dev(src1), dev(gamma), dev(beta), groups)
    check_affine_triple(aff, src0, src1, gamma, beta, groups, fams, 'gn_affine')


# ------------------------------------------------------------------------------------------------------------------ pre-split hand-overs
# the second GroupNorm of these routes comes from the producer's epilogue: `constant` samples give it a near-constant intermediate, and the first
# conv's weight rows of one whole group of its output channels are zeroed, so that group of the intermediate is exactly zero (var == 0 there)

def zero_first_group(sc, next_gn):
    g = cnd.gn_groups(next_gn.num_channels, next_gn.num_groups)
    with torch.no_grad():
        sc.conv.weight[:next_gn.num_channels // g] = 0.0


def jitter_groupnorms(blk, gen):
    with torch.no_grad():
        for sc in (blk.SingleConv1, blk.SingleConv2):
            gn = sc.groupnorm
            gn.weight.add_(dev(0.2 * rnd(gen, gn.num_channels))); gn.bias.add_(dev(0.2 * rnd(gen, gn.num_channels)))


def test_presplit_level0_double_conv(ops):
    """as test_presplit_route_of_a_level0_double_conv (1 -> 8 -> 16 @16^3, rf_conv3d_cin1_presplit -> rf_conv3d_split_pre_k3_relu), with its fused pool"""
    from model.unet import DoubleConv
    n = 2048
    gen = torch.Generator().manual_seed(131)
    src, fams = cnd.mixed(gen, n, 1, 16, 8)
    x = dev(src)
    torch.manual_seed(131)
    blk = DoubleConv(1, 16, encoder=True, num_groups=8).to(DEV)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if 'groupnorm.weight' in name:
                p.copy_(1.0 + 0.3 * rnd(gen, *p.shape))
            elif 'groupnorm.bias' in name:
                p.copy_(rnd(gen, *p.shape, scale=0.4))
            else:
                p.copy_(rnd(gen, *p.shape, scale=0.2))
    zero_first_group(blk.SingleConv1, blk.SingleConv2.groupnorm)

    def run(flag):
        saved, ops.USE_PRESPLIT = ops.USE_PRESPLIT, flag
        try:
            with torch.no_grad():
                return blk(x, pool='also')
        finally:
            ops.USE_PRESPLIT = saved

    with torch.no_grad():
        assert blk.route(x, pool='also') == 'cin1_presplit'
    fast, plain = run(True), run(False)
    idx, sub = subset(n, fams)
    ref = two_layers64(src[idx].double(), (blk.SingleConv1, blk.SingleConv2))
    for f, p_, r, nm in zip(fast, plain, (ref, F.max_pool3d(ref, 2)), ('full', 'pooled')):
        scale = p_.abs().max().item()
        assert (f - p_).abs().max().item() <= 2e-6 * scale, 'routes differ by %.2e' % ((f - p_).abs().max().item() / scale)
        cnd.per_sample_close(f[idx], r, 1e-5, sub, 'pre-split level-0 pair: ' + nm)
        rs = r.abs().max().item()
        ef, ep = (f[idx].cpu().double() - r).abs().max().item() / rs, (p_[idx].cpu().double() - r).abs().max().item() / rs
        assert ef <= max(2e-6, 1.5 * ep), 'pre-split route %.2e from float64, plain route %.2e' % (ef, ep)
        fused_stats_agree(ops, gen, f, 16, 8, 'pre-split level-0 pair: ' + nm)
        fused_stats_agree(ops, gen, p_, 16, 8, 'plain level-0 pair: ' + nm)
        sf, sp = f._rf_stats[0].sum(dim=2), p_._rf_stats[0].sum(dim=2)
        assert torch.allclose(sf, sp, rtol=1e-5, atol=1e-5)


def test_presplit_prepooled_handover(ops):
    """as test_prepooled_handover_between_the_first_two_levels: level 0 -> MaxPool3d(2) -> level 1 with the pooled tensor handed over pre-split"""
    from model.unet import UNet3D
    n = 2100
    torch.manual_seed(177)
    net = UNet3D(1, 16, f_maps=[16, 32, 64, 128], num_groups=8, num_levels=4, is_segmentation=False, remove_n_final_layers=1).to(DEV).eval()
    gen = torch.Generator().manual_seed(16)
    e0, e1 = net.encoders[0], net.encoders[1]
    for blk in (e0.basic_module, e1.basic_module):
        jitter_groupnorms(blk, gen)
        zero_first_group(blk.SingleConv1, blk.SingleConv2.groupnorm)
    src, fams = cnd.mixed(gen, n, 1, 16, 8)
    with torch.no_grad():
        assert e0.basic_module.route(dev(src), pool='only', next_block=e1.basic_module) == 'cin1_presplit_handed' and e1.basic_module.accepts_prepooled(n, 16, 8)
        outs = {}
        try:
            for flag in (True, False):
                ops.USE_PREPOOL = flag
                _, pooled = e0(dev(src), pool='only', next_block=e1.basic_module)
                assert isinstance(pooled, ops.PreSplit) == flag
                outs[flag] = e1(None, prepooled=pooled, pool='also')
        finally:
            ops.USE_PREPOOL = True
    idx, sub = subset(n, fams)
    x64 = two_layers64(src[idx].double(), (e0.basic_module.SingleConv1, e0.basic_module.SingleConv2))
    x64 = two_layers64(F.max_pool3d(x64, 2), (e1.basic_module.SingleConv1, e1.basic_module.SingleConv2))
    for k in (0, 1):
        a_, b_ = outs[True][k], outs[False][k]
        scale = float(b_.abs().max())
        assert (a_ - b_).abs().max().item() <= 2e-6 * max(1.0, scale), 'routes differ by %.2e of %.2f' % ((a_ - b_).abs().max().item(), scale)
        nm = ('level 1 output', 'its fused pool')[k]
        fused_stats_agree(ops, gen, a_, 32, 8, 'pre-pooled hand-over: ' + nm)
        fused_stats_agree(ops, gen, b_, 32, 8, 'fp32 pooled hand-over: ' + nm)
    cnd.per_sample_close(outs[True][0][idx], x64, 1e-5, sub, 'pre-pooled hand-over: level 1 output')
    cnd.per_sample_close(outs[True][1][idx], F.max_pool3d(x64, 2), 1e-5, sub, 'pre-pooled hand-over: its fused pool')


@pytest.mark.parametrize('n', [1030, 2100])                            # 1030: the persistent producer, linear order; 2100: parity-major hand-over
def test_presplit_decoder_pair(ops, n):
    """as test_presplit_route_of_a_decoder_conv_pair: StepDownDoubleConv 32 + 64 -> 56 -> 16 @8^3"""
    from model.unet import StepDownDoubleConv
    c0, c1, cmid, cout = 32, 64, 56, 16
    torch.manual_seed(n)
    blk = StepDownDoubleConv(c0 + c1, cout, encoder=False, num_groups=8).to(DEV).eval()
    assert blk.SingleConv1.conv.out_channels == cmid
    gen = torch.Generator().manual_seed(n + 3)
    jitter_groupnorms(blk, gen)
    zero_first_group(blk.SingleConv1, blk.SingleConv2.groupnorm)
    skip, low, fams = cnd.mixed_pair(gen, n, c0, c1, 8, 8)
    with torch.no_grad():
        assert blk.route(dev(skip), dev(low)) == ('decoder_presplit_pm' if n >= 2048 else 'decoder_presplit')
        assert ops.conv_up_split_presplit_pm_supported(dev(skip), dev(low), cmid, 8, cout) == (n >= 2048)
        got = blk(dev(skip), dev(low))
        try:
            ops.USE_PRESPLIT = False
            plain = blk(dev(skip), dev(low))
        finally:
            ops.USE_PRESPLIT = True
    idx, sub = subset(n, fams)
    x64 = two_layers64(torch.cat((skip[idx], F.interpolate(low[idx], scale_factor=2, mode='nearest')), 1).double(), (blk.SingleConv1, blk.SingleConv2))
    cnd.per_sample_close(got[idx], x64, 1e-5, sub, 'pre-split decoder pair')
    e_pre, e_plain = (got[idx].cpu().double() - x64).abs().max().item(), (plain[idx].cpu().double() - x64).abs().max().item()
    assert e_pre <= 1.5 * e_plain + 1e-7, (e_pre, e_plain)
    assert (got - plain).abs().max().item() <= 2e-6 * max(1.0, float(plain.abs().max()))
    fused_stats_agree(ops, gen, got, cout, 8, 'pre-split decoder pair (%s)' % ('parity-major' if n >= 2048 else 'linear'))
    fused_stats_agree(ops, gen, plain, cout, 8, 'plain decoder pair')


def test_presplit_decoder_pair_parity_major_equals_linear(ops):
    """as test_parity_major_handover_of_the_decoder_pair_equals_the_linear_one, through the ops"""
    n, c0, c1, cmid, cout, groups = 2100, 32, 64, 56, 16, 8
    gen = torch.Generator().manual_seed(277)
    skip, low, fams = cnd.mixed_pair(gen, n, c0, c1, 8, groups)
    g1w, g1b, w1 = layer_params(gen, c0 + c1, cmid)
    g2w, g2b, w2 = layer_params(gen, cmid, cout)
    w1[:cmid // groups] = 0.0
    dskip, dlow = dev(skip), dev(low)
    aff = ops.gn_affine(dskip, dlow, dev(g1w), dev(g1b), groups, 1e-5)
    wp1, wp2 = ops.pack_conv3_up_split_weight(dev(w1), c0), ops.pack_conv3_split_weight(dev(w2))
    assert ops.conv_up_split_presplit_pm_supported(dskip, dlow, cmid, groups, cout)
    lin = ops.conv3d_up_split_presplit(dskip, dlow, aff, wp1, cmid, dev(g2w), dev(g2b), groups, 1e-5)
    pm = ops.conv3d_up_split_presplit(dskip, dlow, aff, wp1, cmid, dev(g2w), dev(g2b), groups, 1e-5, parity_major=True)
    z, y, x = torch.meshgrid(torch.arange(8), torch.arange(8), torch.arange(8), indexing='ij')
    perm = (((z & 1) * 4 + (y & 1) * 2 + (x & 1)) * 64 + (z >> 1) * 16 + (y >> 1) * 4 + (x >> 1)).reshape(-1).to(DEV)
    lin5, pm5 = lin.view(n, cmid // 8, 2, 512, 16), pm.view(n, cmid // 8, 2, 512, 16)
    assert torch.equal(pm5[:, :, :, perm], lin5), 'parity-major bytes are not the linear bytes permuted'
    out_lin = ops.conv3d_split_pre_relu(lin, cmid, n, 8, wp2, cout)
    out_pm = ops.conv3d_split_pre_relu(pm, cmid, n, 8, wp2, cout, parity_major=True)
    assert torch.equal(out_lin, out_pm)
    fused_stats_agree(ops, gen, out_lin, cout, groups, 'pre-split decoder pair, linear consumer')
    fused_stats_agree(ops, gen, out_pm, cout, groups, 'pre-split decoder pair, parity-major consumer')
    # the producer's optional statistics output (per (sample, cout): sum and sum of squares of the ReLU'd conv output, the zeroed group included) against
    # the plain kernel's, as the existing test demands
    from rfuse import _lib
    lib = _lib.load()
    st_pm = torch.empty((n, cmid, 2), dtype=torch.float64, device=DEV)
    scratch = torch.empty_like(pm)
    p = lambda t_: t_.data_ptr() if t_ is not None else None
    dg2w, dg2b = dev(g2w), dev(g2b)
    _lib.check(lib.rf_conv3d_up_split_presplit_pm(p(dskip), c0, p(dlow), c1, n, 8, p(aff), p(wp1), cmid, p(dg2w), p(dg2b), groups, 1e-5, p(scratch), p(st_pm),
                                                  torch.cuda.current_stream().cuda_stream), 'rf_conv3d_up_split_presplit_pm')
    assert torch.equal(scratch, pm)
    plain1 = ops.conv3d_up_split_gn_relu(dskip, dlow, aff, wp1, cmid)
    ref_sum, ref_sq = plain1.double().sum(dim=(2, 3, 4)), (plain1.double() ** 2).sum(dim=(2, 3, 4))
    assert float(ref_sum[:, :cmid // groups].abs().max()) == 0.0 and float(st_pm[:, :cmid // groups].abs().max()) == 0.0       # the zeroed group
    assert (st_pm[..., 0] - ref_sum).abs().max().item() <= 1e-6 * ref_sum.abs().max().item()
    assert (st_pm[..., 1] - ref_sq).abs().max().item() <= 1e-6 * ref_sq.abs().max().item()
    idx, sub = subset(n, fams)
    x64 = torch.cat((skip[idx], F.interpolate(low[idx], scale_factor=2, mode='nearest')), 1).double()
    for gw, gb, w in ((g1w, g1b, w1), (g2w, g2b, w2)):
        x64 = F.relu(F.conv3d(F.group_norm(x64, groups, gw.double(), gb.double(), 1e-5), w.double(), padding=1))
    cnd.per_sample_close(out_pm[idx], x64, 1e-5, sub, 'pre-split decoder pair, parity-major')


@pytest.mark.parametrize('n', [1030, 2070])
def test_presplit_encoder_pair(ops, n):
    """as test_presplit_route_of_an_encoder_pair_on_whole_samples: 16 -> 16 -> 32 @8^3, fused pool; the routes bit-equal"""
    from model.unet import DoubleConv
    torch.manual_seed(121)
    blk = DoubleConv(16, 32, encoder=True, num_groups=8).to(DEV).eval()
    gen = torch.Generator().manual_seed(n + 4)
    jitter_groupnorms(blk, gen)
    zero_first_group(blk.SingleConv1, blk.SingleConv2.groupnorm)
    src, fams = cnd.mixed(gen, n, 16, 8, 8)
    x = dev(src)
    with torch.no_grad():
        assert all(blk.route(x, pool=pool) == 'box_presplit' for pool in (None, 'also', 'only'))
        outs = {}
        try:
            for flag in (True, False):
                ops.USE_PRESPLIT = flag
                outs[flag] = [blk(x), blk(x, pool='also'), blk(x, pool='only')]
        finally:
            ops.USE_PRESPLIT = True
    idx, sub = subset(n, fams)
    x64 = two_layers64(src[idx].double(), (blk.SingleConv1, blk.SingleConv2))
    cnd.per_sample_close(outs[True][0][idx], x64, 1e-5, sub, 'pre-split encoder pair')
    assert torch.equal(outs[True][0], outs[False][0])
    assert torch.equal(outs[True][1][0], outs[False][1][0]) and torch.equal(outs[True][1][1], outs[False][1][1])
    assert outs[True][2][0] is None and torch.equal(outs[True][2][1], outs[False][2][1])
    assert torch.equal(outs[True][1][1], F.max_pool3d(outs[True][0], 2))
    for flag, route in ((True, 'pre-split'), (False, 'plain')):
        o = outs[flag]
        for t, nm in ((o[0], 'full'), (o[1][0], 'full beside pooled'), (o[1][1], 'pooled'), (o[2][1], 'pooled only')):
            fused_stats_agree(ops, gen, t, 32, 8, '%s encoder pair: %s' % (route, nm))


@pytest.mark.parametrize('batch', [3, 5])
def test_final_decoder_head(ops, batch):
    """as test_final_decoder_head_in_the_conv_epilogue (nf = 16): two convs @64^3 from a 32^3 source, 1x1x1 conv + tanh in the second one's epilogue"""
    import model as rf_model
    nf = 16
    torch.manual_seed(nf + batch)
    dec = rf_model.Superresolution08FinalDecoder(nf, 'gcr').to(DEV).eval()
    gen = torch.Generator().manual_seed(18 + batch)
    families = ('near_constant', 'constant', 'big_mean') if batch == 3 else ('near_constant', 'saturated', 'spike', 'constant', 'big_mean')
    src, fams = cnd.mixed(gen, batch, nf, 32, 8, families)
    dc = dec.network[0].basic_module
    zero_first_group(dc.SingleConv1, dc.SingleConv2.groupnorm)
    x = dev(src)
    with torch.no_grad():
        y1 = dc.SingleConv1(None, x)
        assert ops.conv_split_pointwise_supported(y1, nf)
        fused, fused_df = dec(x), dec.forward_df(x, 0.375)
        y2 = dc.SingleConv2(y1)
        plain = ops.conv1x1_tanh(y2, dec.network[1].weight, dec.network[1].bias)
        plain_df = ops.conv1x1_tanh(y2, dec.network[1].weight, dec.network[1].bias, post_add=1.0, post_mul=0.375 / 2)
        assert torch.equal(fused, plain) and torch.equal(fused_df, plain_df)
        # the channel-interleaved hand-over between the two convs (taken from 2048 boxes on) changes the layout of the intermediate, not a bit of the result
        assert ops.conv_up_split_ch8_supported(x, nf, nf) == (batch >= 4)
        saved, ops.USE_CH8 = ops.USE_CH8, False
        try:
            assert torch.equal(dec(x), fused) and torch.equal(dec.forward_df(x, 0.375), fused_df)
        finally:
            ops.USE_CH8 = saved
        idx = list(range(batch))
        x64 = two_layers64(F.interpolate(src[idx].double(), scale_factor=2, mode='nearest'), (dc.SingleConv1, dc.SingleConv2))
        ref = torch.tanh(F.conv3d(x64, dec.network[1].weight.double().cpu(), dec.network[1].bias.double().cpu()))
    cnd.per_sample_close(fused[idx], ref, 1e-5, [fams[i] for i in idx], 'final decoder head')


# ------------------------------------------------------------------------------------------------------------------ backward

def gn_backward64(x, dxn, gamma, groups):
    x64 = x.double().requires_grad_(True)
    g64 = gamma.double().requires_grad_(True)
    b64 = torch.zeros_like(g64).requires_grad_(True)
    F.group_norm(x64, groups, g64, b64, 1e-5).backward(dxn.double())
    return x64.grad, g64.grad, b64.grad


@pytest.mark.parametrize('case', [(18, 16, 1, 8), (18, 64, 2, 8), (1030, 32, 4, 8), (18, 56, 8, 8), (18, 1, 16, 1), (9, 192, 4, 8), (4, 16, 64, 8)])
def test_gn_backward_against_float64(ops, case):
    """rf_gn_backward directly (only the two-stream bit-repeat check called it): dx per sample, dgamma / dbeta per tensor, 2e-4; once more with
    d xn arriving multiplied by 2^7 and the device scalar 2^-7 that takes the factor out again (rfuse/autograd.py: the scaled split data
    gradient); two calls return equal bits"""
    from rfuse import autograd as rfa
    n, c, edge, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 10)
    families = cnd.FAMILIES if n >= NF else ('near_constant', 'big_mean', 'saturated', 'constant')
    x, fams = cnd.mixed(gen, n, c, edge, groups, families)
    dxn = rnd(gen, n, c, edge, edge, edge)
    gamma = 1 + 0.3 * rnd(gen, c)
    rdx, rdg, rdb = gn_backward64(x, dxn, gamma, groups)
    xd, dd, gd = dev(x), dev(dxn), dev(gamma)
    dx, dg, db = rfa.gn_backward(xd, dd, gd, groups, 1e-5)
    cnd.per_sample_close(dx, rdx, 2e-4, fams, 'gn_backward: dx', floor=1e-30)
    cnd.tensor_close(dg, rdg, 2e-4, 'gn_backward: dgamma')
    cnd.tensor_close(db, rdb, 2e-4, 'gn_backward: dbeta')
    dx2, dg2, db2 = rfa.gn_backward(xd, dd, gd, groups, 1e-5)
    assert torch.equal(dx, dx2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    inv = torch.full((1,), 2.0 ** -7, device=DEV)
    sx, sg, sb = rfa.gn_backward(xd, dd * 2.0 ** 7, gd, groups, 1e-5, inv)
    cnd.per_sample_close(sx, rdx, 2e-4, fams, 'gn_backward, scaled d xn: dx', floor=1e-30)
    cnd.tensor_close(sg, rdg, 2e-4, 'gn_backward, scaled d xn: dgamma')
    cnd.tensor_close(sb, rdb, 2e-4, 'gn_backward, scaled d xn: dbeta')


def wgrad64(x, gamma, beta, groups, dz, cout):
    """float64 weight gradient of conv3(GroupNorm(x)) for the upstream gradient dz, in sample chunks (the im2col of a chunk stays small)"""
    cin = x.shape[1]
    dw = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64)
    for i in range(0, x.shape[0], 128):
        xn = F.group_norm(x[i:i + 128].double(), cnd.gn_groups(cin, groups), gamma.double(), beta.double(), 1e-5)
        dw += torch.nn.grad.conv3d_weight(xn, dw.shape, dz[i:i + 128].double(), padding=1)
    return dw


def wgrad_problem(ops, case, seed):
    from rfuse import autograd as rfa
    n, cin, edge, cout, groups = case
    gen = torch.Generator().manual_seed(sum(case) + seed)
    x, fams = cnd.mixed(gen, n, cin, edge, groups)
    gamma, beta = 1 + 0.2 * rnd(gen, cin), 0.2 * rnd(gen, cin)
    y, dy = rnd(gen, n, cout, edge, edge, edge).relu_(), rnd(gen, n, cout, edge, edge, edge)
    xd = dev(x)
    aff = ops.gn_affine(xd, None, dev(gamma), dev(beta), groups)
    return rfa, x, xd, aff, gamma, beta, dev(y), dev(dy)


@pytest.mark.parametrize('case', [(18, 8, 16, 16, 8), (18, 32, 4, 64, 8), (18, 6, 8, 12, 6)])
def test_conv3d_wgrad_against_float64(ops, case):
    """rf_conv3d_k3_wgrad directly (fp32 MFMA; the affine applied while staging): (n, cin, edge, cout, groups)"""
    rfa, x, xd, aff, gamma, beta, y, dy = wgrad_problem(ops, case, 11)
    dz = rfa.relu_backward(dy, y)
    assert torch.equal(dz, dy * (y > 0))
    dw = rfa.conv3d_wgrad(xd, aff, dz, case[3])
    cnd.tensor_close(dw, wgrad64(x, gamma, beta, case[4], dz.cpu(), case[3]), 2e-4, 'conv3d_wgrad (fp32 MFMA) %s' % (case,))
    assert torch.equal(dw, rfa.conv3d_wgrad(xd, aff, dz, case[3]))


@pytest.mark.parametrize('case', [(130, 8, 16, 16, 8), (1030, 16, 8, 32, 8), (1030, 32, 4, 64, 8)])
def test_conv3d_wgrad_split_against_float64(ops, case):
    """rf_conv3d_k3_wgrad_split directly, its scales built as ConvGnRelu.backward builds them"""
    from rfuse import _lib
    n, cin, edge, cout, groups = case
    assert _lib.load().rf_conv3d_k3_wgrad_split_supported(cin, cout, n, edge)
    rfa, x, xd, aff, gamma, beta, y, dy = wgrad_problem(ops, case, 12)
    dz, amax = rfa.relu_backward_amax(dy, y)
    _, scales = rfa.dz_scale(amax, n, cout)
    dw = rfa.conv3d_wgrad_split(xd, aff, dz, scales, cout)
    cnd.tensor_close(dw, wgrad64(x, gamma, beta, groups, dz.cpu(), cout), 2e-4, 'conv3d_wgrad_split %s' % (case,))
    assert torch.equal(dw, rfa.conv3d_wgrad_split(xd, aff, dz, scales, cout))


SINGLE_CONV_CASES = [
    # (n, c0, c1, edge, cout, groups[, stride of the quiet samples])
    (18, 8, 0, 16, 16, 8), (18, 1, 0, 16, 8, 8), (18, 16, 32, 8, 24, 8), (18, 64, 0, 2, 64, 8), (18, 64, 0, 1, 128, 8),
    # enough boxes for the split-operand routes
    (130, 8, 0, 16, 16, 8), (1030, 16, 0, 8, 32, 8), (1030, 32, 0, 4, 64, 8), (1030, 8, 8, 8, 40, 4),
    # every ninth sample's upstream gradient x 2^-12: the split data gradient scales dz by ONE power of two, a quiet sample beside loud ones must still meet its
    # own bar.  With nine families every ninth sample is relu_randn: once more with every tenth, which rotates the quiet sample through all the families
    (1030, 16, 0, 8, 32, 8, 9), (1030, 16, 0, 8, 32, 8, 10),
]


@pytest.mark.parametrize('case', SINGLE_CONV_CASES)
def test_single_conv_gradients_per_sample(ops, case):
    """as test_autograd_gpu.py:test_single_conv_gradients_match_float64_oracle with mixed inputs; dx is held to 2e-4 of EACH sample's own maximum (there the
    maximum over the batch divides: a near-constant sample's |dx| ~ 1e3 would leave the others checked to a few per cent), dW / dgamma / dbeta per tensor"""
    from model.unet import SingleConv
    quiet = case[6] if len(case) > 6 else 0
    case = case[:6]
    n, c0, c1, edge, cout, groups = case
    gen = torch.Generator().manual_seed(sum(case) + 13)
    cin = c0 + c1
    torch.manual_seed(200 + sum(case))                                   # the conv weight's default init, seeded
    layer = SingleConv(cin, cout, num_groups=groups)
    with torch.no_grad():
        layer.groupnorm.weight.copy_(1 + 0.3 * torch.randn(cin, generator=gen))
        layer.groupnorm.bias.copy_(0.3 * torch.randn(cin, generator=gen))
    layer.to(DEV)
    x0, x1, fams = cnd.mixed_pair(gen, n, c0, c1, edge, groups)
    r = torch.randn(n, cout, edge, edge, edge, generator=gen)
    if quiet:
        r[::quiet] *= 2.0 ** -12
    ins = [t.to(DEV).requires_grad_(True) if t is not None else None for t in (x0, x1)]
    y = layer(ins[0], ins[1])
    sd = {'p.groupnorm.weight': layer.groupnorm.weight.detach().cpu().double().requires_grad_(True),
          'p.groupnorm.bias': layer.groupnorm.bias.detach().cpu().double().requires_grad_(True),
          'p.conv.weight': layer.conv.weight.detach().cpu().double().requires_grad_(True)}
    o0 = x0.double().requires_grad_(True) if c0 else None
    o1 = x1.double().requires_grad_(True) if c1 else None
    parts = ([o0] if c0 else []) + ([F.interpolate(o1, scale_factor=2, mode='nearest')] if c1 else [])
    yo = refpath.single_conv_gcr(torch.cat(parts, 1), sd, 'p', groups)
    # an output within round-off of 0 can sit on different sides of the ReLU in fp32 and float64: no upstream gradient there, on either side; at most 4 per case
    flips = (y.detach().cpu() > 0) != (yo.detach() > 0)
    print('\n', case, 'ReLU flips:', int(flips.sum()))
    assert int(flips.sum()) <= 4
    r = r.masked_fill(flips, 0.0)
    (y * r.to(DEV)).sum().backward()
    (yo * r.double()).sum().backward()
    tag = 'SingleConv%s: ' % (' (every %dth sample quiet)' % quiet if quiet else '')
    cnd.per_sample_close(y, yo, 1e-5, fams, tag + 'y')
    if c0:
        cnd.per_sample_close(ins[0].grad, o0.grad, 2e-4, fams, tag + 'dx0', floor=1e-30)
    if c1:
        cnd.per_sample_close(ins[1].grad, o1.grad, 2e-4, fams, tag + 'dx1', floor=1e-30)
    cnd.tensor_close(layer.conv.weight.grad, sd['p.conv.weight'].grad, 2e-4, tag + 'dW %s' % (case,))
    cnd.tensor_close(layer.groupnorm.weight.grad, sd['p.groupnorm.weight'].grad, 2e-4, tag + 'dgamma %s' % (case,))
    cnd.tensor_close(layer.groupnorm.bias.grad, sd['p.groupnorm.bias'].grad, 2e-4, tag + 'dbeta %s' % (case,))


# ------------------------------------------------------------------------------------------------------------------ attention on degenerate rows

@pytest.mark.parametrize('mode,K,c', [(0, 4, 16), (1, 4, 16)])
def test_attention_block_on_degenerate_rows(ops, mode, K, c):
    """what constant patches produce: test_kernels_gpu.py:test_attention_block's set-up with 64 extra rows whose K retrieved patches are one tensor and 64
    whose query and patches are all zero.  Softmax: the weights of such a row are equal across K (1e-6) and the output within the existing 2e-3 of
    the oracle; Gumbel-hard: the arg-max is that of the noise alone."""
    from model.attention import AttentionBlock
    gen = torch.Generator().manual_seed(111 + K + c + mode)
    b, e, extra = 600, 2, 64
    with contextlib.redirect_stdout(io.StringIO()):
        blk = AttentionBlock(c, e, K, True, True, bool(mode), True, True)
    sd = {k: rnd(gen, *v.shape, scale=0.15) for k, v in blk.state_dict().items()}
    blk.load_state_dict(sd)
    blk.to(DEV)
    rows = b + 2 * extra
    x = rnd(gen, rows, c, e, e, e).relu_()
    p = rnd(gen, rows, K, c, e, e, e).relu_()
    p[:, 0] = x + 0.05 * rnd(gen, rows, c, e, e, e)
    same, zero = slice(b, b + extra), slice(b + extra, rows)
    p[same] = p[same][:, 1:2].expand(-1, K, -1, -1, -1, -1).clone()
    x[zero] = 0.0
    p[zero] = 0.0
    noise = -torch.empty(rows, K).exponential_(generator=gen).log() if mode else None
    det, dbg = {}, {}
    with torch.no_grad():
        ref = refpath.attention_block(x, p, {'a.' + k: v for k, v in sd.items()}, 'a', bool(mode), noise, det)
        got = blk(dev(x), dev(p), dev(noise), dbg)
    assert bool(torch.isfinite(got).all())
    wts = dbg['weights'].cpu().reshape(rows, K)
    for sl, nm in ((same, 'identical patches'), (zero, 'all-zero rows')):
        if mode:
            assert torch.equal(wts[sl].argmax(dim=1), noise[sl].argmax(dim=1)), nm + ': the arg-max is not that of the noise alone'
            assert float((got.cpu()[sl] - ref[sl]).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), nm
        else:
            assert float((wts[sl] - 1.0 / K).abs().max()) <= 1e-6, nm + ': softmax weights not equal across K'
            assert float((got.cpu()[sl] - ref[sl]).abs().max()) <= 2e-3 * max(1.0, float(ref.abs().max())), nm
    # the ordinary rows beside them: the existing bars
    sc_err = float((dbg['scores'].cpu().double() - det['scores'].double()).abs().max())
    assert sc_err <= 2e-6 * max(1.0, float(det['scores'].abs().max())), sc_err
    if mode:
        top2 = torch.topk(det['scores'] * 25 + noise, 2, dim=1).values
        safe = (top2[:, 0] - top2[:, 1]) > 1e-4
        assert safe.float().mean() > 0.99
        assert float((got.cpu()[safe] - ref[safe]).abs().max()) <= 1e-5 * max(1.0, float(ref[safe].abs().max()))
    else:
        assert float((got.cpu() - ref).abs().max()) <= 2e-3 * max(1.0, float(ref.abs().max()))
