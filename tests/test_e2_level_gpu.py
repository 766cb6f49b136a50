"""GPU: the retrieval backbone's 2^3 level as one launch (rf_conv3d_e2_level, csrc/conv3d_e2_level.hip, include/rfuse_level.h) against the six launches it
stands in for -- MaxPool3d(2), GroupNorm, conv, GroupNorm, conv and the decoder stage's GroupNorm table -- bit for bit, through the module that chooses
between them (model/unet.py:Encoder, rfuse.routes.level, the switch ops.USE_E2_LEVEL), and against float64 torch on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
import nonfinite
from rfuse import configs as rf_configs
from rfuse import synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C, CM, CO, GROUPS, C_SKIP = 64, 64, 128, 8, 64
E2_TOL = 1e-5          # the bar tests/test_kernels_gpu.py:test_conv3d_e2_split_gemm_form puts on rf_conv3d_e2_split_k3_gn_relu against float64 torch: tol * max(1, max |ref|)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU visible')
    from rfuse import ops as _ops
    return _ops


def make_level(cin, cout, seed, groups=GROUPS, c_skip=C_SKIP, dec_groups=GROUPS):
    """an Encoder level with pooling and the GroupNorm of the decoder stage that would read its output beside a c_skip-channel skip tensor; seeded parameters"""
    from model.unet import Encoder, GroupNormParams
    gen = torch.Generator().manual_seed(seed)
    enc = Encoder(cin, cout, apply_pooling=True, num_groups=groups)
    dec_gn = GroupNormParams(dec_groups, c_skip + cout)
    with torch.no_grad():
        for mod in (enc, dec_gn):
            for name, p in mod.named_parameters():
                if name.endswith('conv.weight'):
                    p.copy_(torch.randn(p.shape, generator=gen) / np.sqrt(8 * p.shape[1]))
                elif name.endswith('weight'):
                    p.copy_(1 + 0.2 * torch.randn(p.shape, generator=gen))
                else:
                    p.copy_(0.2 * torch.randn(p.shape, generator=gen))
    return enc.to(DEV), dec_gn.to(DEV)


def make_input(n, cin, seed):
    """N(0, 1) * 3 + 1; one all-constant sample (variance 0: the eps path), one sample offset by 1e3"""
    x = torch.randn(n, cin, 4, 4, 4, generator=torch.Generator().manual_seed(seed)) * 3 + 1
    x[3] = 2.5
    x[n - 2] += 1e3
    return x


def make_skip(ops, n, c_skip, seed):
    """a skip tensor [n, c_skip, 4^3] that carries its producer's statistics (here: the max-pool's)"""
    big = torch.rand(n, c_skip, 8, 8, 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    skip = ops.maxpool2(big)
    assert ops._fresh_stats(skip) is not None
    return skip


def run_level(ops, enc, dec_gn, x, skip, fused):
    """the level through its module with the form switched on / off -> (out, its statistics, the decoder table, did the one-launch form run)"""
    saved, ops.USE_E2_LEVEL = ops.USE_E2_LEVEL, fused
    try:
        with torch.no_grad():
            out = enc(x, consumer=None if skip is None else (skip, dec_gn))
            took = getattr(out, '_rf_ready_affine', None) is not None if skip is not None else None
            table = None if skip is None else ops.gn_affine(skip, out, dec_gn.weight, dec_gn.bias, dec_gn.num_groups, dec_gn.eps)
    finally:
        ops.USE_E2_LEVEL = saved
    return out, ops._fresh_stats(out)[0], table, took


@pytest.fixture(scope='module')
def level(ops):
    return make_level(C, CO, 11)


@pytest.mark.parametrize('n', [128, 129, 191])
def test_one_launch_is_bit_equal_to_the_six(ops, level, n):
    """n = 128: the bound of rf_conv3d_e2_level_supported (1024 (sample, group) units); 129, 191: a ragged last tile of 1 and of 31 samples"""
    from rfuse import _lib
    enc, dec_gn = level
    assert _lib.load_level().rf_conv3d_e2_level_supported(n, C, CM, CO, GROUPS, GROUPS, C_SKIP, 1, GROUPS) == 1
    x, skip = make_input(n, C, 100 + n).to(DEV), make_skip(ops, n, C_SKIP, 200 + n)
    out1, st1, tab1, took1 = run_level(ops, enc, dec_gn, x, skip, True)
    out6, st6, tab6, took6 = run_level(ops, enc, dec_gn, x, skip, False)
    assert took1 and not took6
    assert out1.shape == (n, CO, 2, 2, 2) and tab1.shape == (n, C_SKIP + CO, 4)
    assert torch.isfinite(out1).all()
    assert torch.equal(out1, out6), 'output'
    assert torch.equal(st1, st6), 'statistics'
    assert torch.equal(tab1, tab6), 'decoder table'
    # without a consumer the launch writes no table and the same output
    out0, st0, _, _ = run_level(ops, enc, None, x, None, True)
    assert torch.equal(out0, out6) and torch.equal(st0, st6)


def test_table_is_not_taken_for_other_parameters_or_modified_ones(ops):
    """the table rides on the output for exactly the tensors and parameters it was computed from"""
    enc, dec_gn = make_level(C, CO, 13)
    n = 128
    x, skip = make_input(n, C, 7).to(DEV), make_skip(ops, n, C_SKIP, 8)
    out, _, table, took = run_level(ops, enc, dec_gn, x, skip, True)
    assert took and out._rf_ready_affine[0] is table
    other = make_level(C, CO, 12)[1]
    with torch.no_grad():
        assert ops.gn_affine(skip, out, other.weight, other.bias, other.num_groups, other.eps) is not table
        dec_gn.bias.add_(1.0)
        fresh = ops.gn_affine(skip, out, dec_gn.weight, dec_gn.bias, dec_gn.num_groups, dec_gn.eps)
    assert fresh is not table and not torch.equal(fresh, table)


UNSUPPORTED = [
    # (n, cin, cout, groups, c_skip, dec_groups): why rf_conv3d_e2_level_supported says 0
    (127, 64, 128, 8, 64, 8),        # 127 * 8 = 1016 (sample, group) units: rf_gn_from_stats takes its 64-lane form, another summation order
    (512, 6, 12, 2, 64, 2),          # cin < 8 and no multiple of 4 (512 * 2 groups: the GroupNorm plans themselves would do)
    (512, 10, 20, 2, 64, 2),         # cin no multiple of 4
    (128, 64, 128, 8, 1952, 16),     # the decoder's 16 groups span (1952 + 128) / 16 = 130 > 128 statistics entries
]


@pytest.mark.parametrize('case', UNSUPPORTED)
def test_unsupported_plans_keep_the_six_launches(ops, case):
    from rfuse import _lib
    n, cin, cout, groups, c_skip, dec_groups = case
    enc, dec_gn = make_level(cin, cout, 21, groups=groups, c_skip=c_skip, dec_groups=dec_groups)
    cmid = enc.basic_module.SingleConv1.conv.out_channels
    assert _lib.load_level().rf_conv3d_e2_level_supported(n, cin, cmid, cout, groups, groups, c_skip, 1, dec_groups) == 0
    x, skip = make_input(n, cin, 5).to(DEV), make_skip(ops, n, c_skip, 6)
    assert enc.level_route(n, cin, 4, skip=(c_skip, 1, dec_groups)) == 'plain'
    out1, st1, tab1, took1 = run_level(ops, enc, dec_gn, x, skip, True)
    out6, st6, tab6, _ = run_level(ops, enc, dec_gn, x, skip, False)
    assert not took1
    assert torch.equal(out1, out6) and torch.equal(st1, st6) and torch.equal(tab1, tab6)


def test_entry_point_refuses_what_it_does_not_support(ops):
    """asked for directly, the launcher refuses before anything reaches the device"""
    x, one = torch.zeros(127, C, 4, 4, 4, device=DEV), torch.zeros(1, device=DEV)
    with pytest.raises(RuntimeError, match=r'^rf_conv3d_e2_level failed \(rc=-2\)'):
        ops.conv3d_e2_level(x, (one, one, GROUPS, 1e-5), one, CM, (one, one, GROUPS, 1e-5), one, CO)


def test_against_float64_torch(ops, level):
    enc, _ = level
    n = 129
    x = make_input(n, C, 31)
    out, _, _, _ = run_level(ops, enc, None, x.to(DEV), None, True)
    y = F.max_pool3d(x.double(), 2)
    for conv in (enc.basic_module.SingleConv1, enc.basic_module.SingleConv2):
        gn = conv.groupnorm
        y = F.group_norm(y, gn.num_groups, gn.weight.detach().cpu().double(), gn.bias.detach().cpu().double(), eps=gn.eps)
        y = F.relu(F.conv3d(y, conv.conv.weight.detach().cpu().double(), None, padding=1))
    err = (out.cpu().double() - y).abs().max().item()
    bound = E2_TOL * max(1.0, y.abs().max().item())
    print(f'\none-launch level vs float64 torch: max abs err {err:.3e}, bound {bound:.3e}')
    assert err <= bound


def test_nonfinite_input_stays_in_its_sample(ops, level):
    """one NaN and one +inf voxel in different samples (pattern of tests/nonfinite.py): the NaN masks of the six-launch route, every other sample bit-equal"""
    enc, dec_gn = level
    n = 129
    x = make_input(n, C, 41)
    x[5, 17, 1, 2, 3] = float('nan')
    x[70, 0, 0, 0, 0] = float('inf')
    x, skip = x.to(DEV), make_skip(ops, n, C_SKIP, 42)
    out1, st1, tab1, took = run_level(ops, enc, dec_gn, x, skip, True)
    out6, st6, tab6, _ = run_level(ops, enc, dec_gn, x, skip, False)
    assert took
    nonfinite.assert_bit_equal_nan(out1, out6, 'output')
    nonfinite.assert_bit_equal_nan(st1, st6, 'statistics')
    nonfinite.assert_bit_equal_nan(tab1, tab6, 'decoder table')
    hit = torch.isnan(out1).flatten(1).any(dim=1).cpu()
    assert hit.nonzero().flatten().tolist() == [5, 70]


def test_engine_runs_the_level_as_one_launch(ops, gpu):
    """RefinementEngine.refine at B = 2 on C2 (512 retrieved patches): the same df with the form on and off; the launch log shows the one entry point where
    the max-pool and the two 2^3 convs of the retrieval backbone's bottom level were"""
    from rfuse import _lib
    from rfuse.database import PatchDatabase
    from rfuse.engine import RefinementEngine
    cfg, B = rf_configs.get_config('C2'), 2
    db = synthetic.make_database(5, cfg, 64 * 30)
    eng = RefinementEngine(cfg, gpu, PatchDatabase(db['emb'], db['meta'], db['volumes'], gpu))
    sds = {}
    for name, m in eng.modules().items():
        sds[name] = helpers.seeded_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}, 77 + len(name))
    eng.load_state_dicts(sds)
    x = torch.from_numpy(np.stack([synthetic.make_chunk(4000 + b, cfg)['input_raw'] for b in range(B)])).to(gpu)
    rows = B * cfg['attn_num_patch'] ** 3
    n = B * cfg['K'] * 64                                        # the retrieval backbone's samples: K retrieved patches for each of the chunk's 64 patch positions
    assert n == 512
    noise = None
    if cfg['attn_retrieval_mode']:
        noise = (-torch.empty(rows, cfg['K']).exponential_(generator=torch.Generator().manual_seed(1)).log() * 4.0).to(gpu)

    def logged(fused):
        records, saved = [], ops.USE_E2_LEVEL
        ops.USE_E2_LEVEL = fused
        _lib.load().start_profile(records)
        _lib.load_level().start_profile(records)
        try:
            df = eng.refine(x, gumbel_noise=noise)
        finally:
            _lib.load_level().stop_profile()
            _lib.load().stop_profile()
            ops.USE_E2_LEVEL = saved
        bottom = [r[0] for r in records if (r[0].startswith('rf_maxpool3d_2') and r[1][:3] == (n, 64, 4))
                  or (r[0] == 'rf_conv3d_e2_split_k3_gn_relu' and r[1][1] == n and r[1][2] == 2)]
        return df, [r[0] for r in records].count('rf_conv3d_e2_level'), bottom
    eng.refine(x, gumbel_noise=noise)                             # packs, range checks
    df1, level_calls1, bottom1 = logged(True)
    df6, level_calls6, bottom6 = logged(False)
    assert (level_calls1, bottom1) == (1, [])
    assert level_calls6 == 0 and sorted(bottom6) == ['rf_conv3d_e2_split_k3_gn_relu'] * 2 + ['rf_maxpool3d_2_stats']
    assert torch.isfinite(df1).all() and torch.equal(df1, df6)
