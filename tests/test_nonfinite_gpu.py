"""Non-finite parity of the forward kernels: a NaN or an infinity in the input reaches exactly the outputs it reaches in the float64
reference, and nothing else moves.

Every case runs an op twice on the same inputs, once clean and once with a few voxels replaced by NaN (or +-inf), with the GroupNorm affine
taken from the CLEAN input so that only the dependency cone of the injected voxels is affected.  Checked: the float64 torch reference marks
exactly the combinatorial cone (tests/nonfinite.py; catches a reference that skips products by zero), the kernel's NaN mask equals the
reference's, the poisoned samples are bit-equal to the clean run outside the cone, every other sample is bit-equal to the clean run
(fused statistics included), and the poisoned samples' fused statistics are non-finite.  The injected voxels sit where kernels go wrong:
box and halo borders of 16^3 / 64^3 samples, the ragged last workgroup, samples that share a workgroup with others (4^3 / 2^3 forms)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nonfinite import (assert_bit_equal_nan, assert_close_finite, assert_close_nonfinite, cone_conv, cone_pool2, cone_up2, point_mask)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU visible')
    from rfuse import ops as _ops
    return _ops


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).float()


def weight(gen, cout, cin, k=3, fan=None):
    w = rnd(gen, cout, cin, k, k, k, scale=1.0 / np.sqrt((fan or k ** 3) * cin))
    w[w == 0] = 1e-3                                            # no exact zeros: NaN * w must stay NaN in every product
    return w


def voxel(edge, which):
    """injected voxel of a sample: a corner, or one whose 3^3 cone crosses 8^3 box borders (and, for 64^3, the far face)"""
    if edge == 1:
        return (0, 0, 0)
    if which == 0:
        return (0, edge - 1, 0)
    return (min(7, edge - 1), min(8, edge - 1), edge - 1)


def poisoned_samples(n):
    """the last sample (the ragged last workgroup) and one inside a workgroup shared with other samples (8 / 64 per workgroup in the 4^3 / 2^3 forms)"""
    return sorted({n - 1, min(n - 1, 9)}) if n > 1 else [0]


def ref_gcr(src0, src1, aff, w, floor=True):
    """float64: ReLU(conv3(GN(cat(src0, up2(src1))))) with the GroupNorm given as the kernels' affine (centre, scale, shift)"""
    parts = [t for t in (src0, F.interpolate(src1, scale_factor=2, mode='nearest') if src1 is not None else None) if t is not None]
    x = torch.cat(parts, 1).double()
    a = aff.double()
    x = (x - a[..., 0, None, None, None]) * a[..., 1, None, None, None] + a[..., 2, None, None, None]
    y = F.conv3d(x, w.double(), None, padding=1)
    return F.relu(y) if floor else y


def inject(srcs, points, value):
    """copies of the sources with value at the (source, sample, channel, z, y, x) points; +-value alternating between points"""
    out = [s.clone() if s is not None else None for s in srcs]
    for i, (si, *p) in enumerate(points):
        out[si][tuple(p)] = value if (i % 2 == 0 or value != value) else -value
    return out


def check_poisoned(name, got_bad, got_clean, ref, cone, kind, tol):
    """one output of one poisoned sample [1, C, ...]: see the module docstring.  kind 'nan': masks equal.  kind 'inf': the split forms carry
    v - hi, which is NaN for an infinite v, so the NaN-versus-infinity kind is deliberately not asserted -- only that every position non-finite
    in the reference is non-finite in the output, and that any extra non-finite output lies inside the cone"""
    ref_nf = ~torch.isfinite(ref)
    if kind == 'inf-presummed':
        # the parity-split fp32 decoder kernel convolves the low-resolution source with taps summed in advance: inf * (w_a + w_b) is +-inf where the
        # reference's inf * w_a + inf * w_b is NaN, and ReLU(-inf) is 0.  Only the cone is asserted for an infinite low-resolution voxel
        assert not (~torch.isfinite(got_bad.cpu()) & ~cone).any(), f'{name}: non-finite outputs outside the cone'
    elif kind == 'nan':
        assert torch.equal(torch.isnan(ref), cone), f'{name}: the float64 reference does not mark exactly the dependency cone'
        assert_close_nonfinite(got_bad, ref, tol, name)
    else:
        assert (ref_nf & ~cone).sum() == 0, f'{name}: reference non-finite outside the cone'
        got_nf = ~torch.isfinite(got_bad.cpu())
        assert not (ref_nf & ~got_nf).any(), f'{name}: {int((ref_nf & ~got_nf).sum())} positions non-finite in the reference are finite in the output'
        assert not (got_nf & ~cone).any(), f'{name}: non-finite outputs outside the cone'
        both = ~got_nf & ~ref_nf
        assert_close_finite(got_bad.cpu(), ref, both, tol, name)
    outside = ~cone
    assert_bit_equal_nan(got_bad.cpu()[outside], got_clean.cpu()[outside], name + ' outside the cone vs the clean run')


def run_case(run, srcs, points, value, ref_fn, cone_fn, tol, presummed=False):
    """run(device sources) -> {name: tensor}; tensors with fused statistics also give '<name>.stats' ([n, C, tiles, 2] float64).
    ref_fn(sources of one sample, float64) -> {name: float64}; cone_fn(masks of the sources of one sample) -> {name: bool}."""
    kind = 'nan' if value != value else ('inf-presummed' if presummed else 'inf')
    dev = lambda ss: [s.to(DEV) if s is not None else None for s in ss]
    clean = {k: v.cpu() for k, v in run(dev(srcs)).items()}
    bad_srcs = inject(srcs, points, value)
    bad = {k: v.cpu() for k, v in run(dev(bad_srcs)).items()}
    n = next(s for s in srcs if s is not None).shape[0]
    poisoned = sorted({p[1] for p in points})
    others = torch.tensor([i for i in range(n) if i not in poisoned], dtype=torch.long)
    for k in clean:
        assert_bit_equal_nan(bad[k][others], clean[k][others], f'{k}: samples without an injected voxel vs the clean run')
        if k.endswith('.stats'):
            for smp in poisoned:
                s = bad[k][smp].sum(dim=1)                                    # [C, 2] over the tiles
                hit = (~torch.isfinite(bad[k[:-len('.stats')]][smp])).flatten(1).any(dim=1)
                assert not torch.isfinite(s[hit]).all(dim=1).any(), \
                    f'{k}: fused statistics of poisoned sample {smp} stay finite in a channel with non-finite outputs'
    for smp in poisoned:
        one = [s[smp:smp + 1] if s is not None else None for s in bad_srcs]
        masks = [point_mask((1,) + tuple(s.shape[1:]), [(0,) + tuple(p[2:]) for p in points if p[0] == si and p[1] == smp]) if s is not None else None
                 for si, s in enumerate(srcs)]
        refs, cones = ref_fn(one), cone_fn(masks)
        for k, ref in refs.items():
            check_poisoned(f'{k} (sample {smp})', bad[k][smp:smp + 1], clean[k][smp:smp + 1], ref, cones[k], kind, tol)


def _stats(d, k, t):
    d[k] = t
    st = getattr(t, '_rf_stats', None)
    if st is not None:
        d[k + '.stats'] = st[0]
    return d


def gcr_points(srcs, n):
    pts = []
    for j, smp in enumerate(poisoned_samples(n)):
        si = j % len([s for s in srcs if s is not None])
        si = [i for i, s in enumerate(srcs) if s is not None][si]
        c, e = srcs[si].shape[1], srcs[si].shape[2]
        pts.append((si, smp, (3 * j + 1) % c) + voxel(e, j))
    return pts


def gcr_case(ops, case, seed, value, runner, pool=False, tol=2e-5, presummed=False):
    """a GroupNorm-conv-ReLU form on (src0, src1): runner(ops, d0, d1, aff, w_dev, cout) -> {name: tensor}; outputs 'out' and, with pool, 'pooled'"""
    n, c0, c1, edge, cout, groups = case
    gen = torch.Generator().manual_seed(seed)
    src0 = rnd(gen, n, c0, edge, edge, edge).relu_() if c0 else None
    src1 = rnd(gen, n, c1, edge // 2, edge // 2, edge // 2).relu_() if c1 else None
    cin = c0 + c1
    gamma, beta = 1 + 0.2 * rnd(gen, cin), 0.2 * rnd(gen, cin)
    w = weight(gen, cout, cin)
    aff = ops.gn_affine(src0.to(DEV) if c0 else None, src1.to(DEV) if c1 else None, gamma.to(DEV), beta.to(DEV), groups)
    aff_cpu, wd = aff.cpu(), w.to(DEV)
    srcs = [src0, src1]
    points = gcr_points(srcs, n)
    order = iter(sorted({p[1] for p in points}))              # run_case asks for the references of the poisoned samples in this order

    def ref_fn(one):
        smp = next(order)
        y = ref_gcr(one[0], one[1], aff_cpu[smp:smp + 1], w)
        if pool == 'only':
            return {'pooled': F.max_pool3d(y, 2)}
        return {'out': y, 'pooled': F.max_pool3d(y, 2)} if pool else {'out': y}

    def cone_fn(masks):
        m = [masks[0], cone_up2(masks[1]) if masks[1] is not None else None]
        cone = cone_conv(torch.cat([t for t in m if t is not None], 1), cout)
        if pool == 'only':
            return {'pooled': cone_pool2(cone)}
        return {'out': cone, 'pooled': cone_pool2(cone)} if pool else {'out': cone}
    run_case(lambda ds: runner(ops, ds[0], ds[1], aff.clone(), wd, cout), srcs, points, value, ref_fn, cone_fn, tol,
             presummed=presummed and any(p[0] == 1 for p in points))


# ---- GroupNorm-conv-ReLU forms ------------------------------------------------------------------------------------------------------

def _run_direct(ops, d0, d1, aff, wd, cout):
    return {'out': ops.conv3d_gn_relu(d0, d1, aff, None, cout, direct_weight=wd)}


def _run_mfma(ops, d0, d1, aff, wd, cout):
    return _stats({}, 'out', ops.conv3d_gn_relu(d0, d1, aff, ops.pack_conv3_weight(wd), cout))


GCR_CASES = [
    # (n, c0, c1, edge, cout, groups)
    (3, 8, 0, 8, 16, 8),
    (1, 16, 0, 16, 32, 8),       # several 8^3 tiles per sample: the cone crosses tile borders
    (2, 32, 64, 8, 56, 8),       # decoder read: skip + upsampled
    (1, 0, 32, 16, 32, 8),       # upsampled source only
    (12, 16, 0, 4, 32, 8),       # 4^3 volumes, 8 per workgroup, partial last workgroup
    (70, 64, 0, 2, 128, 8),      # 2^3 volumes, 64 per workgroup
    (4, 64, 0, 1, 128, 8),       # 1^3 -> direct path
    (1, 6, 0, 8, 12, 6),         # nf = 12
    (4099, 16, 0, 4, 16, 8),     # position-major small-volume form
    (32770, 64, 0, 2, 16, 8),    # ... 2^3, 64 samples per workgroup
    (530, 56, 0, 8, 16, 8),
]


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', GCR_CASES)
def test_conv3d_gn_relu_nonfinite(ops, case, value):
    n, c0, c1, edge = case[:4]
    if edge == 1 or n <= 4:
        gcr_case(ops, case, sum(case) + 1, value, _run_direct)
    if edge >= 2:
        gcr_case(ops, case, sum(case) + 2, value, _run_mfma)


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', [(300, 8, 0, 16, 16, 8), (2, 16, 0, 64, 16, 8), (2100, 16, 0, 4, 16, 8), (130, 6, 0, 16, 12, 6)])
def test_conv3d_gn_relu_pool_nonfinite(ops, case, value):
    """the fused MaxPool3d(2) epilogue: pooled NaN mask = F.max_pool3d's, with and without the full-resolution output"""
    def run_full(ops, d0, d1, aff, wd, cout):
        assert ops.conv_pool_supported(d0, d1, cout)
        full, pooled = ops.conv3d_gn_relu_pool(d0, d1, aff, ops.pack_conv3_weight(wd), cout, keep_full=True)
        return _stats(_stats({}, 'out', full), 'pooled', pooled)

    def run_only(ops, d0, d1, aff, wd, cout):
        none, pooled = ops.conv3d_gn_relu_pool(d0, d1, aff, ops.pack_conv3_weight(wd), cout, keep_full=False)
        assert none is None
        return _stats({}, 'pooled', pooled)
    gcr_case(ops, case, sum(case) + 3, value, run_full, pool=True)
    gcr_case(ops, case, sum(case) + 3, value, run_only, pool='only')


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', [(256, 32, 64, 8, 56, 8), (300, 0, 16, 8, 16, 8), (1027, 64, 128, 4, 64, 8), (2, 0, 16, 64, 16, 8), (40, 6, 12, 16, 12, 6)])
def test_conv3d_up_gn_relu_nonfinite(ops, case, value):
    """the parity-split fp32 decoder kernel: a low-resolution voxel reaches a 4^3 block of outputs"""
    def run(ops, d0, d1, aff, wd, cout):
        assert ops.conv_up_supported(d0, d1, cout)
        return _stats({}, 'out', ops.conv3d_up_gn_relu(d0, d1, aff, ops.pack_conv3_up_weight(wd, case[1]), cout))
    gcr_case(ops, case, sum(case) + 4, value, run, presummed=True)


SPLIT_CASES = [
    # (n, cin, edge, cout, groups) of rf_conv3d_split_k3_gn_relu's forms
    (130, 8, 16, 16, 8),       # box kernel, halos from neighbouring boxes
    (1030, 8, 8, 16, 8),       # whole 8^3 volumes, ragged sample count
    (2100, 24, 8, 12, 6),      # persistent z-column form (zcm), nf = 12
    (5, 16, 64, 16, 8),        # 64^3 samples, 2560 boxes
    (2050, 12, 8, 12, 6),      # zero slots of the last channel chunk
    (1030, 32, 4, 64, 8),      # whole 4^3 samples, 8 per workgroup (s4)
    (1030, 24, 4, 48, 6),
    (16, 24, 32, 48, 6),       # more than 32 couts: cout blocks on grid.y
    (9, 16, 32, 40, 4),
]


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', SPLIT_CASES)
def test_conv3d_split_gn_relu_nonfinite(ops, case, value):
    """the split-operand box / zc / zcm / s4 / grid.y forms, with pool None, 'also' and 'only'"""
    n, cin, edge, cout, groups = case
    gcase = (n, cin, 0, edge, cout, groups)

    def run_none(ops, d0, d1, aff, wd, cout):
        assert ops.conv_split_supported(d0, None, cout)
        return _stats({}, 'out', ops.conv3d_split_gn_relu(d0, aff, ops.pack_conv3_split_weight(wd), cout))

    def run_also(ops, d0, d1, aff, wd, cout):
        full, pooled = ops.conv3d_split_gn_relu(d0, aff, ops.pack_conv3_split_weight(wd), cout, pool='also')
        return _stats(_stats({}, 'out', full), 'pooled', pooled)

    def run_only(ops, d0, d1, aff, wd, cout):
        none, pooled = ops.conv3d_split_gn_relu(d0, aff, ops.pack_conv3_split_weight(wd), cout, pool='only')
        assert none is None
        return _stats({}, 'pooled', pooled)
    gcr_case(ops, gcase, sum(case) + 5, value, run_none, tol=1e-5)
    gcr_case(ops, gcase, sum(case) + 6, value, run_also, pool=True, tol=1e-5)
    gcr_case(ops, gcase, sum(case) + 7, value, run_only, pool='only', tol=1e-5)


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', [(1030, 64, 128, 8, 2), (260, 8, 6, 4, 2), (32, 64, 128, 8, 1), (300, 72, 40, 8, 1)])
def test_conv3d_e2_split_gn_relu_nonfinite(ops, case, value):
    """whole 2^3 / 1^3 volumes as one dense GEMM: a sample is a GEMM column beside the others of its workgroup"""
    n, cin, cout, groups, edge = case

    def run(ops, d0, d1, aff, wd, cout):
        assert ops.conv_e2_split_supported(d0, cout)
        return _stats({}, 'out', ops.conv3d_e2_split_gn_relu(d0, aff, ops.pack_conv3_e2_split_weight(wd, edge), cout))
    gcr_case(ops, (n, cin, 0, edge, cout, groups), sum(case) + 8, value, run, tol=1e-5)


SPLIT_UP_CASES = [
    (256, 32, 64, 8, 56, 8),    # the dominant decoder launch of C1-C4
    (300, 24, 48, 8, 42, 6),
    (1030, 64, 128, 4, 64, 8),  # whole 4^3 samples (s4), ragged
    (4, 0, 16, 64, 16, 8),      # boxes of a 64^3 volume, no skip source
    (16, 48, 96, 32, 78, 6),    # boxes with a skip source
    (2, 24, 48, 64, 24, 6),
    (70, 8, 8, 16, 20, 4),
]


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', SPLIT_UP_CASES)
def test_conv3d_up_split_gn_relu_nonfinite(ops, case, value):
    def run(ops, d0, d1, aff, wd, cout):
        assert ops.conv_up_split_supported(d0, d1, cout)
        return _stats({}, 'out', ops.conv3d_up_split_gn_relu(d0, d1, aff, ops.pack_conv3_up_split_weight(wd, case[1]), cout))
    gcr_case(ops, case, sum(case) + 9, value, run, tol=1e-5)


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', [(5, 16, 64, 16), (300, 8, 16, 8), (37, 16, 32, 8)])
def test_conv3d_up_split_ch8_nonfinite(ops, case, value):
    """the channel-interleaved (persistent) decoder box form"""
    n, c1, edge, cout = case
    from rfuse import _lib

    def run(ops, d0, d1, aff, wd, cout):
        assert _lib.load().rf_conv3d_up_split_ch8_supported(0, c1, n, edge, cout)
        got, stats, tiles = ops.conv3d_up_split_gn_relu_ch8(d1, aff, ops.pack_conv3_up_split_weight(wd, 0), cout)
        return {'out': got.permute(0, 1, 5, 2, 3, 4).reshape(n, cout, edge, edge, edge), 'out.stats': stats}
    gcr_case(ops, (n, 0, c1, edge, cout, 8 if c1 % 8 == 0 else 1), sum(case) + 10, value, run, tol=1e-5)


# ---- pools, 1x1 head, valid convs, linear ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('shape', [(3, 5, 8), (67, 5, 2), (130, 24, 4), (33, 7, 8), (3, 2, 16), (2, 3, 32)])
def test_maxpool2_nonfinite(ops, shape, value):
    """stand-alone MaxPool3d(2): F.max_pool3d's result bit for bit, NaN mask included; statistics of the other samples unmoved"""
    n, c, e = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = rnd(gen, n, c, e, e, e)
    points = [(0, smp, j % c) + voxel(e, j) for j, smp in enumerate(poisoned_samples(n))]

    def run(ds):
        return _stats({}, 'pooled', ops.maxpool2(ds[0]))
    run_case(run, [x], points, value, lambda one: {'pooled': F.max_pool3d(one[0].double(), 2)},
             lambda m: {'pooled': cone_pool2(m[0])}, 0.0)


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
def test_conv1x1_tanh_nonfinite(ops, value):
    gen = torch.Generator().manual_seed(8)
    x = rnd(gen, 3, 16, 16, 16, 16)
    w, b = rnd(gen, 1, 16, 1, 1, 1, scale=0.3), rnd(gen, 1)
    w[w == 0] = 1e-3
    points = [(0, 2, 5, 0, 15, 7), (0, 0, 1, 8, 7, 15)]
    run_case(lambda ds: {'out': ops.conv1x1_tanh(ds[0], w.to(DEV), b.to(DEV))}, [x], points, value,
             lambda one: {'out': torch.tanh(F.conv3d(one[0].double(), w.double(), b.double()))},
             lambda m: {'out': m[0].any(1, keepdim=True)}, 1e-6)


VALID_FORMS = {
    'gather': lambda ops, xd, w, b, cout, k, s, st: ops.conv3d_valid_leaky(xd, w, b, st, 0.2),
    'mfma': lambda ops, xd, w, b, cout, k, s, st: ops.conv3d_valid_leaky_mfma(xd, ops.pack_convv_weight(w), b, cout, k, st, 0.2),
    'lds': lambda ops, xd, w, b, cout, k, s, st: ops.conv3d_valid_leaky_lds(xd, ops.pack_convv_lds_weight(w), b, cout, k, st, 0.2),
    'valu': lambda ops, xd, w, b, cout, k, s, st: ops.conv3d_valid_leaky_valu(xd, ops.pack_convv_valu_weight(w), b, st, 0.2),
    'split': lambda ops, xd, w, b, cout, k, s, st: ops.conv3d_valid_leaky_split(xd, ops.pack_convv_split_weight(w, s, st), b, cout, k, st, 0.2),
}
VALID_CASES = [('gather', (3, 1, 8, 16, 3, 1)), ('gather', (2, 4, 12, 8, 3, 2)), ('mfma', (2, 12, 13, 24, 3, 1)), ('mfma', (3, 24, 11, 48, 3, 2)),
               ('lds', (2, 12, 44, 24, 3, 1)), ('lds', (3, 48, 20, 48, 3, 2)), ('valu', (3, 1, 48, 12, 5, 1)), ('valu', (2, 12, 22, 24, 3, 1)),
               ('split', (2, 12, 44, 24, 3, 1)), ('split', (3, 48, 20, 48, 3, 2)), ('split', (3, 8, 17, 96, 3, 1))]


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('form,spec', VALID_CASES)
def test_conv3d_valid_leaky_nonfinite(ops, form, spec, value):
    """the patch encoders' valid conv + bias + LeakyReLU forms: a voxel reaches the k^3 / stride window of outputs"""
    n, cin, s, cout, k, stride = spec
    gen = torch.Generator().manual_seed(sum(spec) + 12)
    x, w, b = rnd(gen, n, cin, s, s, s), weight(gen, cout, cin, k), rnd(gen, cout)
    wd, bd = w.to(DEV), b.to(DEV)
    points = [(0, smp, (2 * j + 1) % cin, s // 2, s - 1 - j, (j * 5) % s) for j, smp in enumerate(poisoned_samples(n))]
    run_case(lambda ds: {'out': VALID_FORMS[form](ops, ds[0], wd, bd, cout, k, s, stride)}, [x], points, value,
             lambda one: {'out': F.leaky_relu(F.conv3d(one[0].double(), w.double(), b.double(), stride=stride), 0.2)},
             lambda m: {'out': cone_conv(m[0], cout, k, stride, 0)}, 1e-5)


@pytest.mark.parametrize('value', [NAN, INF], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', [(1000, 128, 32, 0), (64, 64, 128, 1), (130, 512, 256, 1), (37, 96, 128, 2), (5, 7, 3, 1)])
def test_linear_nonfinite(ops, case, value):
    """a NaN input component makes its whole output row NaN whatever the activation (ReLU included)"""
    rows, nin, nout, act = case
    gen = torch.Generator().manual_seed(rows + nin + 13)
    x, w, b = rnd(gen, rows, nin), rnd(gen, nout, nin, scale=1 / np.sqrt(nin)), rnd(gen, nout)
    w[w == 0] = 1e-3
    wp = ops.pack_linear_weight(w.to(DEV))
    bad = x.clone()
    poisoned = poisoned_samples(rows)
    for j, r in enumerate(poisoned):
        bad[r, (7 * j + 3) % nin] = value if j % 2 == 0 or value != value else -value
    clean = ops.linear(x.to(DEV), wp, b.to(DEV), nout, act, 0.01).cpu()
    got = ops.linear(bad.to(DEV), wp, b.to(DEV), nout, act, 0.01).cpu()
    ref = F.linear(bad.double(), w.double(), b.double())
    ref = F.relu(ref) if act == 1 else (F.leaky_relu(ref, 0.01) if act == 2 else ref)
    others = [r for r in range(rows) if r not in poisoned]
    assert_bit_equal_nan(got[others], clean[others], 'linear: rows without an injected value')
    for r in poisoned:
        if value != value:
            assert torch.isnan(ref[r]).all()
            assert_close_nonfinite(got[r], ref[r], 1e-5, f'linear row {r}')
        else:
            assert not (~torch.isfinite(ref[r]) & torch.isfinite(got[r])).any(), f'linear row {r}: reference non-finite, output finite'


def test_l2_normalize_rows_nonfinite(ops):
    """F.normalize: a row with a NaN is NaN throughout (its norm is NaN and clamp_min keeps it); the other rows unmoved"""
    gen = torch.Generator().manual_seed(5)
    x = rnd(gen, 77, 64)
    x[3] = 0
    bad = x.clone()
    bad[10, 5] = NAN
    bad[76, 63] = NAN
    clean = ops.l2_normalize_rows_(x.clone().to(DEV)).cpu()
    got = ops.l2_normalize_rows_(bad.clone().to(DEV)).cpu()
    ref = F.normalize(bad.double(), dim=1)
    assert_close_nonfinite(got, ref, 1e-6, 'normalize')
    keep = [r for r in range(77) if r not in (10, 76)]
    assert_bit_equal_nan(got[keep], clean[keep], 'normalize: rows without a NaN')


# ---- module level -------------------------------------------------------------------------------------------------------------------

def test_single_conv_nan_weight_takes_the_fp32_route_and_stays_nan(ops):
    """one NaN weight in one output channel: ops.split_range_ok sends the layer to the fp32 kernels (NaN compares False), and that channel is NaN
    wherever the reference's is -- the ReLU no longer turns it into zeros.  The other channels are bit-equal to the clean layer's fp32 route."""
    from model.unet import SingleConv
    gen = torch.Generator().manual_seed(21)
    n, cin, edge, cout = 3, 16, 16, 32
    m = SingleConv(cin, cout, num_groups=8).to(DEV).requires_grad_(False)
    with torch.no_grad():
        m.groupnorm.weight.copy_(1 + 0.2 * rnd(gen, cin))
        m.groupnorm.bias.copy_(0.2 * rnd(gen, cin))
        m.conv.weight.copy_(weight(gen, cout, cin))
    x = rnd(gen, n, cin, edge, edge, edge).relu_()
    saved = ops.CONV_ARITH
    try:
        ops.CONV_ARITH = 'fp32'
        clean = m(x.to(DEV)).cpu()
    finally:
        ops.CONV_ARITH = saved
    with torch.no_grad():
        m.conv.weight[5, 3, 1, 1, 1] = NAN                     # the centre tap: every output reads a real voxel through it
    assert not ops.split_range_ok(m.conv.weight, m.groupnorm.weight, m.groupnorm.bias, (cin // 8) * edge ** 3)
    got = m(x.to(DEV)).cpu()
    ref = F.relu(F.conv3d(F.group_norm(x.double(), 8, m.groupnorm.weight.cpu().double(), m.groupnorm.bias.cpu().double(), 1e-5),
                          m.conv.weight.cpu().double(), None, padding=1))
    assert torch.isnan(ref[:, 5]).all() and not torch.isnan(ref[:, torch.arange(cout) != 5]).any()
    assert_close_nonfinite(got, ref, 2e-5, 'SingleConv with a NaN weight')
    keep = torch.arange(cout) != 5
    assert_bit_equal_nan(got[:, keep], clean[:, keep], 'SingleConv: the channels without the NaN weight vs the clean fp32 route')


@pytest.mark.parametrize('cls_name,n,cin,cout,edge', [('SingleConv', 1030, 8, 16, 8), ('SingleConv', 4, 16, 32, 16), ('DoubleConv', 1030, 8, 16, 8)])
def test_modules_with_data_derived_groupnorm_isolate_a_nan_sample(ops, cls_name, n, cin, cout, edge):
    """the GroupNorm statistics come from the data: a NaN voxel makes its whole sample NaN (as F.group_norm does), every other sample is bit-equal
    to the clean run"""
    from model import unet
    gen = torch.Generator().manual_seed(n + cin)
    if cls_name == 'SingleConv':
        m = unet.SingleConv(cin, cout, num_groups=8)
    else:
        m = unet.DoubleConv(cin, cout, encoder=True, num_groups=8)
    m = m.to(DEV).requires_grad_(False)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if 'groupnorm.weight' in name:
                p.copy_(1 + 0.2 * rnd(gen, p.numel()))
            elif 'groupnorm.bias' in name:
                p.copy_(0.2 * rnd(gen, p.numel()))
            else:
                p.copy_(weight(gen, p.shape[0], p.shape[1]))
    x = rnd(gen, n, cin, edge, edge, edge).relu_()
    clean = m(x.to(DEV)).cpu()
    bad = x.clone()
    bad[n - 1, cin - 1, 0, edge - 1, 3] = NAN
    got = m(bad.to(DEV)).cpu()
    assert torch.isnan(got[n - 1]).all(), f'{cls_name}: the NaN sample is not NaN throughout ({int(torch.isnan(got[n - 1]).sum())} of {got[n - 1].numel()})'
    assert_bit_equal_nan(got[:n - 1], clean[:n - 1], f'{cls_name}: the other samples vs the clean run')
