"""GPU: the evaluation metrics (csrc/metrics.hip through rfuse/metrics.py; reference util/metrics.py:6-89, util/retrieval.py:167-175).
Counts and squared-distance sums equal a float64 brute force exactly (integer equality) on chunks, densities, word-boundary lines and odd shapes;
distance-field occupancy equals torch's `df <= thr`; the four classes reproduce the reference's own states (tests/golden/metrics.npz); the
scene-level driver equals a per-scene brute force; results keep their bits across calls, beside another stream's F16 MFMAs, without a host sync."""
import numpy as np
import pytest
import torch

import testkit
from rfuse import configs as rf_configs
from rfuse import synthetic
from test_metrics_cpu import STATES, fixture_updates

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def metrics():
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    from rfuse import metrics as m
    return m


def brute(pred, target):
    """float64 brute force on the device: [B, 5] int64 n_pred, n_target, n_inter, s_tp, s_pt (squared distances through the exact expansion
    |a|^2 + |b|^2 - 2 a.b of integer coordinates, tiled)"""
    rows = []
    for p, t in zip(pred[:, 0].bool(), target[:, 0].bool()):
        P, T = torch.nonzero(p).double(), torch.nonzero(t).double()
        s = [0, 0]
        if len(P) and len(T):
            for i, (a, b) in enumerate(((T, P), (P, T))):
                bn = (b * b).sum(1)
                tot = 0
                for k in range(0, len(a), 2048):
                    x = a[k:k + 2048]
                    d2 = (x * x).sum(1)[:, None] + bn[None] - 2.0 * (x @ b.T)
                    tot += int(d2.min(1).values.sum().item())
                s[i] = tot
        rows.append([len(P), len(T), int((p & t).sum().item())] + s)
    return torch.tensor(rows, dtype=torch.int64)


def chunk_occ(seed, cfg):
    return synthetic.make_chunk(seed, cfg)['target_raw']


def check(metrics, pred, target, **kw):
    got = metrics.occupancy_stats(pred, target, **kw).cpu()
    thr = kw.get('threshold')
    p, t = (pred <= thr, target <= thr) if thr is not None else (pred, target)
    want = brute(p, t)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    return got


def test_chunk_batch_equals_brute_force(metrics):
    """B = 8 C2-like 64^3 pairs on the distance-field route (float32 and float16) and on the occupancy route: targets of make_chunk against other
    seeds' and shifted ones"""
    cfg = rf_configs.get_config('C2')
    thr = 0.75 * cfg['dataset_train']['voxel_size_target']
    tg = np.stack([chunk_occ(s, cfg) for s in range(8)])
    pr = np.stack([chunk_occ(s + 50, cfg) if s % 2 else np.roll(tg[s], (1, -2, 3), axis=(0, 1, 2)) for s in range(8)])
    t, p = torch.from_numpy(tg)[:, None].to(DEV), torch.from_numpy(pr)[:, None].to(DEV)
    got = check(metrics, p, t, threshold=thr)
    assert (got[:, 1] > 5000).all() and (got[:, 3] > 0).all()
    check(metrics, p.half(), t.half(), threshold=thr)
    check(metrics, p <= thr, t <= thr)
    check(metrics, (p <= thr).to(torch.uint8) * 7, (t <= thr).to(torch.uint8))


@pytest.mark.parametrize('shape', [(16, 16, 16), (64, 64, 64)])
def test_densities_equal_brute_force(metrics, shape):
    g = torch.Generator().manual_seed(3)
    vols = []
    for q in (0.0, 1e-3, 1e-2, 0.1, 0.3, 0.5):
        vols.append(torch.rand(2, 1, *shape, generator=g) < q)
    one = torch.zeros(2, 1, *shape, dtype=torch.bool)
    one[0, 0, 3, 5, 7] = True
    one[1, 0, -1, 0, -1] = True
    vols.append(one)
    x = torch.cat(vols).to(DEV)
    y = torch.cat([x[2:], x[:2]])
    got = check(metrics, x, y)
    if shape == (64, 64, 64):
        full = torch.ones(1, 1, 64, 64, 64, dtype=torch.bool, device=DEV)
        assert metrics.occupancy_stats(full, full).cpu().tolist() == [[262144] * 3 + [0, 0]]
    assert (got[:2, [0, 2, 3, 4]] == 0).all()                    # empty predictions: no voxels, no intersection, no Chamfer sums


def test_single_voxel_lines_and_word_boundaries(metrics):
    """lines whose only voxel sits at w = 0, 63, 64, 65 or the last w, queried from everywhere in the line and from neighbouring lines"""
    D, H, W = 3, 5, 130
    for w0 in (0, 63, 64, 65, 129):
        p = torch.zeros(1, 1, D, H, W, dtype=torch.bool)
        p[0, 0, 1, 2, w0] = True
        t = torch.zeros_like(p)
        t[0, 0, :, :, ::7] = True
        t[0, 0, 0, 4, 128] = True
        check(metrics, p.to(DEV), t.to(DEV))
        check(metrics, t.to(DEV), p.to(DEV))
    p = torch.zeros(2, 1, 1, 1, 200, dtype=torch.bool)
    p[0, 0, 0, 0, [0, 199]] = True
    p[1, 0, 0, 0, 100] = True
    check(metrics, p.to(DEV), torch.ones_like(p).to(DEV))


@pytest.mark.parametrize('shape', [(4, 6, 1), (5, 7, 63), (3, 9, 65), (6, 4, 129), (1, 33, 70), (40, 1, 66), (1, 1, 1), (70, 3, 5),
                                   (3, 130, 5), (2, 300, 2), (1, 1, 2048), (2048, 1, 1), (1, 2048, 1)])
def test_odd_shapes_equal_brute_force(metrics, shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.rand(3, 1, *shape, generator=g) < 0.05).to(DEV)
    y = (torch.rand(3, 1, *shape, generator=g) < 0.2).to(DEV)
    check(metrics, x, y)


def test_scene_sized_pair_equals_brute_force(metrics):
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(1, 1, 200, 64, 130, generator=g) < 0.004).to(DEV)
    y = (torch.rand(1, 1, 200, 64, 130, generator=g) < 0.002).to(DEV)
    check(metrics, x, y)


def test_unsupported_and_mismatched_inputs(metrics):
    x = torch.zeros(1, 1, 2049, 1, 1, dtype=torch.bool, device=DEV)
    with pytest.raises(RuntimeError, match='1..2048'):
        metrics.occupancy_stats(x, x)
    a = torch.zeros(1, 1, 4, 4, 4, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError):
        metrics.occupancy_stats(a, torch.zeros(1, 1, 4, 4, 5, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        metrics.occupancy_stats(a, a.to(torch.uint8))
    with pytest.raises(ValueError):
        metrics.occupancy_stats(a.float(), a.float())               # a distance field needs a threshold


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_threshold_matches_torch_comparison(metrics, dtype):
    thr = 0.07
    npt = np.float16 if dtype == torch.float16 else np.float32
    tq = npt(torch.tensor(thr, dtype=dtype).item())                 # thr as torch rounds it for `df <= thr`
    special = torch.tensor([float(v) for v in (tq, np.nextafter(tq, npt(np.inf)), np.nextafter(tq, npt(-np.inf)))]
                           + [float('nan'), float('inf'), -float('inf'), 0.0, 3.0], dtype=torch.float64)
    g = torch.Generator().manual_seed(4)
    x = special[torch.randint(0, len(special), (4, 1, 9, 10, 70), generator=g)].to(dtype).to(DEV)
    y = special[torch.randint(0, len(special), (4, 1, 9, 10, 70), generator=g)].to(dtype).to(DEV)
    got = metrics.occupancy_stats(x, y, threshold=thr).cpu()
    assert torch.equal(got, brute(x <= thr, y <= thr))


def test_fixture_parity_with_the_reference_classes(metrics, golden_dir):
    ups, compute = fixture_updates(golden_dir)
    ms = torch.nn.ModuleList([getattr(metrics, n)(compute_on_step=False) for n in STATES]).to(DEV)
    for pred, target, stats, states in ups:
        p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV)
        assert torch.equal(metrics.occupancy_stats(p, t).cpu(), torch.from_numpy(stats))
        for m in ms:
            assert m(p, t) is None
        got = np.array([getattr(m, n).item() for m, s in zip(ms, STATES.values()) for n in (s, 'total')], np.float32)
        np.testing.assert_allclose(got, states, rtol=1e-6)
        assert (got[1::2] == states[1::2]).all()
    np.testing.assert_allclose(np.array([m.compute().item() for m in ms], np.float32), compute, rtol=1e-6)


def test_forward_with_compute_on_step_returns_the_batch_value(metrics):
    x = (torch.rand(3, 1, 8, 8, 8, generator=torch.Generator().manual_seed(1)) < 0.3).to(DEV)
    y = torch.roll(x, 1, dims=2)
    m = metrics.IoU().to(DEV)
    m.iou_sum.fill_(100.0)
    m.total.fill_(1.0)
    v = m(x, y)
    st = brute(x, y).double()
    inter, union = st[:, 2], st[:, 0] + st[:, 1] - st[:, 2]
    assert v.item() == pytest.approx((inter / union).mean().item(), rel=1e-5)
    assert m.total.item() == 4.0


class _Scenes:
    """the attributes util/retrieval.py:167-175 touches"""

    def __init__(self, targets, voxel):
        self.scenes = list(targets)
        self._t = targets
        self.target_voxel_size = voxel

    def get_scene_target(self, scene):
        return self._t[scene]


def test_retrieval_metrics_equals_per_scene_brute_force(metrics):
    rng = np.random.default_rng(2)
    voxel = np.float32(0.05)
    thr = 0.75 * voxel
    shapes = {'scene_a': (40, 24, 70), 'scene_b': (96, 32, 64)}
    targets, retrievals = {}, []
    for name, shp in shapes.items():
        df = rng.uniform(0.0, 0.6, size=shp).astype(np.float32)
        targets[name] = df.astype(np.float16)                       # the scene store's precision
        retr = df + rng.normal(0.0, 0.02, size=shp).astype(np.float32)
        retrievals.append(torch.from_numpy(np.stack([retr, retr + 1.0])))       # [K, X, Y, Z]; only retrievals[i][0] is scored
    got = metrics.retrieval_metrics(retrievals, _Scenes(targets, voxel))
    iou = cd = prec = rec = 0.0
    n_iou = n_cd = 0
    for (name, shp), r in zip(shapes.items(), retrievals):
        p = (r[0] <= thr)[None, None].to(DEV)
        t = (torch.from_numpy(targets[name]) <= thr)[None, None].to(DEV)
        n_p, n_t, n_i, s_tp, s_pt = brute(p, t)[0].tolist()
        union = n_p + n_t - n_i
        if union:
            iou, n_iou = iou + n_i / union, n_iou + 1
        if n_p and n_t:
            cd, n_cd = cd + s_tp / n_t + s_pt / n_p, n_cd + 1
        prec, rec = prec + n_i / n_p, rec + n_i / n_t
    assert n_cd == 2
    np.testing.assert_allclose(got, [iou / n_iou, cd / n_cd, prec / 2, rec / 2], rtol=1e-5)


def test_bits_repeat_beside_f16_mfma_and_without_host_sync(metrics):
    cfg = rf_configs.get_config('C2')
    thr = 0.75 * cfg['dataset_train']['voxel_size_target']
    t = torch.from_numpy(np.stack([chunk_occ(s, cfg) for s in range(16)]))[:, None].to(DEV)
    p = torch.from_numpy(np.stack([chunk_occ(s + 70, cfg) for s in range(16)]))[:, None].to(DEV)
    ref = metrics.occupancy_stats(p, t, threshold=thr).clone()
    for _ in range(5):
        assert torch.equal(metrics.occupancy_stats(p, t, threshold=thr), ref)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream(DEV)
    scratch = torch.empty(256 * 256, device=DEV)
    outs = []
    side.wait_stream(main)
    testkit.f16_mfma_load(main, scratch)
    with torch.cuda.stream(side):
        for _ in range(10):
            outs.append(metrics.occupancy_stats(p, t, threshold=thr))
    torch.cuda.synchronize()
    assert all(torch.equal(o, ref) for o in outs)
    # update() never waits for the device: behind a ~15 ms kernel on the same stream it returns while that kernel still runs, and under
    # torch's sync debug mode (where ROCm's torch enforces it) nothing it does synchronises
    ms = [getattr(metrics, n)(compute_on_step=False).to(DEV) for n in STATES]
    pb, tb = p <= thr, t <= thr
    torch.cuda.synchronize()
    testkit.f16_mfma_load(main, scratch)
    torch.cuda.set_sync_debug_mode('error')
    try:
        for m in ms:
            m.update(pb, tb)
        pending = not main.query()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert pending
    torch.cuda.synchronize()
