"""GPU: the mesh metrics (csrc/mesh_metrics.hip through rfuse/mesh_metrics.py; reference util/mesh_metrics.py:13-120).  Pinned to the reference
through tests/golden/mesh_metrics.npz (the reference's own distance_p2p / get_threshold_percentage / compute_metrics on recorded samples): nearest
neighbours bit for bit, distances to 1 ulp, dot products to 1e-12, threshold counts exactly, the five metrics to 1e-10.  The sampler and the voxeliser
are unpinned (rfuse/mesh_metrics.py docstring) and tested by what defines them.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from test_mesh_metrics_cpu import brute_nearest, face_normals_f32, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU visible')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def fx(golden_dir):
    z = load_fixture(golden_dir)
    z['pred_n'] = face_normals_f32(z['pred_v'], z['pred_t'])[z['pred_f']]
    z['tgt_n'] = face_normals_f32(z['tgt_v'], z['tgt_t'])[z['tgt_f']]
    return z


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def adversarial(case, z):
    rng = np.random.default_rng(17)
    f = np.float32
    if case == 'fixture completeness':
        return z['tgt_p'], z['pred_p']
    if case == 'fixture accuracy':
        return z['pred_p'], z['tgt_p']
    if case == 'duplicates':                       # every target occurs three times, in shuffled order: the lowest copy must win
        base = rng.normal(size=(700, 3)).astype(f)
        tgt = np.concatenate([base, base, base])[rng.permutation(2100)]
        return np.concatenate([base[:300], rng.normal(size=(433, 3)).astype(f)]), tgt
    if case == 'exact ties':                       # cell centres of an integer lattice: eight corners at the same distance
        g = np.stack(np.meshgrid(*[np.arange(11)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(f)
        return (g[rng.permutation(len(g))[:777]] + f(0.5)), g[rng.permutation(len(g))]
    if case == 'n = 1':
        return rng.normal(size=(1, 3)).astype(f), rng.normal(size=(1, 3)).astype(f)
    if case == 'one source':
        return rng.normal(size=(1, 3)).astype(f), rng.normal(size=(3001, 3)).astype(f)
    if case == 'one target':
        return rng.normal(size=(2500, 3)).astype(f), rng.normal(size=(1, 3)).astype(f)
    if case == 'ragged sizes':                     # neither a multiple of the source block (1024) nor of the target tile (1024); several target splits
        return (rng.normal(size=(1500 + 37, 3)) * 30).astype(f), (rng.normal(size=(70001, 3)) * 30).astype(f)
    if case == 'far apart':                        # differences near 1e6 with float32 spacing 0.06: the squares need all of float64
        return (rng.normal(size=(1031, 3)) + 1e6).astype(f), rng.normal(size=(2077, 3)).astype(f)
    raise KeyError(case)


@pytest.mark.parametrize('case', ['fixture completeness', 'fixture accuracy', 'duplicates', 'exact ties', 'n = 1', 'one source', 'one target',
                                  'ragged sizes', 'far apart'])
def test_nearest_neighbour_is_the_exact_float64_argmin(gpu, fx, case):
    from rfuse import mesh_metrics as mm
    src, tgt = adversarial(case, fx)
    d2, idx = mm.nearest_points(dev(src, gpu), dev(tgt, gpu))
    assert d2.dtype == torch.float64 and idx.dtype == torch.int32 and d2.shape == idx.shape == (len(src),)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    want_d2, want_idx, hits = brute_nearest(src, tgt)
    print('%s: %d x %d, %d sources with a tied minimum; d2 differs at %d, idx at %d (of them %d at unique minima)'
          % (case, len(src), len(tgt), (hits > 1).sum(), (d2 != want_d2).sum(), (idx != want_idx).sum(), ((idx != want_idx) & (hits == 1)).sum()))
    if case in ('duplicates', 'exact ties'):
        assert (hits > 1).sum() >= 300
    np.testing.assert_array_equal(d2, want_d2)                  # bit-equal
    np.testing.assert_array_equal(idx[hits == 1], want_idx[hits == 1])
    np.testing.assert_array_equal(idx, want_idx)                # and the lowest index where the minimum is not unique
    if case.startswith('fixture'):
        name = case.split()[1]
        np.testing.assert_array_equal(idx[hits == 1], fx[name + '_idx'][hits == 1])          # cKDTree's neighbours


@pytest.mark.parametrize('name', ['completeness', 'accuracy'])
def test_fixture_distance_p2p_and_threshold_counts(gpu, fx, name):
    from rfuse import mesh_metrics as mm
    s, t = ('tgt', 'pred') if name == 'completeness' else ('pred', 'tgt')
    ps, ns, pt, nt = (dev(fx[k], gpu) for k in (s + '_p', s + '_n', t + '_p', t + '_n'))
    dist, dots = mm.distance_p2p(ps, ns, pt, nt)
    assert dist.dtype == dots.dtype == torch.float64
    d, w = dist.cpu().numpy(), dots.cpu().numpy()
    ulps = np.abs(d - fx[name + '_dist']) / np.spacing(fx[name + '_dist'])
    print('%s: dist max %.3g ulp (%d values differ), dots max abs diff %.3g' % (name, ulps.max(), (ulps > 0).sum(), np.abs(w - fx[name + '_dots']).max()))
    assert ulps.max() <= 1
    assert np.abs(w - fx[name + '_dots']).max() <= 1e-12
    share = mm.get_threshold_percentage(dist, fx['thresholds'])
    assert share.dtype == torch.float64 and share.shape == (1000,)
    counts = share.cpu().numpy() * len(d)
    print('%s: counts differ at %d thresholds' % (name, (np.rint(counts) != fx[name + '_counts']).sum()))
    np.testing.assert_array_equal(share.cpu().numpy(), fx[name + '_counts'] / len(d))          # the same quotient: exactly equal counts
    share2 = mm.get_threshold_percentage(dist, dev(fx['thresholds'], gpu))                       # thresholds already on the device
    assert torch.equal(share, share2)
    # without normals: the reference's NaN column, the same distances
    dist2, nan = mm.distance_p2p(ps, None, pt, nt)
    assert torch.equal(dist, dist2) and bool(torch.isnan(nan).all())
    # a threshold list that ends below the largest distance, and one value
    few = mm.get_threshold_percentage(dist, [float(np.median(d))])
    assert few.cpu().numpy()[0] == (d <= np.median(d)).mean()


def test_fixture_voxels_and_the_five_metrics(gpu, fx):
    from rfuse import mesh_metrics as mm
    pv, pt, tv, tt = (dev(fx[k], gpu) for k in ('pred_v', 'pred_t', 'tgt_v', 'tgt_t'))
    gp, gt, lo = mm.voxel_grids(pv, pt, tv, tt)
    assert gp.dtype == gt.dtype == torch.uint8 and gp.shape == gt.shape
    keep = ~fx['vox_margin']
    flo = fx['vox_lo']
    got, want = [], []
    for g, ref in ((gp, fx['vox_pred']), (gt, fx['vox_tgt'])):
        assert set(np.unique(g.cpu().numpy()).tolist()) <= {0, 1}
        a = {tuple(c) for c in (np.argwhere(g.cpu().numpy() != 0) + np.asarray(lo)).tolist()}
        b = {tuple(c) for c in (np.argwhere(ref) + flo).tolist()}
        skip = {tuple(c) for c in (np.argwhere(~keep) + flo).tolist()}
        print('voxels: %d on the device, %d in the fixture, %d differ outside the margin cells (%d margin cells)' % (len(a), len(b), len((a ^ b) - skip), len(skip)))
        assert (a ^ b) - skip == set()
        got.append(a - skip)
        want.append(b - skip)
    iou = len(got[0] & got[1]) / len(got[0] | got[1])
    assert iou == float(fx['metrics_iou_unflagged'])
    if not (~keep).any():
        assert mm.voxel_iou(pv, pt, tv, tt) == fx['metrics'][0]
    m = mm.combine(iou if (~keep).any() else mm.voxel_iou(pv, pt, tv, tt), dev(fx['pred_p'], gpu), dev(fx['pred_n'], gpu), dev(fx['tgt_p'], gpu),
                   dev(fx['tgt_n'], gpu)).cpu().numpy()
    want_m = fx['metrics'].copy()
    want_m[0] = fx['metrics_iou_unflagged'] if (~keep).any() else want_m[0]
    rel = np.abs(m - want_m) / np.abs(want_m)
    print('metrics', m.tolist(), 'fixture', want_m.tolist(), 'rel. difference', rel.tolist())
    # reordering a float64 sum of 2e4 positive terms moves it by at most n * 2^-53 = 2e-12 relative; one decade of margin
    assert rel.max() <= 1e-10
    m2 = mm.combine(iou, dev(fx['pred_p'], gpu), dev(fx['pred_n'], gpu), dev(fx['tgt_p'], gpu), dev(fx['tgt_n'], gpu)).cpu().numpy()
    assert np.array_equal(m[1:], m2[1:])                        # fixed summation order: the same bits on every call


def tetra():
    """four faces of areas 0.5, 2, 4.5 and one large slanted one, plus a zero-area face and a face that indexes outside the vertex array"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 4], [3, 0, 0], [0, 3, 0], [2, 2, 2], [4, 4, 4]], np.float32)
    t = np.array([[0, 1, 2], [0, 1, 3], [0, 4, 5], [6, 6, 7], [3, 4, 5], [0, 1, 99], [1, 6, 7]], np.int32)
    return v, t


def test_sampler_points_lie_on_their_faces_and_seeds_are_streams(gpu, fx):
    from rfuse import mesh_metrics as mm
    v, t = fx['tgt_v'], fx['tgt_t']
    n = 200000
    p, f, nr = mm.sample_surface(dev(v, gpu), dev(t, gpu), n, seed=5)
    assert p.shape == (n, 3) and p.dtype == torch.float32 and f.shape == (n,) and f.dtype == torch.int32 and nr.shape == (n, 3) and nr.dtype == torch.float32
    p2, f2, nr2 = mm.sample_surface(dev(v, gpu), dev(t, gpu), n, seed=5)
    assert torch.equal(p, p2) and torch.equal(f, f2) and torch.equal(nr, nr2)                  # the same seed: the same bits
    ph, fh, _ = mm.sample_surface(dev(v, gpu), dev(t, gpu), n // 2, seed=5)
    assert torch.equal(ph, p[:n // 2]) and torch.equal(fh, f[:n // 2])                         # sample i depends on (mesh, seed, i) alone
    p3, f3, _ = mm.sample_surface(dev(v, gpu), dev(t, gpu), n, seed=6)
    same = (p3 == p).all(1).float().mean().item()
    print('another seed: %.5f of the points coincide' % same)
    assert same < 1e-3 and not torch.equal(f3, f)
    P, F, N = p.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64), nr.cpu().numpy().astype(np.float64)
    assert F.min() >= 0 and F.max() < len(t)
    tri = v.astype(np.float64)[t.astype(np.int64)][F]
    e1, e2, d = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], P - tri[:, 0]
    c = np.cross(e1, e2)
    area2 = np.linalg.norm(c, axis=-1)
    assert area2.min() > 0                                       # no zero-area face is drawn
    unit = c / area2[:, None]
    b1 = (np.cross(d, e2) * unit).sum(-1) / area2                # barycentric coordinates of the projection
    b2 = (np.cross(e1, d) * unit).sum(-1) / area2
    plane = np.abs((d * unit).sum(-1))
    extent = float(np.ptp(v, axis=0).max())
    print('barycentric min %.3g / %.3g / %.3g, plane distance max %.3g (extent %.3g), normals max diff %.3g'
          % (b1.min(), b2.min(), (1 - b1 - b2).min(), plane.max(), extent, np.abs(N - unit).max()))
    assert min(b1.min(), b2.min(), (1 - b1 - b2).min()) >= -1e-6
    assert plane.max() <= 1e-5 * extent
    assert np.abs(N - unit).max() <= 1e-6                        # the float64 cross product, normalised


def test_sampler_draws_faces_in_proportion_to_their_area(gpu):
    """10^6 samples on a mesh of known unequal areas: every per-face count within 5 sigma of its binomial mean (deterministic for this seed); the
    zero-area face and the face with an index outside the vertex array are never drawn"""
    from rfuse import mesh_metrics as mm
    v, t = tetra()
    n = 1000000
    p, f, nr = mm.sample_surface(dev(v, gpu), dev(t, gpu), n, seed=2024)
    counts = np.bincount(f.cpu().numpy(), minlength=len(t))
    tri = v.astype(np.float64)[np.clip(t, 0, len(v) - 1)]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=-1)
    area[5] = 0.0                                               # refers to vertex 99
    assert area[3] == 0.0 and (np.delete(area, [3, 5]) > 0).all() and area[:3].tolist() == [0.5, 2.0, 4.5]
    q = area / area.sum()
    sigma = np.sqrt(n * q * (1 - q))
    z = np.where(sigma > 0, np.abs(counts - n * q) / np.where(sigma > 0, sigma, 1), 0)
    print('areas', area.tolist(), 'counts', counts.tolist(), 'deviations in sigma', np.round(z, 2).tolist())
    assert counts[3] == 0 and counts[5] == 0
    assert z.max() <= 5
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(nr).all())
    # a surface of total area 0: NaN points, face -1 (no host sync to raise from)
    p0, f0, _ = mm.sample_surface(dev(v, gpu), dev(t[3:4], gpu), 100)
    assert bool(torch.isnan(p0).all()) and bool((f0 == -1).all())


def sphere_field(n, r, c):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing='ij'), -1)
    return np.minimum(np.abs(np.linalg.norm(g - np.asarray(c, np.float32), axis=-1) - r), 3.0).astype(np.float32)


def test_compute_metrics_end_to_end_on_obj_files(gpu, tmp_path):
    from rfuse import mesh, mesh_metrics as mm
    a, b = sphere_field(48, 14.0, (23.5, 24.2, 22.9)), sphere_field(48, 15.0, (24.5, 24.2, 23.4))
    mesh.visualize_sdf_as_mesh(torch.from_numpy(a).to(gpu), tmp_path / 'a.obj')
    mesh.visualize_sdf_as_mesh(torch.from_numpy(b).to(gpu), tmp_path / 'b.obj')
    # 100 000 samples on ~4900 square units: 20 per unit area, so a point has no neighbour within F[9]'s 0.64 with probability exp(-20 pi 0.64^2) = 7e-12
    n = 100000
    same = mm.compute_metrics(tmp_path / 'a.obj', tmp_path / 'a.obj', n_samples=n, seed=3)
    print('identical meshes:', same)
    assert len(same) == 5 and all(isinstance(x, float) for x in same)
    assert same[0] == 1.0 and same[3] == 1.0 and same[4] == 1.0            # F[9]: all points within 0.64, F[14]: within 0.96
    assert 0 < same[1] < 0.5 and same[2] > 0.95                            # two independent samplings of one surface: close, not equal
    diff = mm.compute_metrics(tmp_path / 'a.obj', tmp_path / 'b.obj', n_samples=n, seed=3)
    print('two spheres:', diff)
    assert 0 < diff[0] < 1 and diff[1] > same[1] and 0 < diff[3] <= diff[4] <= 1 and diff[2] > 0.9
    (va, ta), (vb, tb) = mesh.load_obj(tmp_path / 'a.obj'), mesh.load_obj(tmp_path / 'b.obj')
    direct = mm.mesh_metrics(dev(va, gpu), dev(ta, gpu), dev(vb, gpu), dev(tb, gpu), n_samples=n, seed=3)
    assert direct == diff                                                  # compute_metrics is load_obj + mesh_metrics
    assert mm.voxel_iou(dev(va, gpu), dev(ta, gpu), dev(vb, gpu), dev(tb, gpu)) == diff[0]
    # the layers agree: mesh_metrics is sample_surface (seed, seed + 1) -> combine
    pa, _, na = mm.sample_surface(dev(va, gpu), dev(ta, gpu), n, seed=3)
    pb, _, nb = mm.sample_surface(dev(vb, gpu), dev(tb, gpu), n, seed=4)
    assert mm.combine(diff[0], pa, na, pb, nb).tolist() == diff
    acc, _ = mm.distance_p2p(pa, na, pb, nb)
    comp, _ = mm.distance_p2p(pb, nb, pa, na)
    assert abs(0.5 * (acc.mean().item() + comp.mean().item()) - diff[1]) <= 1e-10 * diff[1]          # two summation orders of 1e5 positive terms
    pr, rc = mm.get_threshold_percentage(acc, mm.THRESHOLDS)[9].item(), mm.get_threshold_percentage(comp, mm.THRESHOLDS)[9].item()
    assert abs(2 * pr * rc / (pr + rc) - diff[3]) <= 1e-12
    # F is NaN where precision + recall = 0: two surfaces further apart than F[14]'s threshold
    far = mm.mesh_metrics(dev(va, gpu), dev(ta, gpu), dev(vb + np.float32(500), gpu), dev(tb, gpu), n_samples=2000)
    print('far apart:', far)
    assert far[0] == 0.0 and np.isnan(far[3]) and np.isnan(far[4]) and far[1] > 400
