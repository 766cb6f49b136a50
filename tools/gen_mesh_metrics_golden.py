"""Fixture generator for the mesh metrics (CPU; needs the reference checkout and scipy, as tools/gen_metrics_golden.py needs the checkout): runs the
reference's own ``util/mesh_metrics.py`` -- ``distance_p2p``, ``get_threshold_percentage`` and ``compute_metrics`` as written -- on two marching-cubes
meshes and writes tests/golden/mesh_metrics.npz (arrays only, under 1 MiB).

    python tools/gen_mesh_metrics_golden.py

The reference imports ``trimesh`` and ``util.intersections`` (which imports trimesh); both are stood in for through ``sys.modules``.  ``compute_metrics``
reaches trimesh through ``trimesh.load_mesh(path)`` and uses of the mesh ``.sample(n, return_index=True)``, ``.face_normals`` and
``.voxelized(pitch).points``; the stand-in mesh hands back the recorded samples (whatever count is asked for), the float32-rounded unit face normals
and ``pitch *`` the cells of ``voxelize`` below, the float64 restatement of the voxel rule of include/rfuse_eval.h.

Meshes: oracle/mesh.py marching cubes of the seeded rfuse.synthetic C2 chunk 1, every second voxel (vertices scaled back by 2), at the occupancy level
and at 1.2 x that level shifted by (0.31, -0.17, 0.23).  Samples: N points per mesh from ``sample`` below (numpy, area-weighted, reflected
barycentrics; float32 points as the reference's ``astype(np.float32)`` leaves them).

Layout of tests/golden/mesh_metrics.npz
                        pred_v / tgt_v float32 [V, 3], pred_t / tgt_t int16 [T, 3]; pred_p / tgt_p float32 [N, 3] sample points, pred_f / tgt_f int16 [N]
                        their faces (normals = float32(unit face normal)[face], ``face_normals_f32``); thresholds float64 [1000];
                        completeness_counts / accuracy_counts int64 [1000] (#dist <= t; completeness = target -> prediction);
                        completeness_idx / accuracy_idx int32 [N] cKDTree's neighbours; metrics float64 [5] = compute_metrics;
                        vox_lo int64 [3], vox_shape int64 [3], vox_pred / vox_tgt / vox_margin uint8 packbits of [X, Y, Z] grids over the cells
                        vox_lo + (x, y, z): occupied by the prediction / the target / decided by a separating-axis margin under 1e-9 * pitch;
                        metrics_iou_unflagged float64: the IoU without the vox_margin cells
                        completeness_dist / completeness_dots / accuracy_dist / accuracy_dots float64 [N]: distance_p2p's two results per direction
"""
import sys
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from oracle.gen_golden import REF, save_fixture        # noqa: E402
from oracle.mesh import marching_cubes_reference       # noqa: E402
from rfuse import configs as rf_configs                # noqa: E402  (gen_golden put the product package on the path)
from rfuse import synthetic                            # noqa: E402

N = 20000
PITCH = 1.1875
TIE_CAP = 1e-3          # share of source points whose two nearest targets are equidistant
MARGIN_CAP = 1e-3       # share of union voxels decided by a separating-axis margin under 1e-9 * pitch


def import_reference_mesh_metrics():
    for n in ('trimesh', 'util.intersections'):
        sys.modules[n] = types.ModuleType(n)
    sys.modules['util.intersections'].slice_mesh_plane = None
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules['tqdm'] = types.ModuleType('tqdm')
        sys.modules['tqdm'].tqdm = lambda x, **kw: x
    for k in [k for k in sys.modules if k == 'util' or (k.startswith('util.') and k != 'util.intersections')]:
        del sys.modules[k]
    sys.path.insert(0, str(REF))
    import util.mesh_metrics as ref
    assert str(REF) in ref.__file__, ref.__file__
    return ref


def face_normals_f32(v, t):
    """float32(unit face normal), the float64 cross product of the float32 vertices normalised in float64; zero-area faces give NaN"""
    p = v.astype(np.float64)[t.astype(np.int64)]
    c = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    with np.errstate(invalid='ignore', divide='ignore'):
        return (c / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])[:, None]).astype(np.float32)


def sample(v, t, n, seed):
    """the stand-in for trimesh's mesh.sample: -> (points float32 [n, 3], face int64 [n])"""
    rng = np.random.default_rng(seed)
    p = v.astype(np.float64)[t.astype(np.int64)]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=-1)
    cdf = np.cumsum(area)
    face = np.minimum(np.searchsorted(cdf, rng.random(n) * cdf[-1], side='right'), len(t) - 1)
    r = rng.random((n, 2))
    flip = r.sum(1) > 1
    r[flip] = 1 - r[flip]
    pts = p[face, 0] + r[:, :1] * (p[face, 1] - p[face, 0]) + r[:, 1:] * (p[face, 2] - p[face, 0])
    return pts.astype(np.float32), face


def index_range(verts, pitch):
    lo, hi = np.min([v.min(0) for v in verts], 0).astype(np.float64), np.max([v.max(0) for v in verts], 0).astype(np.float64)
    return (np.floor(lo / pitch - 0.5) - 1).astype(np.int64), (np.ceil(hi / pitch + 0.5) + 1).astype(np.int64)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def voxelize(v, t, pitch, lo, shape):
    """The voxel rule in float64: cell (i, j, k) = the closed cube of edge pitch centred at pitch * (i, j, k), occupied when a triangle is separated from
    it along none of the 13 axes (3 cube axes, the face normal, 9 cube-axis x edge products).  -> (occupied bool [shape], margin float64 [shape]: per
    cell the smallest over the triangles of the largest normalised separation over the axes -- <= 0 occupied, > 0 free; |margin| says how far the
    decision is from flipping).  Operation order as in csrc/mesh_metrics.hip (dot = (x x' + y y') + z z', radius = h ((|x| + |y|) + |z|))."""
    pitch, h = np.float64(np.float32(pitch)), 0.5 * np.float64(np.float32(pitch))
    tri = v.astype(np.float64)[t.astype(np.int64)]                                           # [T, 3, 3]
    margin = np.full(shape, np.inf)
    tlo = np.floor(tri.min(1) / pitch - 0.5) - 1
    thi = np.ceil(tri.max(1) / pitch + 0.5) + 1
    m = int((thi - tlo).max()) + 1
    off = np.stack(np.meshgrid(*[np.arange(m)] * 3, indexing='ij'), -1).reshape(-1, 3)
    unit = np.eye(3)
    for s in range(0, len(tri), 512):
        tr = tri[s:s + 512]
        cells = (tlo[s:s + 512, None, :] + off[None]).astype(np.int64)                      # [n, m^3, 3]
        ok = ((cells <= thi[s:s + 512, None, :]) & (cells >= lo) & (cells < lo + np.asarray(shape))).all(-1)
        ctr = pitch * cells.astype(np.float64)
        vs = tr[:, None, :, :] - ctr[:, :, None, :]                                          # [n, m^3, 3 vertices, 3]
        e = np.stack([tr[:, 1] - tr[:, 0], tr[:, 2] - tr[:, 1], tr[:, 0] - tr[:, 2]], 1)     # [n, 3 edges, 3]
        nrm = np.cross(e[:, 0], e[:, 1])
        axes = [np.broadcast_to(unit[k], nrm.shape) for k in range(3)] + [nrm]
        zero = np.zeros(len(tr))
        for k in range(3):
            d = e[:, k]
            axes += [np.stack([zero, -d[:, 2], d[:, 1]], -1), np.stack([d[:, 2], zero, -d[:, 0]], -1), np.stack([-d[:, 1], d[:, 0], zero], -1)]
        worst = np.full(cells.shape[:2], -np.inf)
        sep = np.zeros(cells.shape[:2], bool)
        for a in axes:
            p = _dot(a[:, None, None, :], vs)                                                # [n, m^3, 3]
            r = h * ((np.abs(a[:, 0]) + np.abs(a[:, 1])) + np.abs(a[:, 2]))[:, None]
            sep |= (p.min(-1) > r) | (p.max(-1) < -r)
            g = np.maximum(p.min(-1) - r, -r - p.max(-1))
            length = np.sqrt(_dot(a, a))[:, None]
            with np.errstate(invalid='ignore', divide='ignore'):
                worst = np.maximum(worst, np.where(length > 0, g / length, -np.inf))
        assert ((worst > 0) == sep)[ok].all()
        idx = (cells - lo)[ok]
        np.minimum.at(margin, (idx[:, 0], idx[:, 1], idx[:, 2]), worst[ok])
    return margin <= 0, margin


class _Voxels:
    def __init__(self, points):
        self.points = points


class _Mesh:
    """what compute_metrics uses of a trimesh.Trimesh"""

    def __init__(self, points, face, normals, cells):
        self._points, self._face, self.face_normals, self._cells = points, face, normals, cells

    def sample(self, count, return_index=False):
        return (self._points.astype(np.float64), self._face) if return_index else self._points.astype(np.float64)

    def voxelized(self, pitch):
        assert pitch == PITCH
        return _Voxels(pitch * self._cells.astype(np.float64))


def main():
    ref = import_reference_mesh_metrics()
    from scipy.spatial import cKDTree
    cfg = rf_configs.get_config('C2')
    level = 0.75 * cfg['dataset_train']['voxel_size_target']
    vol = synthetic.make_chunk(1, cfg)['target_raw'][::2, ::2, ::2]
    pv, pt = marching_cubes_reference(vol, level)
    tv, tt = marching_cubes_reference(vol, 1.2 * level)
    pv = (pv.astype(np.float32) * np.float32(2)).astype(np.float32)
    tv = (tv.astype(np.float64) * 2 + np.array([0.31, -0.17, 0.23])).astype(np.float32)
    assert max(len(pv), len(tv), len(pt), len(tt)) < 32768
    pp, pf = sample(pv, pt, N, 11)
    tp, tf = sample(tv, tt, N, 12)
    pn, tn = face_normals_f32(pv, pt), face_normals_f32(tv, tt)
    assert np.isfinite(pn[pf]).all() and np.isfinite(tn[tf]).all()

    out = {}
    thresholds = np.linspace(64. / 1000, 64, 1000)
    for name, (src, nsrc, tgt, ntgt) in (('completeness', (tp, tn[tf], pp, pn[pf])), ('accuracy', (pp, pn[pf], tp, tn[tf]))):
        dist, dots = ref.distance_p2p(src, nsrc.astype(np.float64), tgt, ntgt.astype(np.float64))
        two, idx2 = cKDTree(tgt).query(src, k=2)
        assert np.array_equal(two[:, 0], dist)
        ties = float((two[:, 0] == two[:, 1]).mean())
        print('%s: share of source points with two equidistant nearest targets %.4f %%' % (name, 100 * ties))
        assert ties <= TIE_CAP, ties
        share = np.array(ref.get_threshold_percentage(dist, thresholds))
        counts = np.rint(share * len(dist)).astype(np.int64)
        assert np.array_equal(counts, np.array([(dist <= t).sum() for t in thresholds]))
        out[name + '_counts'], out[name + '_idx'] = counts, idx2[:, 0].astype(np.int32)
        out[name + '_dist'], out[name + '_dots'] = dist.astype(np.float64), dots.astype(np.float64)

    lo, hi = index_range([pv, tv], np.float64(np.float32(PITCH)))
    shape = tuple(int(s) for s in hi - lo + 1)
    (gp, mp), (gt, mt) = voxelize(pv, pt, PITCH, lo, shape), voxelize(tv, tt, PITCH, lo, shape)
    union = gp | gt
    flagged = ((np.abs(mp) < 1e-9 * PITCH) | (np.abs(mt) < 1e-9 * PITCH))
    share = float((flagged & (union | flagged)).sum() / union.sum())
    print('voxels: %d / %d occupied, union %d; share decided by a margin under 1e-9 pitch %.4f %%' % (gp.sum(), gt.sum(), union.sum(), 100 * share))
    assert share <= MARGIN_CAP, share

    meshes = {'pred': _Mesh(pp, pf, pn.astype(np.float64), np.argwhere(gp) + lo), 'target': _Mesh(tp, tf, tn.astype(np.float64), np.argwhere(gt) + lo)}
    sys.modules['trimesh'].load_mesh = lambda path: meshes[path]
    metrics = np.array(ref.compute_metrics('pred', 'target'), np.float64)
    print('compute_metrics [iou, chamferL1, normals_correctness, F[9], F[14]] =', metrics.tolist())
    keep = ~flagged
    out.update(pred_v=pv, pred_t=pt.astype(np.int16), tgt_v=tv, tgt_t=tt.astype(np.int16), pred_p=pp, pred_f=pf.astype(np.int16), tgt_p=tp,
               tgt_f=tf.astype(np.int16), thresholds=thresholds, metrics=metrics, vox_lo=lo.astype(np.int64), vox_shape=np.array(shape, np.int64),
               vox_pred=np.packbits(gp.reshape(-1)), vox_tgt=np.packbits(gt.reshape(-1)), vox_margin=np.packbits(flagged.reshape(-1)),
               metrics_iou_unflagged=np.float64((gp & gt & keep).sum() / ((gp | gt) & keep).sum()))
    save_fixture('mesh_metrics', **out)
    assert (REPO / 'tests' / 'golden' / 'mesh_metrics.npz').stat().st_size < 1 << 20


if __name__ == '__main__':
    main()
