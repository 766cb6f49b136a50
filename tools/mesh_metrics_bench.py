"""Dev tool (GPU box): the mesh metrics' device path (rfuse.mesh_metrics, csrc/mesh_metrics.hip) stage by stage, against the reference's algorithm
(util/mesh_metrics.py:84-108: nearest neighbours of 100 000 points in 100 000) done two other ways on the same box: a chunked float64 squared-distance
min in torch on the same GPU, and scipy's cKDTree on the host when scipy is importable there (skipped, and said so, otherwise).

    python tools/mesh_metrics_bench.py [--reps 20] [--samples 100000] [--skip-torch]

Workload: the marching-cubes meshes of two seeded C2 chunks (the target of seed 3 and the same field at 1.2 x the level, shifted), 100 000 samples
each, one full ``mesh_metrics`` call.  Every number is the median of --reps calls after a warm-up, each call bracketed by HIP events on the current
stream (so a call's host side is in it).  The nearest-neighbour rate counts, per (source, target) pair, the 8 float64 operations of the definition
(3 subtractions, 3 multiplications, 2 additions; the compare and the select are not counted) over the call time, against 78.6 TFLOP/s, the vector
FP64 peak of the MI355X data sheet -- a figure that counts a fused multiply-add as two, so unfused operations can reach half of it."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / 'retrieval-fuse_amd'))
from rfuse import configs, mesh, mesh_metrics as mm, synthetic      # noqa: E402

FP64_VECTOR_PEAK = 78.6e12
OPS_PER_PAIR = 8


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times), min(times), max(times)


def torch_nearest(src, tgt, block=1024):
    """the reference's query as a brute force in torch: float64 squared distances of a block of sources to every target, min and argmin"""
    s, t = src.double(), tgt.double()
    d2, idx = [], []
    for k in range(0, len(s), block):
        d = s[k:k + block, None, :] - t[None]
        m = (d * d).sum(-1).min(1)
        d2.append(m.values)
        idx.append(m.indices)
    return torch.cat(d2), torch.cat(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--samples', type=int, default=100000)
    ap.add_argument('--skip-torch', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    cfg = configs.get_config('C2')
    level = 0.75 * cfg['dataset_train']['voxel_size_target']
    vol = torch.from_numpy(synthetic.make_chunk(3, cfg)['target_raw']).to(dev)
    vp, tp = mesh.marching_cubes(vol, level)
    vt, tt = mesh.marching_cubes(vol, 1.2 * level)
    vt = vt + torch.tensor([0.31, -0.17, 0.23], device=dev)
    n = a.samples
    print('meshes: %d / %d vertices, %d / %d triangles; %d samples each' % (len(vp), len(vt), len(tp), len(tt), n))
    pp, _, pn = mm.sample_surface(vp, tp, n, 0)
    pt, _, tn = mm.sample_surface(vt, tt, n, 1)
    d2, idx = mm.nearest_points(pp, pt)
    rows = [('mesh_metrics, the whole call (five floats back)', lambda: mm.mesh_metrics(vp, tp, vt, tt, n_samples=n)),
            ('  voxel_iou (2 x voxelise + occupancy counts, extent read back)', lambda: mm.voxel_iou(vp, tp, vt, tt)),
            ('  sample_surface (areas, cumsum, draw), one mesh', lambda: mm.sample_surface(vp, tp, n, 0)),
            ('  nearest_points, one direction', lambda: mm.nearest_points(pp, pt)),
            ('  distance_p2p, one direction (nearest + statistics)', lambda: mm.distance_p2p(pp, pn, pt, tn)),
            ('  combine (both directions, counts, five metrics)', lambda: mm.combine(0.5, pp, pn, pt, tn))]
    res = {}
    for name, fn in rows:
        res[name] = timed(fn, a.reps)
        print('%-66s %10.1f us/call  (min %.1f, max %.1f)' % ((name,) + res[name]))
    nn_us = res['  nearest_points, one direction'][0]
    rate = n * n * OPS_PER_PAIR / (nn_us * 1e-6)
    print('nearest_points: %d x %d pairs x %d float64 operations in %.1f us per CALL = %.2f TFLOP/s = %.1f %% of the %.1f TFLOP/s vector-FP64 peak '
          '(spec; counts an FMA as two -- unfused operations top out at half of it); %.2f G pairs/s; the kernel alone: a rocprofv3 --kernel-trace run'
          % (n, n, OPS_PER_PAIR, nn_us, rate / 1e12, 100 * rate / FP64_VECTOR_PEAK, FP64_VECTOR_PEAK / 1e12, n * n / nn_us / 1e3))
    if not a.skip_torch:
        rd2, ridx = torch_nearest(pp, pt)
        print('torch float64 brute force: d2 bit-equal %s, idx equal %s' % (bool(torch.equal(rd2, d2)), bool(torch.equal(ridx.int(), idx))))
        us = timed(lambda: torch_nearest(pp, pt), max(3, a.reps // 5), warmup=1)
        print('%-66s %10.1f us/call  (min %.1f, max %.1f)  -> %.1fx nearest_points' % (('torch route: chunked float64 (d * d).sum(-1).min(1), one direction',) + us + (us[0] / nn_us,)))
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        print('cKDTree on the host: skipped, scipy is not importable on this machine')
    else:
        s, t = pp.cpu().numpy(), pt.cpu().numpy()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            dist, kidx = cKDTree(t).query(s)
            ts.append((time.perf_counter() - t0) * 1e6)
        print('cKDTree(tgt).query(src) on the host (build + query, one thread, median of 3): %.1f us  -> %.1fx nearest_points; distances bit-equal to '
              'sqrt(d2): %s' % (statistics.median(ts), statistics.median(ts) / nn_us, bool(np.array_equal(dist, np.sqrt(d2.cpu().numpy())))))


if __name__ == '__main__':
    main()
