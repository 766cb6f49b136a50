"""Dev tool (GPU box): the evaluation metrics' device path (rfuse.metrics.occupancy_stats, csrc/metrics.hip) against the reference's algorithm
done in torch on the same device (per volume torch.nonzero, then a tiled squared-distance min, util/metrics.py:42-49).

    python tools/metrics_bench.py [--reps 200] [--skip-torch]

Inputs: B = 32 pairs of 64^3 C2-like volumes (make_chunk targets of seeds 0..31 against the targets of seeds 100..131, occupied at
0.75 * voxel_size) as float32 distance fields and as bool grids, with and without Chamfer; one 512 x 128 x 512 scene pair at ~1 % occupancy.
Every number is the median of --reps calls, each bracketed by HIP events after a warm-up (so a call's host side is in it).  The pack pass's rate
printed here is the chamfer=False call on the float32 fields, bytes read (both fields) over the CALL time, against the 6.3 TB/s an MI355X reaches on
a copy; the kernel's own rate needs its time from a kernel trace (profiles/metrics_bench.txt)."""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / 'retrieval-fuse_amd'))
from rfuse import configs, metrics, synthetic      # noqa: E402

HBM_PEAK = 6.3e12


def timed(fn, reps, warmup=10):
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
    return statistics.median(times)


def torch_route(pred, target):
    """the reference's algorithm: nonzero per volume (a host sync each), squared distances to every point of the other cloud in tiles, min, mean"""
    out = []
    for p, t in zip(pred[:, 0], target[:, 0]):
        P, T = torch.nonzero(p).float(), torch.nonzero(t).float()
        if len(P) == 0 or len(T) == 0:
            out.append(float('nan'))
            continue
        m = []
        for a, b in ((T, P), (P, T)):
            m.append(torch.cat([torch.cdist(a[k:k + 4096], b).square_().min(1).values for k in range(0, len(a), 4096)]).mean())
        out.append(m[0] + m[1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--skip-torch', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    cfg = configs.get_config('C2')
    thr = 0.75 * cfg['dataset_train']['voxel_size_target']
    B = 32
    t = torch.from_numpy(np.stack([synthetic.make_chunk(s, cfg)['target_raw'] for s in range(B)]))[:, None].to(dev)
    p = torch.from_numpy(np.stack([synthetic.make_chunk(100 + s, cfg)['target_raw'] for s in range(B)]))[:, None].to(dev)
    tb, pb = t <= thr, p <= thr
    occ = tb.reshape(B, -1).sum(1)
    print('chunk batch: B = %d x 64^3, target occupancy %d..%d voxels per chunk' % (B, occ.min().item(), occ.max().item()))
    rows = []
    for name, fn in (('df f32, chamfer', lambda: metrics.occupancy_stats(p, t, threshold=thr)),
                     ('df f32, counts only (pack pass)', lambda: metrics.occupancy_stats(p, t, threshold=thr, chamfer=False)),
                     ('bool, chamfer', lambda: metrics.occupancy_stats(pb, tb)),
                     ('bool, counts only (pack pass)', lambda: metrics.occupancy_stats(pb, tb, chamfer=False))):
        us = timed(fn, a.reps)
        rows.append((name, us))
        print('  %-34s %9.1f us/call  %9.0f volumes/s' % (name, us, B / us * 1e6))
    pack_us = dict(rows)['df f32, counts only (pack pass)']
    nbytes = 2 * t.numel() * 4
    print('  counts-only call on float32 fields: %.1f MB read in %.1f us per CALL = %.2f TB/s (%.0f %% of %.1f TB/s); host side and launches included --'
          ' the kernel alone: a rocprofv3 --kernel-trace run of this tool'
          % (nbytes / 1e6, pack_us, nbytes / pack_us / 1e6, 100 * nbytes / pack_us / 1e6 / (HBM_PEAK / 1e12), HBM_PEAK / 1e12))
    stats = metrics.occupancy_stats(pb, tb)
    mine = ((stats[:, 3].double() / stats[:, 1].double()).float() + (stats[:, 4].double() / stats[:, 0].double()).float()).tolist()
    if not a.skip_torch:
        ref = torch_route(pb, tb)
        torch.cuda.synchronize()
        reps = max(3, a.reps // 40)
        us = timed(lambda: torch_route(pb, tb), reps, warmup=1)
        err = max(abs(x - y) / max(abs(y), 1e-30) for x, y in zip(mine, ref))
        print('  torch route (nonzero + tiled cdist^2 min, per volume): %.1f us/call (median of %d)  -> speed-up %.0fx over "df f32, chamfer";'
              ' max rel. difference of the per-volume Chamfer terms %.1e (fp32 cdist rounding)' % (us, reps, us / dict(rows)['df f32, chamfer'], err))
    S = (512, 128, 512)
    g = torch.Generator(device=dev).manual_seed(5)
    st = torch.rand(1, 1, *S, generator=g, device=dev) < 0.01
    sp = torch.roll(st, (1, 2, -1), dims=(2, 3, 4)) | (torch.rand(1, 1, *S, generator=g, device=dev) < 0.002)
    us = timed(lambda: metrics.occupancy_stats(sp, st), max(10, a.reps // 10))
    s = metrics.occupancy_stats(sp, st)[0].tolist()
    print('scene pair %d x %d x %d (bool), %d / %d occupied voxels: %.1f us/call with Chamfer' % (S + (s[0], s[1], us)))


if __name__ == '__main__':
    main()
