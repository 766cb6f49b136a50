"""Dev tool (GPU box): the retrieval trainer's IoU matrix on the device (rfuse.losses.target_iou_matrix, csrc/iou_matrix.hip) against plain torch on the
same GPU, in the same process.

    python tools/iou_matrix_bench.py [--reps 200] [--out profiles/iou_matrix_bench.txt] [--rows matrix|step]

Rows ``matrix``: ``target_iou_matrix(target, mean, std, thr, repeat=2)`` from normalised float32 targets at B = 128, 192, 512 on 32^3 windows, B = 128 on
24^3 and B = 2048 on 32^3 (the validation batch), against
  (a) the reference's formula as written (util/misc.py:51-59 on ``target * std + mean <= thr``, then ``.repeat(2, 2)``): four [B^2, V] bool tensors.  A row
      whose 4 * B^2 * V bytes exceed --budget-gib is skipped, and the output says so;
  (b) the strongest plain-torch restatement: the occupancy cast to float32, ``b @ b.T`` for the intersections (exact: the counts stay below 2^24), the row
      sums for the counts, the same four float32 operations, ``.repeat(2, 2)``.
Rows ``step``: ``RetrievalStepLoss`` forward + backward to the two feature tensors with and without ``iou_scaling`` at B = 128 and 512, dim 64.
Every figure is the median of --reps iterations, each bracketed by HIP events after a warm-up (the host side of the calls is in it), with the 10th / 90th
percentile as the spread.  The matrices of the three paths are compared bit for bit before anything is timed.

The two groups of rows can be run as separate processes, each under its own time limit:

    timeout -k 10 600 python tools/iou_matrix_bench.py --rows matrix --out profiles/iou_matrix_bench.txt && \\
    timeout -k 10 300 python tools/iou_matrix_bench.py --rows step --out profiles/iou_matrix_bench.txt --append
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / 'retrieval-fuse_amd'))
from rfuse.losses import RetrievalStepLoss, target_iou_matrix         # noqa: E402

MEAN, STD, VOXEL = 0.059954833543534335, 0.010110036361741626, 0.020834      # rfuse.configs: ShapeNetV2
THR = 0.75 * VOXEL


def timed(fn, reps, warmup=20):
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
    times.sort()
    return statistics.median(times), times[len(times) // 10], times[len(times) * 9 // 10]


def reference_formula(target):
    """get_iou_matrix as written, on the trainer's occupancy"""
    batch_shapes = target * STD + MEAN <= THR
    n, _, d, h, w = batch_shapes.shape
    lhs = batch_shapes.bool().expand(-1, n, -1, -1, -1).reshape((n * n, 1, d, h, w))
    rhs = batch_shapes.bool().reshape((1, n, d, h, w)).expand(n, -1, -1, -1, -1).reshape((n * n, 1, d, h, w))
    intersection = (lhs & rhs).squeeze(1).sum(-1).sum(-1).sum(-1)
    union = (lhs | rhs).squeeze(1).sum(-1).sum(-1).sum(-1)
    return (intersection / (union + 1e-5)).reshape((n, n)).repeat(2, 2)


def matmul_formula(target):
    b = (target * STD + MEAN <= THR).reshape(target.shape[0], -1).to(torch.float32)
    inter = b @ b.t()
    counts = b.sum(1)
    return (inter / ((counts[:, None] + counts[None, :] - inter) + 1e-5)).repeat(2, 2)


def targets(b, win, gen, dev):
    """normalised truncated distances to spherical shells: occupancies from a few voxels to about a third of the window"""
    ax = (torch.arange(win, dtype=torch.float32) + 0.5) / win * 2 - 1
    x = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).to(dev)
    centre = (torch.rand(b, 1, 1, 1, 3, generator=gen) * 0.8 - 0.4).to(dev)
    radius = (0.05 + 0.85 * torch.rand(b, 1, 1, 1, generator=gen)).to(dev)
    width = (0.5 + 5.5 * torch.rand(b, 1, 1, 1, generator=gen)).to(dev)
    raw = ((x[None] - centre).norm(dim=-1) - radius).abs() * VOXEL * (win / 2) / width
    return ((raw.clamp(max=3 * VOXEL) - MEAN) / STD).reshape(b, 1, win, win, win).contiguous()


def fmt(t):
    return '%9.1f (%.1f .. %.1f)' % t


def matrix_rows(a, lines, dev, gen):
    budget = int(a.budget_gib * (1 << 30))
    for b, win in ((128, 32), (192, 32), (512, 32), (128, 24), (2048, 32)):
        t = targets(b, win, gen, dev)
        v = win ** 3
        occ = (t * STD + MEAN <= THR).reshape(b, -1)
        got = target_iou_matrix(t, MEAN, STD, THR)
        same_b = torch.equal(got, matmul_formula(t))
        t_hip = timed(lambda: target_iou_matrix(t, MEAN, STD, THR), a.reps)
        t_b = timed(lambda: matmul_formula(t), a.reps)
        need = 4 * b * b * v
        if need <= budget:
            same_a = torch.equal(got, reference_formula(t))
            t_a = timed(lambda: reference_formula(t), a.reps, warmup=3)
            part_a = '(a) reference formula %s   (a) / HIP = %7.1f   bits equal: %s' % (fmt(t_a), t_a[0] / t_hip[0], same_a)
        else:
            part_a = '(a) reference formula SKIPPED: its four [B^2, V] bool tensors take %.1f GiB, over the budget of %.1f GiB' % (need / (1 << 30), a.budget_gib)
        lines.append('B = %4d, %2d^3, occupancy %.4f .. %.3f   HIP %s   (b) float matmul %s   (b) / HIP = %5.2f   bits equal: %s   %s'
                     % (b, win, float(occ.float().mean(1).min()), float(occ.float().mean(1).max()), fmt(t_hip), fmt(t_b), t_b[0] / t_hip[0], same_b, part_a))
        print(lines[-1], flush=True)
        del t, occ, got
        torch.cuda.empty_cache()


def step_rows(a, lines, dev, gen):
    for b in (128, 512):
        t = targets(b, 32, gen, dev)
        ft = torch.randn(b, 64, 1, 1, 1, generator=gen).to(dev).requires_grad_(True)
        fi = (ft.detach().cpu() + 0.5 * torch.randn(b, 64, 1, 1, 1, generator=gen)).to(dev).requires_grad_(True)
        res = []
        for scaling in (True, False):
            step = RetrievalStepLoss(0.2, MEAN, STD, VOXEL, iou_scaling=scaling)

            def run():
                total, _ = step(fi, ft, t)
                total.backward()
                fi.grad = ft.grad = None
                return total.detach()
            res.append((timed(run, a.reps), float(run())))
        (t_on, l_on), (t_off, l_off) = res
        lines.append('RetrievalStepLoss forward + backward, B = %4d, dim 64, 32^3 targets   iou_scaling %s   without %s   difference %7.1f   [loss %.6f vs %.6f]'
                     % (b, fmt(t_on), fmt(t_off), t_on[0] - t_off[0], l_on, l_off))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--append', action='store_true')
    ap.add_argument('--rows', choices=('matrix', 'step', 'all'), default='all')
    ap.add_argument('--budget-gib', type=float, default=40.0, help='baseline (a) is skipped where 4 * B^2 * V bytes exceed this')
    a = ap.parse_args()
    assert a.reps >= 200 or a.out is None, 'a recorded profile needs at least 200 timed iterations'
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(1)
    lines = []
    if not a.append:
        lines += ['the retrieval trainer\'s IoU matrix, [2B, 2B] float32 from normalised float32 targets (ShapeNetV2 constants), %s' % torch.cuda.get_device_name(0),
                  'HIP events around each iteration, %d timed iterations after 20 warm-up (baseline (a): after 3); median (p10 .. p90) in us' % a.reps]
    if a.rows in ('matrix', 'all'):
        matrix_rows(a, lines, dev, gen)
    if a.rows in ('step', 'all'):
        step_rows(a, lines, dev, gen)
    if a.out:
        with open(a.out, 'a' if a.append else 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
