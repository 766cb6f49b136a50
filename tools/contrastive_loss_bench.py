"""Dev tool (GPU box): the contrastive losses' device path (rfuse.losses.AttnContrastiveLoss / NTXent, csrc/ntxent.hip) against the same calls through
``model.loss.NTXentLoss`` in plain torch on the same GPU, in the same process.

    python tools/contrastive_loss_bench.py [--reps 200] [--out profiles/contrastive_loss_bench.txt]

Workloads, forward plus backward to the two feature tensors:
  * the sliced loss of one training step at the reference's batch of 8: N = 8 * 4096 rows, 64 slices of 512, dim 32, tau = 0.05, max_rows = 1280, about
    25 % of the rows occupied, and a fully occupied variant (the first two slices fill 1024 of the 1280 rows; the rest do not fit).  The torch side is the
    trainer's own loop (trainer/train_refinement.py:208-221) around model.loss.NTXentLoss: two host round trips and a boolean index per slice.
  * one NTXent call at B = 128, 192, 512 and 2048 with dim 64, tau = 0.2 (the retrieval trainer, 2048 = its validation batch), with and without the
    [2B, 2B] IoU matrix.
Every figure is the median of --reps iterations, each bracketed by HIP events after a warm-up (the host side of the calls is in it), with the 10th / 90th
percentile as the spread.  The loss values and the largest gradient difference of the two paths are printed beside the times.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / 'retrieval-fuse_amd'))
from model.loss import NTXentLoss                            # noqa: E402
from rfuse.losses import AttnContrastiveLoss, NTXent         # noqa: E402


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


def torch_sliced(crit, num_slices, fpred, ftgt, occupancy, max_rows=1280):
    """compute_sliced_attn_nt_xent_loss as the trainer has it"""
    split = fpred.shape[0] // num_slices
    taken = 0
    loss = torch.zeros(1, dtype=torch.float32, device=fpred.device)
    for b in range(num_slices):
        b_occ = occupancy[b * split:(b + 1) * split] > 0
        if b_occ.sum() > 0 and taken + b_occ.sum().item() <= max_rows:
            loss = crit(fpred[b * split:(b + 1) * split][b_occ], ftgt[b * split:(b + 1) * split][b_occ]) + loss
            taken += b_occ.sum().item()
    return loss


def compare(name, hip, ref, leaves, reps, lines):
    def run(fn):
        loss = fn()
        loss.sum().backward()
        out = (loss.detach().reshape(-1), [t.grad for t in leaves])
        for t in leaves:
            t.grad = None
        return out
    (l_h, g_h), (l_t, g_t) = run(hip), run(ref)
    gerr = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(g_h, g_t))
    t_h, t_t = timed(lambda: run(hip), reps), timed(lambda: run(ref), reps)
    lines.append('%-34s HIP %9.1f (%.1f .. %.1f)   torch %9.1f (%.1f .. %.1f)   torch / HIP = %6.2f   [loss %.6f vs %.6f; gradients differ by %.1e of their maximum]'
                 % (name, *t_h, *t_t, t_t[0] / t_h[0], float(l_h), float(l_t), gerr))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert a.reps >= 200 or a.out is None, 'a recorded profile needs at least 200 timed iterations'
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(1)
    lines = ['contrastive losses, forward and backward to both feature tensors, float32 features, %s' % torch.cuda.get_device_name(0),
             'HIP events around each iteration, %d timed iterations after 20 warm-up; median (p10 .. p90) in us' % a.reps]
    n, dim = 8 * 4096, 32
    ftgt = torch.nn.functional.normalize(torch.randn(n, dim, generator=gen), dim=1)
    fpred = torch.nn.functional.normalize(ftgt + 0.5 * torch.randn(n, dim, generator=gen), dim=1)
    fpred, ftgt = fpred.to(dev).requires_grad_(True), ftgt.to(dev).requires_grad_(True)
    acl, crit = AttnContrastiveLoss(0.05, 1280), NTXentLoss(0.05, True)
    for name, occ in (('sliced, 64 x 512 rows, 25 % occupied', torch.rand(n, generator=gen) < 0.25), ('sliced, 64 x 512 rows, all occupied', torch.ones(n, dtype=torch.bool))):
        occ = occ.to(dev)
        compare(name, lambda: acl(64, fpred, ftgt, occ), lambda: torch_sliced(crit, 64, fpred, ftgt, occ), (fpred, ftgt), a.reps, lines)
        lines[-1] += '   counts %s' % acl.last_counts.tolist()
    for b in (128, 192, 512, 2048):
        zjs = torch.randn(b, 64, generator=gen)
        zis = (zjs + 0.5 * torch.randn(b, 64, generator=gen)).to(dev).requires_grad_(True)
        zjs = zjs.to(dev).requires_grad_(True)
        half = torch.rand(b, b, generator=gen)
        iou = torch.maximum(half, half.t()).fill_diagonal_(1.0).repeat(2, 2).to(dev)
        ntx, crit = NTXent(0.2, True), NTXentLoss(0.2, True)
        compare('NTXent B = %4d, dim 64' % b, lambda: ntx(zis, zjs), lambda: crit(zis, zjs), (zis, zjs), a.reps, lines)
        compare('NTXent B = %4d, dim 64, IoU' % b, lambda: ntx(zis, zjs, iou), lambda: crit(zis, zjs, iou), (zis, zjs), a.reps, lines)
    if a.out:
        Path(a.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
