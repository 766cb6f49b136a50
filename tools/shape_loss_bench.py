"""Dev tool (GPU box): the shape loss's device path (rfuse.losses.ShapeLoss, csrc/shape_loss.hip) against the same formulas in plain torch on the same
GPU, in the same process.

    python tools/shape_loss_bench.py [--reps 200] [--batches 4 32] [--no-step] [--out profiles/shape_loss_bench.txt]

Workload: what the loss costs one training_step_full of the reference's trainer -- one augment_batch_data and the three loss_shape calls (fused, backbone-only
and retrieval-only predictions), forward and backward to the three predictions, on [B,1,64,64,64] volumes.  Every figure is the median of --reps
iterations, each bracketed by HIP events after a warm-up (the host side of the calls is in it), with the 10th / 90th percentile as the spread.  Launches are
counted from a torch.profiler trace of one iteration.

The torch side is written from the formulas (README / include/rfuse_train.h), not from the reference: one conv3d with the three stencils stacked, and masked
sums in place of the reference's boolean index, so it has no device-to-host sync either -- the comparison is against the better torch formulation.

Unless --no-step: runs tools/train_bench.py C3 4 in a child process afterwards and prints what share of that step the torch formulation would have been.
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / 'retrieval-fuse_amd'))
from rfuse import configs, synthetic      # noqa: E402
from rfuse.losses import ShapeLoss        # noqa: E402

W_OCC, LAM_REC, LAM_N = 8, 1, 0.5


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


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA'))
    except Exception as exc:      # a profiler that does not work here costs the count, not the timing
        return 'n/a (%s)' % type(exc).__name__


class TorchShapeLoss:
    """the formulas in plain torch"""

    def __init__(self, trunc, mean, std, dev):
        self.trunc, self.mean, self.std = trunc, mean, std
        s, d = torch.tensor([1., 2., 1.], device=dev), torch.tensor([1., 0., -1.], device=dev)
        outer = lambda a, b, c: a[:, None, None] * b[None, :, None] * c[None, None, :]
        self.k = torch.stack([outer(d, s, s), outer(s, d, s), outer(s, s, -d)])[:, None]

    def sobel(self, v):
        return F.conv3d(F.pad(v, (1,) * 6, value=self.trunc), self.k)

    def normals(self, v):
        g = self.sobel(v)
        return g / torch.sqrt((g * g).sum(1, keepdim=True) + 1e-5)

    @torch.no_grad()
    def augment(self, batch):
        t = batch['target']
        batch['normals'] = self.normals(t * self.std + self.mean)
        batch['weights'] = 1 + (t < self.trunc).float() * (W_OCC - 1)
        batch['empty'] = t >= self.trunc

    def loss(self, pred, batch):
        df = (pred + 1) * self.trunc / 2
        w = torch.where(batch['empty'] & (df >= self.trunc), torch.zeros_like(pred), batch['weights'])
        l1 = ((pred - (2 * ((batch['target'] * self.std + self.mean) / self.trunc) - 1)).abs() * w).mean()
        n_p, n_t = self.normals(df), batch['normals']
        valid = (n_p.norm(dim=1) != 0) & (n_t.norm(dim=1) != 0)
        cos = F.cosine_similarity(F.normalize(n_p, dim=1), F.normalize(n_t, dim=1), dim=1)
        normal = 1 - (cos * valid).sum() / valid.sum()
        return LAM_REC * l1 + LAM_N * normal, l1, normal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--batches', type=int, nargs='+', default=[4, 32])
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert a.reps >= 200 or a.out is None, 'a recorded profile needs at least 200 timed iterations'
    dev = torch.device('cuda:0')
    cfg = configs.get_config('C3')
    d = cfg['dataset_train']
    trunc = configs.truncations(cfg)[1]
    lines = ['shape loss, one training_step_full worth: 1 x augment_batch_data + 3 x loss_shape, forward and backward, [B,1,64,64,64] float32, %s'
             % torch.cuda.get_device_name(0), 'HIP events around each iteration, %d timed iterations after 20 warm-up; median (p10 .. p90) in us' % a.reps]
    torch_us, hip_us = {}, {}
    for B in a.batches:
        raw = np.stack([synthetic.make_chunk(s, cfg)['target_raw'] for s in range(B)])[:, None].astype(np.float32)
        target = torch.from_numpy((raw - np.float32(d['target_mean'])) / np.float32(d['target_std'])).to(dev)
        gen = torch.Generator().manual_seed(B)
        preds = [torch.clamp(torch.from_numpy(2 * raw / trunc - 1) + 0.3 * torch.randn(raw.shape, generator=gen), -1, 1).to(dev).requires_grad_(True) for _ in range(3)]
        hip, ref = ShapeLoss.from_config(cfg), TorchShapeLoss(trunc, d['target_mean'], d['target_std'], dev)

        def run(augment, loss):
            batch = {'target': target}
            augment(batch)
            total = sum(loss(p, batch)[0] for p in preds)
            total.backward()
            out = (total.detach(), [p.grad for p in preds])
            for p in preds:
                p.grad = None
            return out
        run_hip = lambda: run(hip.augment_batch_data, hip.loss_shape)
        run_torch = lambda: run(ref.augment, ref.loss)
        (t_h, g_h), (t_t, g_t) = run_hip(), run_torch()
        gerr = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(g_h, g_t))
        res = {}
        for name, fn in (('hip', run_hip), ('torch', run_torch)):
            res[name] = timed(fn, a.reps) + (launches(fn),)
        torch_us[B], hip_us[B] = res['torch'][0], res['hip'][0]
        lines.append('B = %2d   HIP %9.1f (%.1f .. %.1f), %s launches   torch %9.1f (%.1f .. %.1f), %s launches   torch / HIP = %.2f   '
                     '[sum of the three totals %.6f vs %.6f; gradients differ by %.1e of their maximum]'
                     % (B, *res['hip'], *res['torch'], res['torch'][0] / res['hip'][0], float(t_h), float(t_t), gerr))
        print(lines[-1], flush=True)
        del preds, target
        torch.cuda.empty_cache()
    if not a.no_step and 4 in torch_us:
        out = subprocess.run([sys.executable, str(REPO / 'tools' / 'train_bench.py'), 'C3', '4', '20'], capture_output=True, text=True, timeout=900)
        step = json.loads(out.stdout.strip().splitlines()[-1])['ms_per_step']
        lines.append('tools/train_bench.py C3, B = 4 (L1 stand-in loss): %.2f ms per step; the torch formulation of the shape loss above is %.2f ms = %.1f %% of that step, '
                     'the HIP path %.1f %%' % (step, torch_us[4] / 1e3, 100 * torch_us[4] / 1e3 / step, 100 * hip_us[4] / 1e3 / step))
        print(lines[-1], flush=True)
    if a.out:
        Path(a.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
