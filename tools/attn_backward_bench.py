"""Dev tool (GPU box): the patch-attention stage of the training graph (PatchedAttentionBlock.forward in grad mode, forward + backward) through the
HIP route (rfuse.autograd.AttnFuse / Unfold3d / Fold3d / GatherRetrieved: rf_attn_fuse + rf_attn_fuse_backward and the index-map kernels) against the
element-wise torch formula the modules used before (tests/attention_backward_ref.py:torch_patched_forward), in the same process on the same GPU.

    python tools/attn_backward_bench.py [--reps 200] [--parent-root DIR [--train-rounds 3]] [--out profiles/attn_backward_bench.txt]

Per config (C3 B = 4: softmax, K = 4; C1 B = 4: Gumbel-hard; C4 B = 4: K = 8; x_predicted [B,nf,32^3], retrieved [B*K,nf,32^3], 4096 rows per chunk):
  stage time     median (p10 .. p90) of --reps iterations, each bracketed by HIP events after a warm-up (the host side of the calls is in it)
  launches       device kernels of one iteration, from a torch.profiler trace
  peak bytes     torch.cuda.max_memory_allocated over one iteration, above what was allocated before it
  backward kernel  rf_attn_fuse_backward alone on the stage's shapes, and its byte floor: per row it reads (2 + K) d + (1 + K) f + K floats and writes
                 (1 + K) (d + f), at 4.5 TB/s
The accuracy table is that of tests/test_attention_backward_gpu.py (same inputs, same float64 reference, same comparator).
--parent-root DIR: a checkout of the parent commit with its library built; runs tools/train_bench.py C3 4 of both trees in child processes, alternating.
"""
import argparse
import contextlib
import io
import json
import statistics
import subprocess
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / 'retrieval-fuse_amd'), str(REPO / 'tests')]
import attention_backward_ref as ref      # noqa: E402
import model                              # noqa: E402
from rfuse import configs, ops            # noqa: E402

HBM_BYTES_PER_S = 4.5e12


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


def peak_bytes(fn, dev):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base


def accuracy_table(dev):
    lines = ['accuracy: max-abs error / max-abs of the float64 reference on the same float32 inputs, R = 2048, d = 128, f = 32 (rows with a discrete '
             'decision within rounding left out)']
    for K in (4, 8):
        for mode, a in ((ref.SOFTMAX, 1024.0), (ref.GUMBEL_HARD, 25.0)):
            inp = ref.make_inputs(2048, K, 128, 32, 0)
            want = ref.reference_f64(*inp, mode, a)
            keep = want['score_gap'] >= 1e-6
            if mode == ref.GUMBEL_HARD:
                keep &= want['logit_gap'] >= 1e-4
            x, p, xf, pf, noise, dout = (t.to(dev) for t in inp)
            got = ops.attn_fuse_backward(x, p, xf, pf.reshape(-1, 32), noise if mode == ref.GUMBEL_HARD else None, dout, mode, a)
            old = ref.torch_formula_grads(x, p, xf, pf, noise, dout, mode, a)
            cells = []
            for name, g, c in zip(('dx', 'dp', 'dxf', 'dpf'), got, old):
                w = want[name][keep]
                cells.append('%s hip %.2e torch %.2e' % (name, ref.rel_err(g.cpu().reshape(want[name].shape)[keep], w),
                                                         ref.rel_err(c.cpu().reshape(want[name].shape)[keep], w)))
            lines.append('  K = %d %-11s %4d rows out   %s' % (K, 'softmax' if mode == ref.SOFTMAX else 'Gumbel-hard', int((~keep).sum()), '   '.join(cells)))
    return lines


def stage(name, B, reps, dev):
    cfg = configs.get_config(name)
    K, nf = cfg['K'], cfg['nf']
    with contextlib.redirect_stdout(io.StringIO()):
        block = model.get_attention_block(cfg).to(dev).train()
    gen = torch.Generator().manual_seed(B)
    xp = torch.randn(B, nf, 32, 32, 32, generator=gen).to(dev).requires_grad_(True)
    xr = torch.randn(B * K, nf, 32, 32, 32, generator=gen).to(dev).requires_grad_(True)
    dout = torch.randn(B, nf, 32, 32, 32, generator=gen).to(dev)
    rows = B * 4096
    noise = (-torch.empty(rows, K).exponential_(generator=gen).log()).to(dev) if cfg['attn_retrieval_mode'] else None

    def run(forward):
        forward().backward(dout)
        for t in [xp, xr] + list(block.parameters()):
            t.grad = None
    run_new = lambda: run(lambda: block(xp, xr, noise))
    run_old = lambda: run(lambda: ref.torch_patched_forward(block, xp, xr, 0, 0, noise))
    res = {}
    for tag, fn in (('HIP', run_new), ('torch formula', run_old)):
        res[tag] = timed(fn, reps) + (launches(fn), peak_bytes(fn, dev))
    lines = ['%s B = %d (%d rows, K = %d, %d channels x 2^3, %s)' % (name, B, rows, K, nf, 'Gumbel-hard' if noise is not None else 'softmax')]
    for tag in ('HIP', 'torch formula'):
        lines.append('  %-14s stage forward + backward %9.1f us (%.1f .. %.1f), %s launches, peak %.1f MB' % (tag, *res[tag][:4], res[tag][4] / 1e6))
    lines.append('  torch formula / HIP = %.2f' % (res['torch formula'][0] / res['HIP'][0]))

    # the backward kernel alone
    d, f = nf * 8, 32
    mode, a = (ref.GUMBEL_HARD, 25.0) if noise is not None else (ref.SOFTMAX, 1024.0)
    x, p = torch.randn(rows, d, generator=gen).to(dev), torch.randn(rows, K, d, generator=gen).to(dev)
    xf = torch.randn(rows, f, generator=gen)
    pf = (xf[:, None] * (1 + 0.3 * torch.rand(rows, K, 1, generator=gen)) + 0.1 * torch.randn(rows, K, f, generator=gen)).reshape(rows * K, f).to(dev)
    xf, g = xf.to(dev), torch.randn(rows, d, generator=gen).to(dev)
    med, lo, hi = timed(lambda: ops.attn_fuse_backward(x, p, xf, pf, noise, g, mode, a), reps)
    nbytes = 4 * rows * ((2 + K) * d + (1 + K) * f + K + (1 + K) * (d + f))
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    lines.append('  rf_attn_fuse_backward alone (with its four output allocations) %7.1f us (%.1f .. %.1f); %.1f MB -> byte floor %.1f us at 4.5 TB/s: %.2f of the floor'
                 % (med, lo, hi, nbytes / 1e6, floor_us, floor_us / med))
    return lines


def train_lines(parent_root, rounds=3):
    lines = ['tools/train_bench.py C3 4 20, parent commit and this one in child processes on this box, alternating (ms per training step)']
    for i in range(rounds):
        for tag, root in (('parent', Path(parent_root).resolve()), ('this', REPO)):
            out = subprocess.run([sys.executable, str(root / 'tools' / 'train_bench.py'), 'C3', '4', '20'], capture_output=True, text=True, cwd=str(root))
            try:
                d = json.loads(out.stdout.strip().splitlines()[-1])
                top = ', '.join('%s %.2f' % kv for kv in list(d['hip_entry_points_ms'].items())[:4])
                lines.append('  round %d %-6s %.3f ms/step   loss %.6f   HIP entry points %.2f ms (%s)' % (i, tag, d['ms_per_step'], d['loss'], d['hip_ms_total'], top))
            except Exception:
                lines.append('  round %d %-6s failed: %s' % (i, tag, (out.stderr or out.stdout)[-300:]))
            print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--train-rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert a.reps >= 200 or a.out is None, 'a recorded profile needs at least 200 timed iterations'
    dev = torch.device('cuda:0')
    lines = ['patch-attention stage in grad mode (PatchedAttentionBlock.forward, forward + backward), HIP route vs the element-wise torch formula, %s'
             % torch.cuda.get_device_name(0), 'HIP events around each iteration, %d timed iterations after 20 warm-up; median (p10 .. p90)' % a.reps]
    for name in ('C3', 'C1', 'C4'):
        lines += stage(name, 4, a.reps, dev)
        print('\n'.join(lines[-5:]), flush=True)
    lines += accuracy_table(dev)
    print('\n'.join(lines[-5:]), flush=True)
    if a.parent_root:
        lines += train_lines(a.parent_root, a.train_rounds)
    text = '\n'.join(lines) + '\n'
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    print(text)


if __name__ == '__main__':
    main()
