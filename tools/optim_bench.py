"""Dev tool (GPU box): what the optimiser step costs, alone and inside both training steps.

1. One ``step()`` alone -- gradients in place, nothing else on the stream -- of ``torch.optim.Adam`` (default: foreach), ``torch.optim.Adam(fused=True)``
   where this torch accepts it, and ``rfuse.optim.Adam`` (csrc/optim.hip), on the parameters of the C2, C4 and C5 encoder pairs (rfuse/configs.py;
   lr 1e-4, weight decay 5e-5 as trainer/train_retrieval.py:37) and on the phase-3 parameter set of C3 (all four networks, lr 1e-4).  HIP events around
   every step, 20 warm-up steps, median of 5 rounds x 40 steps per optimiser, the optimisers ALTERNATING inside a round (same box, same minute).  An
   event pair spans from the moment the stream reaches the step to its last kernel, so it includes the time the host needs to issue the launches:
   that is what a training step pays.  ``host ms`` is the time ``step()`` takes to return.  bytes/s = 28 bytes per element (p, g, m, v read, p, m, v written).
2. The worst error ratio of tests/test_optim_gpu.py's bar on the C4 pair's tensors: 3 steps along gradients of NT-Xent's size (1e-4), each compared with
   float64 from the kernel's own state; error / diff32 (torch CPU float32 against the same float64), over the tensors of at least 2048 elements and over all.
3. tools/retrieval_train_bench.py (C2, C4, C5) and tools/train_bench.py (C3, B = 4) with ``--optimizer torch`` and ``--optimizer rfuse``, each in a fresh
   process, alternating, 3 rounds; the median ms per step of each.

    python tools/optim_bench.py [--out FILE] [--skip-training]
"""
import argparse
import contextlib
import io
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / 'retrieval-fuse_amd'), str(REPO / 'tests'), str(REPO / 'tools')]
import torch

DEV = torch.device('cuda:0')
ROUNDS, STEPS, WARMUP = 5, 40, 20
LINES = []


def say(text=''):
    print(text, flush=True)
    LINES.append(text)


def parameter_sets():
    import model
    from model import retrieval
    from rfuse import configs as rf_configs
    from retrieval_train_bench import PAIRS
    sets = {}
    for pair, ((qn, qnf, _), (tn, tnf, _), _) in PAIRS.items():
        nets = [getattr(retrieval, qn)(qnf, 64), getattr(retrieval, tn)(tnf, 64)]
        sets['%s pair (%s + %s)' % (pair, qn, tn)] = ([p for n in nets for p in n.parameters()], dict(lr=1e-4, weight_decay=5e-5))
    cfg = rf_configs.get_config('C3')
    with contextlib.redirect_stdout(io.StringIO()):
        mods = [model.get_unet_backbone(cfg), model.get_decoder(cfg), model.get_retrieval_backbone(cfg), model.get_attention_block(cfg)]
    sets['C3 phase 3 (four networks)'] = ([p for m in mods for p in m.parameters()], dict(lr=1e-4))
    return sets


def optimisers():
    from rfuse.optim import Adam
    kinds = [('torch.optim.Adam (foreach)', lambda ps, kw: torch.optim.Adam(ps, **kw))]
    try:
        probe = torch.nn.Parameter(torch.zeros(8, device=DEV))
        probe.grad = torch.zeros_like(probe)
        torch.optim.Adam([probe], fused=True).step()
        torch.cuda.synchronize()
        kinds.append(('torch.optim.Adam(fused=True)', lambda ps, kw: torch.optim.Adam(ps, fused=True, **kw)))
    except Exception as e:                                           # this torch does not take fused=True on this device: say so, measure the others
        say('torch.optim.Adam(fused=True) is not available here: %s' % str(e).splitlines()[0])
    kinds.append(('rfuse.optim.Adam', lambda ps, kw: Adam(ps, **kw)))
    return kinds


def step_alone():
    say('== one optimiser step alone (median of %d rounds x %d steps, optimisers alternating; HIP events per step) ==' % (ROUNDS, STEPS))
    kinds = optimisers()
    g = torch.Generator().manual_seed(0)
    for name, (cpu_params, kw) in parameter_sets().items():
        elements = sum(p.numel() for p in cpu_params)
        say('%s: %d tensors, %d elements (%d of fewer than 2048), %s' % (name, len(cpu_params), elements, sum(p.numel() < 2048 for p in cpu_params), kw))
        runs = []
        for kind, make in kinds:
            ps = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in cpu_params]
            for p in ps:
                p.grad = (torch.randn(p.shape, generator=g) * 1e-4).to(DEV)
            opt = make(ps, kw)
            for _ in range(WARMUP):
                opt.step()
            runs.append((kind, opt, [], []))
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for kind, opt, gpu_ms, host_ms in runs:
                events = []
                for _ in range(STEPS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    t0 = time.perf_counter()
                    opt.step()
                    host_ms.append((time.perf_counter() - t0) * 1e3)
                    e1.record()
                    events.append((e0, e1))
                    torch.cuda.synchronize()                         # every step starts on an idle stream: the pair spans this step alone
                gpu_ms += [a.elapsed_time(b) for a, b in events]
        base = None
        for kind, _, gpu_ms, host_ms in runs:
            ms = statistics.median(gpu_ms)
            base = base or ms
            say('    %-30s %8.4f ms  (host %7.4f ms)  %8.2f GB/s  x%.2f of torch default' % (kind, ms, statistics.median(host_ms), 28 * elements / ms / 1e6, ms / base))
        del runs
    say()


def error_ratio():
    import optim_ref as oref
    from model import retrieval
    from rfuse.optim import Adam
    say('== error against float64, relative to torch CPU float32 (the bar of tests/test_optim_gpu.py is 4) ==')
    torch.manual_seed(1)
    nets = [retrieval.Patch08(16, 64), retrieval.Patch32(8, 64)]
    params = [torch.nn.Parameter(p.detach().clone().to(DEV)) for n in nets for p in n.parameters()]
    opt = Adam(params, lr=1e-4, weight_decay=5e-5)
    g = torch.Generator().manual_seed(2)
    worst = {'large': (0.0, ''), 'all': (0.0, '')}
    for step in range(3):
        before = []
        for p in params:
            p.grad = (torch.randn(p.shape, generator=g) * 1e-4).to(DEV)
            st = opt.state.get(p, {})
            zeros = torch.zeros(p.shape)
            before.append((p.detach().cpu().clone(), st['exp_avg'].cpu().clone() if st else zeros, st['exp_avg_sq'].cpu().clone() if st else zeros.clone()))
        opt.step()
        torch.cuda.synchronize()
        for i, (p, (p0, m0, v0)) in enumerate(zip(params, before)):
            args = (p0, p.grad.cpu(), m0, v0, step, 1e-4, (0.9, 0.999), 1e-8, 5e-5)
            ref, cpu32 = oref.adam_f64(*args), oref.torch_adam(*args)
            got = (p.detach().cpu(), opt.state[p]['exp_avg'].cpu(), opt.state[p]['exp_avg_sq'].cpu())
            for x, c, r, which in zip(got, cpu32, ref, 'pmv'):
                diff32, err = float((c.double() - r).abs().max()), float((x.double() - r).abs().max())
                ratio = err / diff32 if diff32 > 0 else (0.0 if err == 0 or torch.equal(x, r.float()) else float('inf'))
                what = 'tensor %d (%d elements), %s after step %d: error %.3e, diff32 %.3e' % (i, p.numel(), which, step + 1, err, diff32)
                for key in (['large'] if p.numel() >= 2048 else []) + ['all']:
                    if ratio > worst[key][0]:
                        worst[key] = (ratio, what)
    say('C4 pair (Patch08 + Patch32), %d tensors, 3 steps, gradients of 1e-4, weight decay 5e-5' % len(params))
    say('    worst error / diff32 over the tensors of at least 2048 elements: %.3f  (%s)' % worst['large'])
    say('    worst error / diff32 over all tensors:                          %.3f  (%s)' % worst['all'])
    say()


def training_steps():
    say('== the training steps with each optimiser (fresh process per run, alternating, 3 rounds; median ms per step) ==')
    results = {}
    for _ in range(3):
        for optimizer in ('torch', 'rfuse'):
            for tag, cmd in (('retrieval', [sys.executable, str(REPO / 'tools' / 'retrieval_train_bench.py'), 'C2', 'C4', 'C5', '--steps', '30', '--warmup', '5', '--optimizer', optimizer]),
                             ('refinement', [sys.executable, str(REPO / 'tools' / 'train_bench.py'), 'C3', '4', '10', '--optimizer', optimizer, '--no-cpu-oracle'])):
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    raise RuntimeError('%s failed (%d): %s' % (' '.join(cmd), out.returncode, out.stderr[-2000:]))
                for line in out.stdout.splitlines():
                    if line.startswith('{'):
                        d = json.loads(line)
                        key = ('retrieval step %s, B = %d' % (d['pair'], d['batch'])) if tag == 'retrieval' else 'refinement step C3 phase 3, B = %d' % d['chunks_per_step']
                        results.setdefault(key, {}).setdefault(optimizer, []).append(d['ms_per_step'])
    for key, by_opt in results.items():
        t, r = statistics.median(by_opt['torch']), statistics.median(by_opt['rfuse'])
        say('    %-40s torch.optim.Adam %8.3f ms   rfuse.optim.Adam %8.3f ms   (%+.3f ms, %+.1f %%)   runs %s / %s' % (
            key, t, r, r - t, (r - t) / t * 100, [round(x, 3) for x in by_opt['torch']], [round(x, 3) for x in by_opt['rfuse']]))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='file for the text that is printed')
    ap.add_argument('--skip-training', action='store_true', help='leave out part 3 (the two training benches)')
    a = ap.parse_args()
    say('optimiser step: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    say()
    step_alone()
    error_ratio()
    if not a.skip_training:
        training_steps()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
