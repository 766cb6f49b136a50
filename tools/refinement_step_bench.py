"""Dev tool (GPU box): one training step of each phase of the refinement trainer -- forward, backward and rfuse.optim.Adam -- through
``rfuse.training.RefinementStep``, timed with HIP events next to the SAME graph as it ran before that class existed, composed here from the drop-in modules:
the decoder's head in grad mode as the broadcast product torch differentiates, torch's occupancy_from_prediction (threshold, cast, max_pool3d, bool, cast,
unfold, ne, any), and nothing frozen (every network in grad mode, as the reference runs it).

    python tools/refinement_step_bench.py --parent <checkout of the parent commit, built> [--config C3] [--batches 4 8] [--steps 10] [--rounds 3] [--out ..]
    python tools/refinement_step_bench.py                       # without a parent checkout: both halves on this build, in one process

With ``--parent`` the baseline half runs ON THE PARENT'S BUILD (its library, its Python side: none of this commit's needs_input_grad skips), the step half
on this one, each in a fresh process of its own, alternating round by round on one box (box-to-box spread is 3-7 %, tools/abn_bench.sh); the medians
over the rounds are reported.  The baseline half uses nothing this tool's commit added, so this file runs against the parent's tree (``--root``).  Without
``--parent`` the two halves share one process, one build and the modules: the baseline then already has this commit's skips, and the header line says so.

Also: the head's backward alone (rf_pointwise_tanh_backward) with its achieved GB/s against its byte count -- h read, dh written, out and dout read --
and the launches of library entry points per step (torch's own kernels are not in that count: the baseline's head and occupancy are torch kernels).
"""
import argparse
import contextlib
import io
import json
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
_root = [a.split('=', 1)[1] if '=' in a else sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == '--root' or a.startswith('--root=')]
REPO = Path(_root[0]).resolve() if _root else HERE              # the tree whose package and library are measured (before its imports)
sys.path[:0] = [str(REPO), str(REPO / 'retrieval-fuse_amd'), str(REPO / 'tests')]
import torch
import torch.nn.functional as F

import model
from model.attention import Fold3D, Unfold3D
from rfuse import _lib, configs as rf_configs
from rfuse.losses import AttnContrastiveLoss, ShapeLoss
from rfuse.optim import Adam

NETWORKS = ('unet_backbone', 'decoder', 'retrieval_backbone', 'patched_attention_block')
PHASE_NETWORKS = (('unet_backbone', 'decoder'), ('retrieval_backbone',), ('patched_attention_block',), NETWORKS)
SIDE = {'loss_side_task_retr': 0.5, 'loss_side_task_unet': 0.25}          # the bench's own choice; the weights do not change the work


class BaselineStep:
    """the four training steps with the pieces that existed before rfuse.training: see the module docstring"""

    def __init__(self, phase, mods, cfg):
        self.phase, self.m, self.cfg = phase, mods, cfg
        d = cfg['dataset_train']
        self.trunc, self.thr = rf_configs.truncations(cfg)[1], d['voxel_size_target'] * 0.75
        self.shape_loss, self.loss_attn = ShapeLoss.from_config(cfg), AttnContrastiveLoss(0.05, 1280)
        nf = mods['retrieval_backbone'].nf
        self.unfold_shape, self.unfold_features, self.fold_shape, self.fold_features = Unfold3D(16, 1), Unfold3D(8, nf), Fold3D(4, 16, 1), Fold3D(4, 8, nf)

    def parameters(self):
        return [p for net in PHASE_NETWORKS[self.phase] for p in self.m[net].parameters()]

    def decoder(self, x):
        dec = self.m['decoder']
        x = dec.network[0](x)
        w, b = dec.network[1].weight, dec.network[1].bias
        return torch.tanh((x.unsqueeze(1) * w.view(1, w.shape[0], w.shape[1], 1, 1, 1)).sum(dim=2) + b.view(1, -1, 1, 1, 1))

    def occupancy(self, pred):
        df = (pred + 1) * self.trunc / 2
        return F.max_pool3d((df <= self.thr).float(), kernel_size=2, stride=2).bool().detach()

    def training_step(self, batch):
        m, sl = self.m, self.shape_loss
        sl.augment_batch_data(batch)
        if self.phase == 0:
            return sl.loss_shape(self.decoder(m['unet_backbone'](batch['input'])), batch)[0]
        if self.phase == 1:
            return sl.loss_shape(self.fold_shape(self.decoder(m['retrieval_backbone'](self.unfold_shape(batch['target'])))), batch)[0]
        b, k = batch['target'].shape[0], self.cfg['K']
        x_back = m['unet_backbone'](batch['input'])
        if self.phase == 2:
            x_target = self.fold_features(m['retrieval_backbone'](self.unfold_shape(batch['target'])))
            fpred, ftgt, occ = m['patched_attention_block'].get_features(x_back, x_target, self.occupancy(self.decoder(x_back)))
            return self.loss_attn(b * 8, fpred, ftgt, occ)
        retrievals = batch['retrieval'][:, :k].reshape(b * k, 1, 64, 64, 64)
        both = self.fold_features(m['retrieval_backbone'](self.unfold_shape(torch.cat([retrievals, batch['target']], 0))))
        x_retrieval, x_target = both[:b * k], both[b * k:]
        pred = self.decoder(m['patched_attention_block'](x_back, x_retrieval))
        pred_retr = self.fold_shape(self.decoder(self.unfold_features(x_target)))
        pred_back = self.decoder(x_back)
        fpred, ftgt, occ = m['patched_attention_block'].get_features(x_back, x_target, self.occupancy(pred_back))
        return (sl.loss_shape(pred, batch)[0] + self.loss_attn(b * 8, fpred, ftgt, occ) * 0.01 + sl.loss_shape(pred_retr, batch)[0] * SIDE['loss_side_task_retr']
                + sl.loss_shape(pred_back, batch)[0] * SIDE['loss_side_task_unet'])


def libraries():
    libs = [_lib.load(), _lib.load_train(), _lib.load_contrastive(), _lib.load_attn_train(), _lib.load_level(), _lib.load_optim()]
    if hasattr(_lib, 'load_step'):
        libs.append(_lib.load_step())
    return libs


def make_runner(step, data, new):
    opt = Adam(step.parameters(), lr=1e-5)

    def run():
        opt.zero_grad(set_to_none=True)
        batch = dict(data)
        loss = step.training_step(batch)['loss'] if new else step.training_step(batch)
        loss.sum().backward()
        opt.step()
    return run


def timed(run, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def launches(run):
    records = []
    libs = libraries()
    for lib in libs:
        lib.start_profile(records)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        for lib in libs:
            lib.stop_profile()
    names = [r[0] for r in records if _lib.is_status(r[0], next(lib._table for lib in libs if r[0] in lib._table))]
    return len(names), sum(n.endswith(('wgrad', 'wgrad_split')) for n in names)


def head_alone(B, nf, dev, steps=20):
    from rfuse import ops
    g = torch.Generator().manual_seed(1)
    h = torch.randn(B, nf, 64, 64, 64, generator=g).relu().to(dev)
    out = torch.tanh(torch.randn(B, 1, 64, 64, 64, generator=g)).to(dev)
    dout = torch.randn(B, 1, 64, 64, 64, generator=g).to(dev)
    w = torch.randn(1, nf, 1, 1, 1, generator=g).to(dev)
    run = lambda: ops.pointwise_tanh_backward(h, out, dout, w)
    timed(run, 3)
    ms = min(timed(run, steps) for _ in range(3))
    nbytes = B * 64 ** 3 * 4 * (2 * nf + 2)
    return ms, nbytes


def measure(args, halves):
    """-> {'B,phase': {half: ([ms per round], launches, weight-gradient launches)}}, {'B': (head ms, bytes)}: ``halves`` of ('baseline', 'step') in this process"""
    cfg = rf_configs.get_config(args.config)
    trunc = rf_configs.truncations(cfg)[1]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        mods = {'unet_backbone': model.get_unet_backbone(cfg), 'decoder': model.get_decoder(cfg), 'retrieval_backbone': model.get_retrieval_backbone(cfg),
                'patched_attention_block': model.get_attention_block(cfg)}
    for m in mods.values():
        m.to(dev).train()
    S, K = cfg['dataset_train']['input_chunk_size'], cfg['K']
    table, heads = {}, {}
    for B in args.batches:
        gen = torch.Generator().manual_seed(3)
        data = {'input': torch.randn(B, 1, S, S, S, generator=gen).to(dev), 'retrieval': torch.randn(B, K, 64, 64, 64, generator=gen).to(dev),
                'target': (torch.rand(B, 1, 64, 64, 64, generator=gen) * trunc).to(dev)}
        for phase in range(4):
            runners = {}
            if 'baseline' in halves:
                runners['baseline'] = make_runner(BaselineStep(phase, mods, cfg), data, False)
            if 'step' in halves:
                from rfuse.training import RefinementStep
                runners['step'] = make_runner(RefinementStep.from_config(cfg, phase, mods, **(SIDE if phase == 3 else {})), data, True)
            times = {k: [] for k in runners}
            for run in runners.values():
                timed(run, 2)
            for _ in range(args.rounds):
                for k, run in runners.items():
                    times[k].append(timed(run, args.steps))
            table['%d,%d' % (B, phase)] = {k: (times[k],) + launches(run) for k, run in runners.items()}
        if 'step' in halves:
            heads[str(B)] = head_alone(B, cfg['nf'], dev)
    return table, heads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C3')
    ap.add_argument('--batches', type=int, nargs='+', default=[4, 8])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent', help='a built checkout of the parent commit: the baseline half runs there, in processes of its own')
    ap.add_argument('--root', help='(used by --parent) the tree to import the package from')
    ap.add_argument('--only', choices=['baseline', 'step'], help='(used by --parent) one half, one round, results as JSON to --json')
    ap.add_argument('--json')
    ap.add_argument('--out', default=str(HERE / 'profiles' / 'refinement_step_bench.txt'))
    args = ap.parse_args()
    if args.only:
        args.rounds = 1
        table, heads = measure(args, (args.only,))
        Path(args.json).write_text(json.dumps({'table': table, 'heads': heads}))
        return
    if args.parent:
        table, heads = {}, {}
        common = ['--config', args.config, '--steps', str(args.steps), '--batches'] + [str(b) for b in args.batches]
        with tempfile.TemporaryDirectory() as tmp:
            for rnd in range(args.rounds):
                for half, root in (('baseline', str(Path(args.parent).resolve())), ('step', str(HERE))):
                    out = Path(tmp) / ('%s_%d.json' % (half, rnd))
                    subprocess.run([sys.executable, str(Path(__file__).resolve()), '--root', root, '--only', half, '--json', str(out)] + common, check=True,
                                   cwd=root, timeout=600)
                    got = json.loads(out.read_text())
                    for key, halves in got['table'].items():
                        ms, n, nw = halves[half]
                        entry = table.setdefault(key, {}).setdefault(half, ([], n, nw))
                        entry[0].extend(ms)
                    for B, (ms, nbytes) in got['heads'].items():
                        if B not in heads or ms < heads[B][0]:
                            heads[B] = (ms, nbytes)
        how = 'baseline on the parent commit\'s build, step on this one, a fresh process each, alternating round by round on one box'
    else:
        table, heads = measure(args, ('baseline', 'step'))
        how = 'both halves in ONE process on THIS build (the baseline has this commit\'s needs_input_grad skips), alternating'
    lines = ['refinement training step, %s, forward + backward + rfuse.optim.Adam, ms per step: median of %d rounds of %d steps' % (args.config, args.rounds, args.steps),
             how,
             '%-3s %-5s %12s %12s %8s   %s' % ('B', 'phase', 'baseline ms', 'step ms', 'ratio', 'library launches per step (of them weight gradients): baseline -> step')]
    for B in args.batches:
        for phase in range(4):
            e = table['%d,%d' % (B, phase)]
            med = {k: statistics.median(v[0]) for k, v in e.items()}
            lines.append('%-3d %-5d %12.3f %12.3f %8.3f   %d (%d) -> %d (%d)' % (B, phase, med['baseline'], med['step'], med['step'] / med['baseline'],
                                                                             e['baseline'][1], e['baseline'][2], e['step'][1], e['step'][2]))
        ms, nbytes = heads[str(B)]
        lines.append('B = %d: head backward alone (rf_pointwise_tanh_backward) [%d, %d, 64^3]: %.4f ms, %.1f MB by byte count (h read, dh written, out and dout read), '
                     '%.0f GB/s' % (B, B, rf_configs.get_config(args.config)['nf'], ms, nbytes / 1e6, nbytes / ms / 1e6))
    print('\n'.join(lines))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
