"""Dev tool (GPU box): one step of the reference's retrieval training (trainer/train_retrieval.py:73-87: both patch encoders forward, normalise,
NTXentLoss(0.2, cosine), backward; Adam lr 1e-4, weight decay 5e-5, :37) through the drop-in ``model`` package in grad mode, for the C2, C4 and C5
encoder pairs at their reference batch sizes.  Prints ms per step (HIP events), a per-kernel table of one profiled step, and achieved TFLOP/s
against the useful conv FLOPs of the SPECs (backward = data gradient of every layer but the first + weight gradient), one JSON line per pair.

    python tools/retrieval_train_bench.py [pair ...] [--steps N] [--warmup W] [--out DIR]
"""
import argparse
import json
import sys
from collections import defaultdict
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / 'retrieval-fuse_amd')]
import torch
import torch.nn.functional as F

from model import retrieval
from model.loss import NTXentLoss
from rfuse import _lib

# pair -> (query class, nf, window), (target class, nf, window), reference train batch
PAIRS = {
    'C2': (('Patch04', 32, 4), ('Patch32', 8, 32), 128),
    'C4': (('Patch08', 16, 8), ('Patch32', 8, 32), 192),
    'C5': (('PCPatch48', 12, 48), ('Patch24V2', 12, 24), 128),
}
NEW_KERNELS = ('rf_conv3d_valid_leaky_backward', 'rf_conv3d_valid_dgrad', 'rf_conv3d_valid_wgrad')


def conv_flops(net, b, win):
    """useful FLOPs of one forward of the conv layers, and of their backward (dgrad skipped on the first layer)"""
    fwd = bwd = 0
    if not isinstance(net, retrieval._ConvPatchEncoder):
        dims = [l.weight.shape for l in net.layers if hasattr(l, 'weight')]
        fwd = sum(2 * b * o * i for o, i in dims)
        return fwd, 2 * fwd
    s = win
    for j, layer in enumerate(l for l in net.layers if hasattr(l, 'kernel_size')):
        so = (s - layer.kernel_size) // layer.stride + 1
        f = 2 * b * layer.out_channels * layer.in_channels * layer.kernel_size ** 3 * so ** 3
        fwd += f
        bwd += f if j == 0 else 2 * f
        s = so
    return fwd, bwd


def run(pair, steps, warmup, optimizer='torch'):
    (qn, qnf, qw), (tn, tnf, tw), b = PAIRS[pair]
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    fq, ft = getattr(retrieval, qn)(qnf, 64).to(dev), getattr(retrieval, tn)(tnf, 64).to(dev)
    if optimizer == 'rfuse':
        from rfuse.optim import Adam
    else:
        Adam = torch.optim.Adam
    opt = Adam(list(fq.parameters()) + list(ft.parameters()), lr=1e-4, weight_decay=5e-5)
    loss_mod = NTXentLoss(0.2, True)
    g = torch.Generator().manual_seed(1)
    xq = (torch.rand(b, 1, qw, qw, qw, generator=g) * 2 - 1).to(dev)
    xt = (torch.rand(b, 1, tw, tw, tw, generator=g) * 2 - 1).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        zq = F.normalize(fq(xq).reshape(b, -1), dim=1)
        zt = F.normalize(ft(xt).reshape(b, -1), dim=1)
        loss = loss_mod(zq, zt)
        loss.backward()
        opt.step()
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps

    records = []
    lib = _lib.load()
    lib.start_profile(records)
    try:
        step()
        torch.cuda.synchronize()
    finally:
        lib.stop_profile()
    table = defaultdict(lambda: [0, 0.0])
    big = {}
    for name, ints, a, z, _ in records:
        t = a.elapsed_time(z)
        table[name][0] += 1
        table[name][1] += t
        # the 12 -> 24 @42^3 layer of PCPatch48 (input 44^3): dgrad ints (n, cout, so, cin, k, stride, s), wgrad ints (n, cin, s, cout, k, stride, ws)
        if name == 'rf_conv3d_valid_dgrad' and ints[1:4] == (24, 42, 12):
            big['dgrad_12_24_ms'] = t
        if name == 'rf_conv3d_valid_wgrad' and ints[1:4] == (12, 44, 24):
            big['wgrad_12_24_ms'] = t
    fl = [conv_flops(fq, b, qw), conv_flops(ft, b, tw)]
    fwd, bwd = sum(f for f, _ in fl), sum(x for _, x in fl)
    new_ms = sum(table[k][1] for k in NEW_KERNELS)
    kern_ms = sum(v[1] for v in table.values())
    out = {'pair': pair, 'batch': b, 'encoders': [qn, tn], 'optimizer': optimizer, 'ms_per_step': round(ms, 3), 'fwd_gflop': round(fwd / 1e9, 2), 'bwd_gflop': round(bwd / 1e9, 2),
           'tflops_step': round((fwd + bwd) / ms / 1e9, 2), 'profiled_kernel_ms': round(kern_ms, 3), 'new_kernels_ms': round(new_ms, 3),
           'new_kernels_share_of_step': round(new_ms / ms, 3)}
    layer_flop = 2 * 128 * 24 * 12 * 27 * 42 ** 3
    for key, t in big.items():
        out[key] = round(t, 3)
        out[key.replace('_ms', '_tflops')] = round(layer_flop / t / 1e9, 2)
    lines = ['%-40s %6s %10s' % ('kernel (one profiled step)', 'calls', 'ms')]
    for name, (calls, t) in sorted(table.items(), key=lambda kv: -kv[1][1]):
        lines.append('%-40s %6d %10.3f' % (name, calls, t))
    return out, '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('pairs', nargs='*', default=list(PAIRS))
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None, help='directory for retrieval_train_<pair>.txt')
    ap.add_argument('--optimizer', choices=['torch', 'rfuse'], default='torch', help='rfuse: the update by rfuse.optim.Adam (csrc/optim.hip); the committed profiles use torch')
    a = ap.parse_args()
    for pair in a.pairs:
        res, table = run(pair, a.steps, a.warmup, a.optimizer)
        print(table)
        print(json.dumps(res), flush=True)
        if a.out:
            Path(a.out).mkdir(parents=True, exist_ok=True)
            (Path(a.out) / ('retrieval_train_%s.txt' % pair)).write_text(table + '\n' + json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
