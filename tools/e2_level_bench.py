"""Dev tool (GPU box): the retrieval backbone's 2^3 level of C2 (n = 8192; 64 ch @4^3 -> pool -> 64 -> 64 -> 128 @2^3, the decoder stage's GroupNorm over 64 skip +
128 upsampled channels) as the six launches of the plain route and as the one launch of rf_conv3d_e2_level, HIP events, the two alternating in one process:
best and median of repeated blocks, and a digest of all outputs so that a variant that changes bits is caught in the same run.

    python tools/e2_level_bench.py [n] [blocks] [reps]"""
import hashlib
import statistics
import sys
from pathlib import Path
REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / 'retrieval-fuse_amd')]
import torch
from rfuse import ops
from model.unet import Encoder, GroupNormParams

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 7
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
dev = torch.device('cuda:0')
torch.manual_seed(0)
enc, dec_gn = Encoder(64, 128, apply_pooling=True).to(dev), GroupNormParams(8, 64 + 128).to(dev)
with torch.no_grad():
    for p in list(enc.parameters()) + list(dec_gn.parameters()):
        if p.dim() == 1:
            p.add_(0.1 * torch.randn_like(p))
    # the tensor the level reads is the one its predecessor has just written (134 MB at n = 8192); the skip tensor is that same tensor
    skip = ops.maxpool2(torch.randn(n, 64, 8, 8, 8, device=dev).relu_())
gn = (dec_gn.weight, dec_gn.bias, dec_gn.num_groups, dec_gn.eps)


def run(fused):
    ops.USE_E2_LEVEL = fused
    with torch.no_grad():
        out = enc(skip, consumer=(skip, dec_gn))
        return out, ops._fresh_stats(out)[0], ops.gn_affine(skip, out, *gn)


def digest(ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def block(fused):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run(fused)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


with torch.no_grad():
    assert enc.level_route(n, 64, 4, skip=(64, 1, 8)) == 'e2_level', 'the one-launch form does not take this shape'
d6, d1 = digest(run(False)), digest(run(True))
for f in (False, True):
    for _ in range(3):
        run(f)
times = {False: [], True: []}
for _ in range(blocks):
    for f in (False, True):
        times[f].append(block(f))
print('n = %d, %d blocks of %d calls each, alternating; us per level (launches back to back on one stream, host enqueue included)' % (n, blocks, reps))
for f, name in ((False, 'six launches'), (True, 'one launch  ')):
    t = times[f]
    print('%s  best %7.1f  median %7.1f  worst %7.1f   blocks %s' % (name, min(t), statistics.median(t), max(t), ' '.join('%.1f' % v for v in t)))
print('digest of (out, statistics, decoder table): six %s  one %s  %s' % (d6, d1, 'EQUAL' if d6 == d1 else 'DIFFERENT'))
