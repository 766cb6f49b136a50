"""Fixture generator for the evaluation metrics (CPU; needs the reference checkout, as oracle/gen_golden.py does):
runs the reference's own ``util/metrics.py`` classes on seeded occupancy grids and writes tests/golden/metrics.npz.

The reference imports two packages this image lacks; they are stood in for through ``sys.modules``:
  * ``torchmetrics.metric.Metric``: the part of it the reference touches -- ``add_state`` sets a tensor attribute, ``forward`` calls ``update``;
  * ``external.ChamferDistancePytorch.chamfer3D.dist_chamfer_3D.chamfer_3DDist``: an exact brute-force search.  ASSUMPTION: like the CUDA
    extension it replaces (whose source is not in the reference tree), it returns SQUARED Euclidean distances -- dist1 [1, n1] from every point
    of the first cloud to its nearest point of the second, dist2 [1, n2] the other way -- and zeros for a side whose other cloud is empty.

    python tools/gen_metrics_golden.py

Layout of the fixture (one entry per ``update`` call u; every volume [B, 1, D, H, W]):
  u{u}_shape        int64 [5]
  u{u}_pred / _target  uint8: np.packbits of the bool grids (C order)
  u{u}_stats        int64 [B, 5]: n_pred, n_target, n_inter and the squared-distance sums the stand-in returned (s_tp = sum dist1, s_pt = sum dist2;
                    0 where a cloud is empty)
  u{u}_states       float32 [8]: iou_sum, IoU.total, cd_sum, Chamfer3D.total, precision_sum, Precision.total, recall_sum, Recall.total after the call
  compute           float32 [4]: IoU, Chamfer3D, Precision, Recall .compute() after the last call
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from oracle.gen_golden import REF, save_fixture        # noqa: E402  (the reference checkout, and the churn-free writer)
from rfuse import configs as rf_configs                 # noqa: E402  (gen_golden put the product package on the path)
from rfuse import synthetic                             # noqa: E402

_CALLS = []


class _Metric(torch.nn.Module):
    def __init__(self, compute_on_step=True, **kwargs):
        super().__init__()
        self.compute_on_step = compute_on_step

    def add_state(self, name, default, dist_reduce_fx=None):
        setattr(self, name, default.clone())

    def forward(self, *args):
        self.update(*args)
        return self.compute() if self.compute_on_step else None


class _ExactChamfer(torch.nn.Module):
    def forward(self, xyz1, xyz2):
        a, b = xyz1[0].double(), xyz2[0].double()

        def nearest(p, q):
            if len(q) == 0:
                return torch.zeros(len(p), dtype=torch.float64)
            return torch.cat([((p[i:i + 512, None, :] - q[None]) ** 2).sum(-1).min(1).values for i in range(0, len(p), 512)]) \
                if len(p) else torch.zeros(0, dtype=torch.float64)
        d1, d2 = nearest(a, b), nearest(b, a)
        _CALLS.append((int(d1.sum().item()), int(d2.sum().item())))
        z1, z2 = torch.zeros(1, len(a), dtype=torch.int32), torch.zeros(1, len(b), dtype=torch.int32)
        return d1.float()[None], d2.float()[None], z1, z2


def import_reference_metrics():
    for n in ('torchmetrics', 'torchmetrics.metric', 'external', 'external.ChamferDistancePytorch', 'external.ChamferDistancePytorch.chamfer3D'):
        sys.modules[n] = types.ModuleType(n)
    sys.modules['torchmetrics.metric'].Metric = _Metric
    dist_mod = types.ModuleType('external.ChamferDistancePytorch.chamfer3D.dist_chamfer_3D')
    dist_mod.chamfer_3DDist = _ExactChamfer
    sys.modules['external.ChamferDistancePytorch.chamfer3D'].dist_chamfer_3D = dist_mod
    for k in [k for k in sys.modules if k == 'util' or k.startswith('util.')]:
        del sys.modules[k]
    sys.path.insert(0, str(REF))
    import util.metrics as ref_metrics
    assert str(REF) in ref_metrics.__file__, ref_metrics.__file__
    return ref_metrics


def _occ(seed, cfg):
    return synthetic.make_chunk(seed, cfg)['target_raw'] <= np.float32(0.75 * cfg['dataset_train']['voxel_size_target'])


def _blobs(rng, shape, n):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing='ij'), -1).astype(np.float64)
    occ = np.zeros(shape, bool)
    for _ in range(n):
        c, r = rng.uniform(0, shape), rng.uniform(2.0, 6.0)
        occ |= np.abs(np.linalg.norm(g - c, axis=-1) - r) <= 0.8
    return occ


def updates():
    """[(pred, target)] of bool [B, 1, D, H, W]: normal chunks, identical grids, empty pred, single voxels at opposite corners; a shifted chunk, empty
    target, both empty; a non-cubic pair"""
    cfg = rf_configs.get_config('C2')
    t0, t1, t2 = _occ(0, cfg), _occ(1, cfg), _occ(2, cfg)
    p0 = _occ(100, cfg)
    empty = np.zeros((64, 64, 64), bool)
    corner_a, corner_b = empty.copy(), empty.copy()
    corner_a[0, 0, 0] = True
    corner_b[63, 63, 63] = True
    u0 = (np.stack([p0, t1, empty, corner_a]), np.stack([t0, t1, t2, corner_b]))
    u1 = (np.stack([np.roll(t2, (2, -1, 3), axis=(0, 1, 2)), t0, empty]), np.stack([t2, empty, empty]))
    rng = np.random.default_rng(7)
    u2 = (np.stack([_blobs(rng, (24, 40, 70), 3) for _ in range(2)]), np.stack([_blobs(rng, (24, 40, 70), 3) for _ in range(2)]))
    return [(p[:, None], t[:, None]) for p, t in (u0, u1, u2)]


def main():
    ref = import_reference_metrics()
    metrics = [ref.IoU(compute_on_step=False), ref.Chamfer3D(compute_on_step=False), ref.Precision(compute_on_step=False),
               ref.Recall(compute_on_step=False)]
    names = [('iou_sum', 'total'), ('cd_sum', 'total'), ('precision_sum', 'total'), ('recall_sum', 'total')]
    out = {}
    for u, (pred, target) in enumerate(updates()):
        pt, tt = torch.from_numpy(pred), torch.from_numpy(target)
        _CALLS.clear()
        for m in metrics:
            m(pt, tt)
        B = pred.shape[0]
        assert len(_CALLS) == B
        stats = np.zeros((B, 5), np.int64)
        for b in range(B):
            stats[b, :3] = pred[b].sum(), target[b].sum(), (pred[b] & target[b]).sum()
            if stats[b, 0] and stats[b, 1]:
                stats[b, 3:] = _CALLS[b]            # chamfer(points_target, points_pred): dist1 over the target points, dist2 over the predicted ones
        out['u%d_shape' % u] = np.array(pred.shape, np.int64)
        out['u%d_pred' % u] = np.packbits(pred.reshape(-1))
        out['u%d_target' % u] = np.packbits(target.reshape(-1))
        out['u%d_stats' % u] = stats
        out['u%d_states' % u] = np.array([float(getattr(m, n)) for m, ns in zip(metrics, names) for n in ns], np.float32)
    out['compute'] = np.array([float(m.compute()) for m in metrics], np.float32)
    save_fixture('metrics', **out)
    print({k: v.tolist() for k, v in out.items() if k.endswith(('states', 'stats')) or k == 'compute'})


if __name__ == '__main__':
    main()
