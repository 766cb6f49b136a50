"""Evaluation metrics on the device: the reference's ``util/metrics.py:6-89`` (IoU, Chamfer3D, Precision, Recall -- imported by
trainer/train_refinement.py:16) and ``util/retrieval.py:167-175`` ``get_metrics_for_retrieval``.

The reference's Chamfer3D takes ``torch.nonzero`` of every volume (a host sync each) and runs the un-vendored ``chamfer_3DDist`` brute-force
search over the points.  Here one launch sequence (csrc/metrics.hip, ``rf_occupancy_stats``) gives per volume the exact int64 counts n_pred,
n_target, n_inter and the two directed sums of squared nearest-neighbour distances (a squared Euclidean distance transform on the voxel grid);
the metrics apply the reference's float32 expressions to them on the device.  No host synchronisation, no loop over volumes.

    stats = occupancy_stats(pred_bool, target_bool)              # int64 [B, 5]: n_pred, n_target, n_inter, s_tp, s_pt
    metrics = torch.nn.ModuleList([IoU(compute_on_step=False), Chamfer3D(compute_on_step=False),
                                   Precision(compute_on_step=False), Recall(compute_on_step=False)]).cuda()
    for m in metrics: m(pred_bool, target_bool)
    iou, cd, precision, recall = (m.compute() for m in metrics)

The metric classes need no torchmetrics: they are ``torch.nn.Module`` s whose states are float32 tensors with the reference's names and whose
``compute()`` sums the states over ``process_group`` when torch.distributed runs with several ranks (torchmetrics' ``dist_reduce_fx="sum"``).
As in torchmetrics the states are plain tensor attributes that ``.to()`` / ``.cuda()`` move (``_apply``), not buffers: a checkpoint of the module
that holds them has no metric keys, and DistributedDataParallel, which broadcasts every buffer from rank 0 before each forward, never sees them --
each rank keeps its own sums until ``compute()`` adds them up.
"""
import torch

from . import _lib
from .ops import _p, _stream, _device_scoped

OCC_GRID, OCC_DF_F32, OCC_DF_F16 = 0, 1, 2          # include/rfuse.h RF_OCC_*
_KINDS = {torch.bool: OCC_GRID, torch.uint8: OCC_GRID, torch.float32: OCC_DF_F32, torch.float16: OCC_DF_F16}


def _operand(t, threshold, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor' % what)
    if not t.is_cuda:
        raise RuntimeError('%s: the evaluation metrics run on the GPU only (got a %s tensor); there is no CPU fallback' % (what, t.device))
    kind = _KINDS.get(t.dtype)
    if kind is None:
        raise ValueError('%s: expected a bool / uint8 occupancy grid or a float32 / float16 distance field, got %s' % (what, t.dtype))
    if kind == OCC_GRID:
        if threshold is not None:
            raise ValueError('%s: a threshold applies to distance fields, not to a %s occupancy grid' % (what, t.dtype))
        return t.contiguous(), kind, 0.0
    if threshold is None:
        raise ValueError('%s: a %s distance field needs a threshold (occupied = df <= threshold)' % (what, t.dtype))
    # `df <= threshold` in torch compares with the Python scalar cast to df's dtype; a CPU 0-dim tensor does the same cast without a device sync
    return t.contiguous(), kind, float(torch.tensor(float(threshold), dtype=t.dtype))


def _stats(p, pk, pt, t, tk, tt, chamfer):
    B, _, D, H, W = (int(s) for s in p.shape)
    out = torch.empty((B, 5), dtype=torch.int64, device=p.device)
    if B == 0:
        return out
    lib = _lib.load()
    nbytes = max(int(lib.rf_occupancy_stats_ws_bytes(B, D, H, W, int(chamfer))), 1)      # 0 = unsupported edges: the launch says why
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    lib.rf_occupancy_stats(_p(p), pk, pt, _p(t), tk, tt, B, D, H, W, int(chamfer), _p(out), _p(ws), nbytes, _stream())
    return out


@_device_scoped
@torch.no_grad()
def occupancy_stats(pred, target, threshold=None, chamfer=True):
    """pred, target: [B, 1, D, H, W] on the GPU, both bool / uint8 occupancy (non-zero = occupied) or both float32 / float16 distance fields with
    ``threshold`` (occupied iff df <= threshold, threshold rounded to the dtype first; NaN unoccupied).  Edges 1..2048.
    -> int64 [B, 5] device tensor, per volume n_pred, n_target, n_inter, s_tp = sum_{t in T} min_{p in P} |t - p|^2, s_pt = sum_{p in P}
    min_{t in T} |p - t|^2 (squared voxel-index units, exact; both 0 when either set is empty or chamfer is False).  Current stream, no sync."""
    p, pk, pt = _operand(pred, threshold, 'occupancy_stats: pred')
    t, tk, tt = _operand(target, threshold, 'occupancy_stats: target')
    if pred.dtype != target.dtype:
        raise ValueError('occupancy_stats: pred is %s, target is %s' % (pred.dtype, target.dtype))
    if pred.device != target.device:
        raise ValueError('occupancy_stats: pred on %s, target on %s' % (pred.device, target.device))
    if p.dim() != 5 or p.shape[1] != 1 or p.shape != t.shape:
        raise ValueError('occupancy_stats: expected two [B, 1, D, H, W] volumes of one shape, got %s and %s' % (tuple(p.shape), tuple(t.shape)))
    return _stats(p, pk, pt, t, tk, tt, chamfer)


class _Metric(torch.nn.Module):
    """torchmetrics.Metric's surface as the reference uses it: update / forward / compute / reset, sum-reduced float32 states."""
    _sum = None
    _chamfer = False

    def __init__(self, compute_on_step=True, dist_sync_on_step=False, process_group=None, dist_sync_fn=None):
        super().__init__()
        self.compute_on_step = compute_on_step
        self.dist_sync_on_step = dist_sync_on_step
        self.process_group = process_group
        for name in self._state_names():
            setattr(self, name, torch.zeros((), dtype=torch.float32))        # a plain attribute, not a buffer (module docstring)

    def _state_names(self):
        return (self._sum, 'total')

    def _apply(self, fn, *args, **kwargs):
        this = super()._apply(fn, *args, **kwargs)
        for name in self._state_names():
            setattr(this, name, fn(getattr(this, name)))
        return this

    def _increments(self, stats):
        raise NotImplementedError

    def _add(self, inc):
        for name in self._state_names():
            getattr(self, name).add_(inc[name])

    def _value(self, states):
        return states[self._sum].float() / states['total']

    def update(self, preds, target):
        self._add(self._increments(occupancy_stats(preds, target, chamfer=self._chamfer)))

    def forward(self, preds, target):
        inc = self._increments(occupancy_stats(preds, target, chamfer=self._chamfer))
        self._add(inc)
        if not self.compute_on_step:
            return None
        return self._value({name: torch.as_tensor(inc[name], dtype=torch.float32, device=getattr(self, name).device) for name in self._state_names()})

    def compute(self):
        states = {name: getattr(self, name) for name in self._state_names()}
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.process_group) > 1:
            flat = torch.stack([states[name] for name in self._state_names()])          # a copy: the local states stay unsynced
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.process_group)
            states = dict(zip(self._state_names(), flat))
        return self._value(states)

    def reset(self):
        for name in self._state_names():
            getattr(self, name).zero_()


class IoU(_Metric):
    """util/metrics.py:6-25: sum over volumes with a non-empty union of n_inter / (union + 1e-5); ``total`` counts them."""
    _sum = 'iou_sum'

    def _increments(self, stats):
        inter, union = stats[:, 2], stats[:, 0] + stats[:, 1] - stats[:, 2]
        valid = union > 0
        iou = inter / (union + 1e-5)
        return {'iou_sum': torch.where(valid, iou, torch.zeros_like(iou)).sum(), 'total': valid.sum()}


class Chamfer3D(_Metric):
    """util/metrics.py:28-55: per volume mean(dist1) + mean(dist2) with dist1 = squared distance of every target voxel to the nearest predicted one
    and dist2 the other way (each mean the exact quotient rounded once to float32, added in float32).  A volume with an empty set is skipped: in the
    reference its mean over an empty tensor is NaN and is dropped at :48-50.  ``total`` counts the volumes taken."""
    _sum = 'cd_sum'
    _chamfer = True

    def _increments(self, stats):
        n_p, n_t = stats[:, 0], stats[:, 1]
        valid = (n_p > 0) & (n_t > 0)
        cd = (stats[:, 3].double() / n_t.double()).float() + (stats[:, 4].double() / n_p.double()).float()
        return {'cd_sum': torch.where(valid, cd, torch.zeros_like(cd)).sum(), 'total': valid.sum()}


class Precision(_Metric):
    """util/metrics.py:58-72: sum over all volumes of n_inter / (n_pred + 1e-5)."""
    _sum = 'precision_sum'

    def _increments(self, stats):
        return {'precision_sum': (stats[:, 2] / (stats[:, 0] + 1e-5)).sum(), 'total': stats.shape[0]}


class Recall(_Metric):
    """util/metrics.py:75-89: sum over all volumes of n_inter / (n_target + 1e-5)."""
    _sum = 'recall_sum'

    def _increments(self, stats):
        return {'recall_sum': (stats[:, 2] / (stats[:, 1] + 1e-5)).sum(), 'total': stats.shape[0]}


def f1(precision, recall):
    """trainer/train_refinement.py:141"""
    return 2 * (precision * recall) / (precision + recall)


def _scene_operand(x, threshold, dev):
    x = torch.as_tensor(x).to(dev)
    if x.dtype not in (torch.float32, torch.float16):
        x = x <= threshold                   # other dtypes (float64 fields): the reference's own comparison, then the occupancy route
    return _operand(x[None, None], None if x.dtype == torch.bool else threshold, 'retrieval_metrics')


@torch.no_grad()
def retrieval_metrics(retrievals, dataset):
    """util/retrieval.py:167-175 get_metrics_for_retrieval: IoU, Chamfer, precision and recall of the nearest retrieval ``retrievals[i][0]`` of every
    scene of ``dataset.scenes`` against ``dataset.get_scene_target(scene)``, both occupied where df <= 0.75 * dataset.target_voxel_size.  Scenes
    may differ in size.  -> [iou, cd, precision, recall] as Python floats (computed on the current GPU)."""
    dev = torch.device('cuda', torch.cuda.current_device())
    metrics = [m.to(dev) for m in (IoU(compute_on_step=False), Chamfer3D(compute_on_step=False), Precision(compute_on_step=False),
                                   Recall(compute_on_step=False))]
    thr = 0.75 * dataset.target_voxel_size
    for idx, scene in enumerate(dataset.scenes):
        p, pk, pt = _scene_operand(retrievals[idx][0], thr, dev)
        t, tk, tt = _scene_operand(dataset.get_scene_target(scene), thr, dev)
        if p.shape != t.shape:
            raise ValueError('retrieval_metrics: scene %s: retrieval %s, target %s' % (scene, tuple(p.shape[2:]), tuple(t.shape[2:])))
        stats = _stats(p, pk, pt, t, tk, tt, True)
        for m in metrics:
            m._add(m._increments(stats))
    return [m.compute().cpu().item() for m in metrics]
