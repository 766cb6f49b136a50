"""The shape loss of the reference's refinement trainer on the device: ``RefinementTrainingModule.augment_batch_data`` / ``loss_shape`` /
``adjust_weights`` (trainer/train_refinement.py:175-183, :231-253), ``PatchedSceneDataset.compute_normals`` (dataset/patched_scene_dataset.py:139-146)
and ``get_cosine_similarity`` (model/loss.py:78-85), in csrc/shape_loss.hip behind include/rfuse_train.h.  NO CPU fallback.

    sl = ShapeLoss(target_trunc, target_mean, target_std, weight_occupied=8, loss_reconstruction=1, loss_normal=0.5)   # or ShapeLoss.from_config(cfg)
    sl.augment_batch_data(batch)                     # adds batch['weights'], batch['empty'] (bool), batch['normals']     -- one launch
    total, l1, normal = sl.loss_shape(pred, batch)   # differentiable with respect to pred only                           -- two launches, one more backward
    sl.compute_normals(v)                            # forward only

The reference evaluates this as ~40 elementwise / pad / conv3d / cat / boolean-index / reduction launches plus their autograd mirror, and the boolean
index waits for the host to learn the number of valid voxels.  Here nothing synchronises: the scalars and the count stay on the device, and two calls on
the same input return the same bits (float64 partial sums combined in a fixed order, no atomics).

What differs from the reference's float32 evaluation is rounding only: the 27 Sobel taps are accumulated exactly and rounded once (a flat neighbourhood
gives a gradient of exactly 0, on which the valid mask ``|n| != 0`` rests, independent of any summation order), the sums of the two means are float64, and
the gradient is the analytic ``d cos / d g = (t^ - g^ (g^ . t^)) / |g|`` evaluated in float64 instead of autograd through three normalisations.
"""
import torch

from . import _lib
from . import configs as _configs
from .ops import _p, _stream, _device_scoped


def _f32(x):
    """a Python / numpy scalar as the float32 value torch gives it beside a float32 tensor (no device involved)"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _volume(t, what, dtype=torch.float32, channels=1):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor' % what)
    if not t.is_cuda:
        raise RuntimeError('%s: the shape loss runs on the GPU only (got a %s tensor); there is no CPU fallback' % (what, t.device))
    if t.dim() != 5 or t.shape[1] != channels:
        raise ValueError('%s: expected a [B, %d, D, H, W] tensor, got %s' % (what, channels, tuple(t.shape)))
    if t.dtype != dtype:
        raise TypeError('%s: expected %s, got %s' % (what, dtype, t.dtype))
    if t.numel() == 0:
        raise ValueError('%s: an empty tensor %s' % (what, tuple(t.shape)))
    return t.contiguous()


@_device_scoped
@torch.no_grad()
def _sobel_normals(v, scale, shift, pad, thr=0.0, w_occ_minus_1=0.0, augment=False):
    n, _, d, h, w = v.shape
    normals = torch.empty((n, 3, d, h, w), dtype=torch.float32, device=v.device)
    weights = torch.empty_like(v) if augment else None
    empty = torch.empty(v.shape, dtype=torch.bool, device=v.device) if augment else None
    _lib.load_train().rf_train_sobel_normals(_p(v), n, d, h, w, scale, shift, pad, thr, w_occ_minus_1, _p(normals), _p(weights), _p(empty), _stream())
    return normals, weights, empty


@_device_scoped
def _forward(pred, target, weights, empty, normals, trunc, mean, std, lam_rec, lam_n, need_grad):
    n, _, d, h, w = pred.shape
    lib = _lib.load_train()
    dev = pred.device
    nbytes = int(lib.rf_train_shape_loss_ws_bytes(n, d, h, w))
    if nbytes == 0:
        raise ValueError('loss_shape: %s is outside the supported range (at most 2^31 - 1 voxels per volume and 8 x 8 x 32 tiles per batch)' % (tuple(pred.shape),))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    grad_l1 = torch.empty_like(pred) if need_grad else None
    grad_g = torch.empty((n, 3, d, h, w), dtype=torch.float32, device=dev) if need_grad else None
    lib.rf_train_shape_loss(_p(pred), _p(target), _p(weights), _p(empty), _p(normals), n, d, h, w, trunc, mean, std, lam_rec, lam_n, _p(out), _p(counts),
                            _p(grad_l1), _p(grad_g), _p(ws), nbytes, _stream())
    return out, counts, grad_l1, grad_g


@_device_scoped
def _backward(grad_l1, grad_g, coef, counts, shape, trunc):
    n, _, d, h, w = shape
    dpred = torch.empty(shape, dtype=torch.float32, device=coef.device)
    _lib.load_train().rf_train_shape_loss_backward(_p(grad_l1), _p(grad_g), _p(coef), _p(counts), n, d, h, w, trunc, _p(dpred), _stream())
    return dpred


class _ShapeLossFn(torch.autograd.Function):
    """(pred; target, weights, empty, normals, constants) -> (float32 [3] = total, l1, normal; counts); the gradient goes to pred only"""

    @staticmethod
    def forward(ctx, pred, target, weights, empty, normals, trunc, mean, std, lam_rec, lam_n):
        need_grad = ctx.needs_input_grad[0]
        out, counts, grad_l1, grad_g = _forward(pred, target, weights, empty, normals, trunc, mean, std, lam_rec, lam_n, need_grad)
        if need_grad:
            ctx.save_for_backward(grad_l1, grad_g, counts)
        ctx.consts = (tuple(pred.shape), trunc, lam_rec, lam_n)
        ctx.mark_non_differentiable(counts)
        return out, counts

    @staticmethod
    def backward(ctx, g_out, _g_counts):
        grad_l1, grad_g, counts = ctx.saved_tensors
        shape, trunc, lam_rec, lam_n = ctx.consts
        # a = g_total * lambda_rec + g_l1, b = g_total * lambda_n + g_normal; a term that was not evaluated is the constant zeros(1): nothing flows through it
        coef = torch.stack((g_out[0] * lam_rec + g_out[1], g_out[0] * lam_n + g_out[2]))
        dpred = _backward(grad_l1 if lam_rec > 0 else None, grad_g if lam_n > 0 else None, coef, counts, shape, trunc)
        return (dpred,) + (None,) * 9


class ShapeLoss:
    """The three methods of the reference's trainer that make up its shape loss, one call each (see the module docstring)."""

    def __init__(self, target_trunc, target_mean, target_std, weight_occupied=8, loss_reconstruction=1, loss_normal=0.5):
        self.target_trunc, self.target_mean, self.target_std = float(target_trunc), float(target_mean), float(target_std)
        self.weight_occupied, self.loss_reconstruction, self.loss_normal = weight_occupied, loss_reconstruction, loss_normal
        self.last_counts = None      # int64 [2] on the device, of the latest loss_shape: valid voxels, voxels empty in target and prediction

    @classmethod
    def from_config(cls, config, **hparams):
        """``config``: an rfuse.configs dictionary (dataset_train carries voxel_size_target, target_mean, target_std); ``hparams``: weight_occupied,
        loss_reconstruction, loss_normal where they differ from the reference's base configs (8, 1, 0.5)."""
        d = config['dataset_train']
        return cls(_configs.truncations(config)[1], d['target_mean'], d['target_std'], **hparams)

    def compute_normals(self, v):
        """PatchedSceneDataset.compute_normals: [B,1,D,H,W] -> [B,3,D,H,W], the Sobel gradient of v padded with target_trunc, over sqrt(|g|^2 + 1e-5)."""
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise RuntimeError('compute_normals is forward only (v requires grad); loss_shape differentiates the normals of its prediction itself')
        return _sobel_normals(_volume(v, 'compute_normals: v'), 1.0, 0.0, _f32(self.target_trunc))[0]

    def augment_batch_data(self, batch):
        """trainer :231-237: batch['normals'] = the normals of the denormalised target, batch['weights'] = weight_occupied where the (normalised)
        target is below target_trunc and 1 elsewhere, batch['empty'] = target >= target_trunc (bool).  One launch."""
        t = _volume(batch['target'].detach() if isinstance(batch['target'], torch.Tensor) else batch['target'], "augment_batch_data: batch['target']")
        trunc = _f32(self.target_trunc)
        normals, weights, empty = _sobel_normals(t, _f32(self.target_std), _f32(self.target_mean), trunc, trunc, _f32(self.weight_occupied - 1), augment=True)
        batch['weights'], batch['empty'], batch['normals'] = weights, empty, normals

    def loss_shape(self, pred_shape, batch):
        """trainer :175-183: (total_loss, loss_l1, loss_normal) of a prediction in [-1, 1] against the augmented batch.  Scalars of shape () on the
        device; a term whose hyper-parameter is <= 0 is reported as zeros(1) (and total then has shape (1,)), as in the reference."""
        pred = _volume(pred_shape, 'loss_shape: pred_shape')
        target = _volume(batch['target'].detach(), "loss_shape: batch['target']")
        weights = _volume(batch['weights'].detach(), "loss_shape: batch['weights']")
        empty = _volume(batch['empty'], "loss_shape: batch['empty']", torch.bool)
        normals = _volume(batch['normals'].detach(), "loss_shape: batch['normals']", channels=3)
        for name, t in (('target', target), ('weights', weights), ('empty', empty)):
            if t.shape != pred.shape:
                raise ValueError("loss_shape: batch['%s'] is %s, pred_shape %s" % (name, tuple(t.shape), tuple(pred.shape)))
        if normals.shape[0] != pred.shape[0] or normals.shape[2:] != pred.shape[2:]:
            raise ValueError("loss_shape: batch['normals'] is %s, pred_shape %s" % (tuple(normals.shape), tuple(pred.shape)))
        out, counts = _ShapeLossFn.apply(pred, target, weights, empty, normals, _f32(self.target_trunc), _f32(self.target_mean), _f32(self.target_std),
                                         _f32(self.loss_reconstruction), _f32(self.loss_normal))
        total, l1, normal = out.unbind(0)
        self.last_counts = counts
        if not self.loss_reconstruction > 0:
            l1, total = l1.detach().reshape(1), total.reshape(1)
        if not self.loss_normal > 0:
            normal, total = normal.detach().reshape(1), total.reshape(1)
        return total, l1, normal
