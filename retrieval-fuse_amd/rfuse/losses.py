"""The losses of the reference's refinement trainer on the device.  First the shape loss: ``RefinementTrainingModule.augment_batch_data`` / ``loss_shape`` /
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

Then the contrastive term (csrc/ntxent.hip behind include/rfuse_contrastive.h), also without a CPU fallback:

    ntx = NTXent(temperature, use_cosine_similarity=True, sig_scale=80, sig_shift=-65)      # model/loss.py NTXentLoss, one group
    loss = ntx(zis, zjs, iou_matrix=None)                                                    # () float32
    acl = AttnContrastiveLoss(temperature=0.05, max_rows=1280)                               # trainer :208-221 compute_sliced_attn_nt_xent_loss
    loss = acl(num_slices, x_attn_fpred, x_attn_ftgt, occupancy_attn)                        # (1,) float32; acl.last_counts int64 [3] on the device

The reference's sliced loss asks the host twice per slice whether and how many rows are occupied, boolean-indexes them and runs NTXentLoss on each slice in
turn.  Here the selection is made on the device (the same greedy rule in slice order), the similarity matrix is never materialised, and nothing waits for the
host: four launches forward, one backward.  The arithmetic is float64 from the float32 features on, the sums have one order: the same bits on every call.

And the producer of that IoU matrix with the rest of the retrieval trainer's step (csrc/iou_matrix.hip behind include/rfuse_pairs.h), without a CPU fallback:

    m = iou_matrix(occupancy)                                                                # util/misc.py get_iou_matrix: bool / uint8 [n,1,D,H,W] -> [n, n]
    m = target_iou_matrix(batch['target'], target_mean, target_std, 0.75 * voxel_size)       # trainer/train_retrieval.py:85 with its .repeat(2, 2): [2B, 2B]
    step = RetrievalStepLoss.from_config(cfg, temperature=0.2)                               # trainer/train_retrieval.py:77-88
    total_loss, loss_contrastive = step(features_in, features_tgt, batch['target'], train=True)

The reference materialises four [n^2, D, H, W] bool tensors; here a window becomes one bit per voxel and a pair one AND + popcount per 64 voxels.  The counts
are integers and the four float32 operations after them are the reference's: the matrix has the reference's bits.
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


# ------------------------------------------------------------------------------------------------ the contrastive loss
_NTX_SLICES, _NTX_GROUP, _NTX_DIM = 4096, 4096, 256      # the supported range of include/rfuse_contrastive.h


def _features(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor' % what)
    if not t.is_cuda:
        raise RuntimeError('%s: the contrastive loss runs on the GPU only (got a %s tensor); there is no CPU fallback' % (what, t.device))
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError('%s: expected a non-empty [rows, features] tensor, got %s' % (what, tuple(t.shape)))
    if t.dtype != torch.float32:
        raise TypeError('%s: expected torch.float32, got %s' % (what, t.dtype))
    return t.contiguous()


@_device_scoped
def _ntx_forward(zis, zjs, occ, iou, num_slices, max_rows, cosine, tau, sig_scale, sig_shift):
    n_rows, dim = zis.shape
    lib = _lib.load_contrastive()
    dev = zis.device
    nbytes = int(lib.rf_ntx_ws_bytes(n_rows, num_slices, max_rows, dim))
    if nbytes == 0:
        raise ValueError('contrastive loss: %d rows of %d features in %d slices, at most %d rows, is outside the supported range (1 <= features <= %d, '
                         'slices <= %d, 1 <= min(rows // slices, max_rows) <= %d)' % (n_rows, dim, num_slices, max_rows, _NTX_DIM, _NTX_SLICES, _NTX_GROUP))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    lib.rf_ntx_plan(_p(occ), n_rows, num_slices, max_rows, dim, _p(ws), nbytes, _p(counts), _stream())
    lib.rf_ntx_forward(_p(zis), _p(zjs), _p(iou), n_rows, num_slices, max_rows, dim, cosine, tau, sig_scale, sig_shift, _p(ws), nbytes, _p(loss), _stream())
    return loss, counts, ws


@_device_scoped
def _ntx_backward(g, iou, ws, shape, num_slices, max_rows, cosine, tau, sig_scale, sig_shift):
    n_rows, dim = shape
    dzis = torch.empty(shape, dtype=torch.float32, device=g.device)
    dzjs = torch.empty(shape, dtype=torch.float32, device=g.device)
    _lib.load_contrastive().rf_ntx_backward(_p(iou), _p(g), n_rows, num_slices, max_rows, dim, cosine, tau, sig_scale, sig_shift, _p(ws), ws.numel(), _p(dzis),
                                            _p(dzjs), _stream())
    return dzis, dzjs


class _NTXentFn(torch.autograd.Function):
    """(zis, zjs; occupancy, iou, constants) -> (float32 [1], counts); the gradient goes to the two feature tensors only"""

    @staticmethod
    def forward(ctx, zis, zjs, occ, iou, num_slices, max_rows, cosine, tau, sig_scale, sig_shift):
        loss, counts, ws = _ntx_forward(zis, zjs, occ, iou, num_slices, max_rows, cosine, tau, sig_scale, sig_shift)
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(ws, iou) if iou is not None else ctx.save_for_backward(ws)
        ctx.consts = (tuple(zis.shape), num_slices, max_rows, cosine, tau, sig_scale, sig_shift)
        ctx.mark_non_differentiable(counts)
        return loss, counts

    @staticmethod
    def backward(ctx, g_loss, _g_counts):
        ws, iou = (tuple(ctx.saved_tensors) + (None,))[:2]
        dzis, dzjs = _ntx_backward(g_loss.to(torch.float32).contiguous(), iou, ws, *ctx.consts)
        return (dzis, dzjs) + (None,) * 8


class NTXent:
    """One ``model.loss.NTXentLoss`` call on the device: ``zis``, ``zjs`` float32 [B, dim] (1 <= B <= 4096, dim <= 256), optionally the [2B, 2B] IoU matrix of
    the retrieval trainer's ``iou_scaling`` (rows and columns in the order [zjs; zis]).  Returns the scalar () float32."""

    def __init__(self, temperature, use_cosine_similarity=True, sig_scale=80, sig_shift=-65):
        self.temperature, self.use_cosine_similarity, self.sig_scale, self.sig_shift = temperature, bool(use_cosine_similarity), sig_scale, sig_shift

    def __call__(self, zis, zjs, iou_matrix=None):
        zis, zjs = _features(zis, 'NTXent: zis'), _features(zjs, 'NTXent: zjs')
        if zis.shape != zjs.shape:
            raise ValueError('NTXent: zis is %s, zjs %s' % (tuple(zis.shape), tuple(zjs.shape)))
        b = zis.shape[0]
        if iou_matrix is not None:
            iou_matrix = _features(iou_matrix.detach(), 'NTXent: iou_matrix')
            if iou_matrix.shape != (2 * b, 2 * b):
                raise ValueError('NTXent: iou_matrix is %s, expected %s' % (tuple(iou_matrix.shape), (2 * b, 2 * b)))
        loss, _ = _NTXentFn.apply(zis, zjs, None, iou_matrix, 1, b, int(self.use_cosine_similarity), _f32(self.temperature), _f32(self.sig_scale),
                                  _f32(self.sig_shift))
        return loss.reshape(())


class AttnContrastiveLoss:
    """``RefinementTrainingModule.compute_sliced_attn_nt_xent_loss`` (trainer :208-221) with its ``NTXentLoss(temperature, True)``: the rows of the two feature
    tensors [N, dim] in ``num_slices`` slices of N // num_slices rows, the rows with ``occupancy_attn > 0`` of a slice one NT-Xent group, slices taken in order
    while the selected rows stay within ``max_rows``; the sum of the groups' losses, shape (1,).  ``last_counts``: int64 [3] on the device = occupied rows over
    all slices (the trainer's ``attn_occupancy``), selected rows, selected groups.  Nothing waits for the host."""

    def __init__(self, temperature=0.05, max_rows=1280):
        self.temperature, self.max_rows = temperature, int(max_rows)
        self.last_counts = None

    def __call__(self, num_slices, x_attn_fpred, x_attn_ftgt, occupancy_attn):
        zis, zjs = _features(x_attn_fpred, 'AttnContrastiveLoss: x_attn_fpred'), _features(x_attn_ftgt, 'AttnContrastiveLoss: x_attn_ftgt')
        if zis.shape != zjs.shape:
            raise ValueError('AttnContrastiveLoss: x_attn_fpred is %s, x_attn_ftgt %s' % (tuple(zis.shape), tuple(zjs.shape)))
        if not isinstance(occupancy_attn, torch.Tensor) or not occupancy_attn.is_cuda:
            raise RuntimeError('AttnContrastiveLoss: occupancy_attn must be a GPU tensor; there is no CPU fallback')
        if occupancy_attn.numel() != zis.shape[0]:
            raise ValueError('AttnContrastiveLoss: occupancy_attn has %d entries for %d rows' % (occupancy_attn.numel(), zis.shape[0]))
        occ = (occupancy_attn.detach().reshape(-1) > 0).contiguous()          # bool: one byte per row, 0 / 1
        loss, counts = _NTXentFn.apply(zis, zjs, occ, None, int(num_slices), self.max_rows, 1, _f32(self.temperature), 0.0, 0.0)
        self.last_counts = counts
        return loss


# ------------------------------------------------------------------------------------------------ the retrieval trainer's IoU matrix and step
_IOU_MAX_N, _IOU_MAX_VOXELS = 8192, 1 << 24      # the supported range of include/rfuse_pairs.h


def _windows(t, what, dtypes):
    """what a tensor says about itself, before the question where it lives"""
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s: expected a torch.Tensor' % what)
    if t.dim() != 5 or t.shape[1] != 1 or t.numel() == 0:
        raise ValueError('%s: expected a non-empty [n, 1, D, H, W] tensor, got %s' % (what, tuple(t.shape)))
    if t.dtype not in dtypes:
        raise TypeError('%s: expected %s, got %s' % (what, ' or '.join(str(d) for d in dtypes), t.dtype))
    return t.detach()


def _on_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError('%s: the IoU matrix is built on the GPU only (got a %s tensor); there is no CPU fallback' % (what, t.device))
    return t.contiguous()


def _pack(x, kind, scale, shift, thr, other_n):
    """one launch: (bits int64 [n, ceil(voxels / 64)], counts int32 [n]) of the windows ``x``"""
    n, voxels = x.shape[0], x[0].numel()
    lib = _lib.load_pairs()
    if int(lib.rf_iou_ws_bytes(n, other_n, voxels)) == 0:
        raise ValueError('iou_matrix: %d x %d samples of %d voxels is outside the supported range (1 <= samples <= %d, voxels <= %d)'
                         % (n, other_n, voxels, _IOU_MAX_N, _IOU_MAX_VOXELS))
    bits = torch.empty((n, (voxels + 63) // 64), dtype=torch.int64, device=x.device)
    counts = torch.empty(n, dtype=torch.int32, device=x.device)
    lib.rf_iou_pack(_p(x), kind, scale, shift, thr, n, voxels, _p(bits), _p(counts), _stream())
    return bits, counts, voxels


def _pairs(a, b, voxels, repeat):
    if repeat not in (1, 2):
        raise ValueError('iou_matrix: repeat is 1 or 2, got %r' % (repeat,))
    (bits_a, counts_a), (bits_b, counts_b) = a, (b if b is not None else (None, None))
    n_a, n_b = counts_a.numel(), counts_a.numel() if b is None else counts_b.numel()
    out = torch.empty((repeat * n_a, repeat * n_b), dtype=torch.float32, device=bits_a.device)
    _lib.load_pairs().rf_iou_matrix(_p(bits_a), _p(counts_a), n_a, _p(bits_b), _p(counts_b), n_b, voxels, repeat, _p(out), _stream())
    return out


@_device_scoped
@torch.no_grad()
def iou_matrix(batch_shapes, other=None, repeat=1):
    """``util.misc.get_iou_matrix`` (util/misc.py:51-59) on the device: ``batch_shapes`` bool / uint8 [n, 1, D, H, W], non-zero = occupied; float32 [n, n] =
    intersection / (union + 1e-5) of every pair of windows, the reference's bits.  With ``other`` ([m, 1, D, H, W], the same window) the [n, m] matrix of
    the two sets; ``repeat=2`` returns what ``.repeat(2, 2)`` would.  Two launches (three with ``other``) on the current stream, nothing waits for the host,
    and no [n^2, D, H, W] tensor exists."""
    a = _windows(batch_shapes, 'iou_matrix: batch_shapes', (torch.bool, torch.uint8))
    if other is None:
        bits, counts, voxels = _pack(_on_gpu(a, 'iou_matrix: batch_shapes'), 0, 0.0, 0.0, 0.0, a.shape[0])
        return _pairs((bits, counts), None, voxels, repeat)
    b = _windows(other, 'iou_matrix: other', (torch.bool, torch.uint8))
    if b.shape[2:] != a.shape[2:]:
        raise ValueError('iou_matrix: other has windows of %s, batch_shapes of %s' % (tuple(b.shape[2:]), tuple(a.shape[2:])))
    bits_a, counts_a, voxels = _pack(_on_gpu(a, 'iou_matrix: batch_shapes'), 0, 0.0, 0.0, 0.0, b.shape[0])
    bits_b, counts_b, _ = _pack(_on_gpu(b, 'iou_matrix: other'), 0, 0.0, 0.0, 0.0, a.shape[0])
    return _pairs((bits_a, counts_a), (bits_b, counts_b), voxels, repeat)


@_device_scoped
@torch.no_grad()
def target_iou_matrix(target, target_mean, target_std, threshold, repeat=2):
    """The trainer's ``get_iou_matrix(denormalize_target(batch['target']) <= threshold).repeat(2, 2)`` (trainer/train_retrieval.py:85) from the normalised
    float32 targets [B, 1, D, H, W]: a voxel is occupied iff ``target * target_std + target_mean <= threshold`` in float32, operation by operation.
    ``repeat=2``: the [2B, 2B] matrix that ``NTXent`` takes, written once."""
    t = _on_gpu(_windows(target, 'target_iou_matrix: target', (torch.float32,)), 'target_iou_matrix: target')
    bits, counts, voxels = _pack(t, 1, _f32(target_std), _f32(target_mean), _f32(threshold), t.shape[0])
    return _pairs((bits, counts), None, voxels, repeat)


class RetrievalStepLoss:
    """The tail of ``RetrievalTrainingModule.step`` (trainer/train_retrieval.py:77-88): the two encoders' feature volumes through ``reshape_features``
    (permute / reshape and F.normalize, in torch and differentiable), the code noise of a training step, the IoU matrix of the batch's targets when
    ``iou_scaling`` is set, and ``NTXent(temperature, True)``.  Returns ``(total_loss, loss_contrastive)``; gradients flow to the two feature tensors only."""

    def __init__(self, temperature, target_mean, target_std, voxel_size_target, iou_scaling=True, contrastive_weight=1.0, code_noise=0.0):
        self.temperature, self.target_mean, self.target_std = temperature, float(target_mean), float(target_std)
        self.threshold = 0.75 * voxel_size_target
        self.iou_scaling, self.contrastive_weight, self.code_noise = bool(iou_scaling), contrastive_weight, code_noise
        self.ntxent = NTXent(temperature, True)

    @classmethod
    def from_config(cls, config, **retrieval_training):
        """``config``: an rfuse.configs dictionary or the reference's own (dataset_train carries target_mean, target_std and the raw voxel_size_target);
        ``retrieval_training``: the constructor's keywords, or the reference's ``retrieval_training`` section as it stands (``temprature``, ``iou_scaling``,
        ``loss: {contrastive: w}``, ``code_noise``; its other keys belong to the optimiser and the loader)."""
        d, rt = config['dataset_train'], dict(retrieval_training)
        if 'temprature' in rt:
            rt['temperature'] = rt.pop('temprature')
        if 'loss' in rt:
            rt['contrastive_weight'] = rt.pop('loss')['contrastive']
        if 'temperature' not in rt:
            raise TypeError('RetrievalStepLoss.from_config: the temperature is missing')
        keep = {k: rt[k] for k in ('iou_scaling', 'contrastive_weight', 'code_noise') if k in rt}
        return cls(rt['temperature'], d['target_mean'], d['target_std'], d['voxel_size_target'], **keep)

    @staticmethod
    def reshape_features(feats):
        feature_dim = feats.shape[1]
        return torch.nn.functional.normalize(feats.permute((0, 2, 3, 4, 1)).reshape((-1, feature_dim)), dim=1)

    def __call__(self, features_in, features_tgt, target, train=False):
        for t, what in ((features_in, 'features_in'), (features_tgt, 'features_tgt')):
            if not isinstance(t, torch.Tensor):
                raise TypeError('RetrievalStepLoss: %s: expected a torch.Tensor' % what)
            if t.dim() != 5:
                raise ValueError('RetrievalStepLoss: %s: expected a [B, dim, d, h, w] tensor, got %s' % (what, tuple(t.shape)))
            if not t.is_cuda:
                raise RuntimeError('RetrievalStepLoss: %s: the step loss runs on the GPU only (got a %s tensor); there is no CPU fallback' % (what, t.device))
        if not self.contrastive_weight > 0:              # the reference's zeros(1), times the weight
            zero = torch.zeros(1, dtype=torch.float32, device=features_in.device)
            return zero * self.contrastive_weight, zero
        zis, zjs = self.reshape_features(features_in), self.reshape_features(features_tgt)
        if train and self.code_noise > 0:
            zis = zis + torch.empty_like(zis).normal_(mean=0, std=self.code_noise)
            zjs = zjs + torch.empty_like(zjs).normal_(mean=0, std=self.code_noise)
        iou = target_iou_matrix(target, self.target_mean, self.target_std, self.threshold, repeat=2) if self.iou_scaling else None
        loss_contrastive = self.ntxent(zis, zjs, iou)
        return loss_contrastive * self.contrastive_weight, loss_contrastive
