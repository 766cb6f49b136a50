"""Training slice: ``torch.autograd.Function``s whose forward AND backward run the HIP kernels.

The reference trains THROUGH the drop-in modules (trainer/train_refinement.py:41-43 optimisers over unet_backbone / decoder /
retrieval_backbone / attention parameters, :295-306 phase hand-over).  Built here:

  ConvGnRelu   y = ReLU(conv3(GroupNorm(x)))   one SingleConv 'gcr' layer (reference model/unet.py:19-76) -- 97 % of the FLOPs
      forward   rf_gn_stats / rf_gn_from_stats + the inference kernels, chosen by routes.single in its order for a written-out concatenation (split-operand F16 forms where
                the parameters are inside their range: one batched range check per optimiser step)
      backward  rf_relu_backward[_amax] -> d xn = conv3(dz, W^T with flipped taps), no ReLU: rf_conv3d_split_k3_gn on dz scaled by a power of two
                into the f16 pairs' range (rf_dgrad_scale_affine; the scale leaves again in the GroupNorm backward), else rf_conv3d_k3_gn (fp32 MFMA)
                rf_conv3d_k3_wgrad_split (F16 matrix cores, split operands; edge >= 8 boxes and whole 4^3 samples) / rf_conv3d_k3_wgrad (fp32 MFMA)
                rf_gn_backward (three passes, every tensor read once per pass)                  = dx, dgamma, dbeta
                2^3 / 1^3 volumes: weight gradient as a split-K MFMA GEMM (rf_linear_wgrad) on the unfolded input, float64 slice sum
  Linear       y = act(x W^T + b)               the layers of AttentionFeatureEncoder (reference model/attention.py:29-46)
      backward  dx = rf_linear(dpre, W^T-as-weight),  dW = rf_linear_wgrad(dpre, x) in row chunks summed in float64
  MaxPool3d(2) / nearest x2 upsample             rf_maxpool3d_2 + rf_maxpool3d_2_backward, rf_upsample3d_2 + rf_sumpool3d_2 (bit-equal to torch's)
  ConvValidLeaky  y = LeakyReLU(conv_valid(x, W, stride) + b)   one layer of the conv patch encoders (reference model/retrieval.py:4-361), trained
                with NT-Xent by trainer/train_retrieval.py
      forward   the inference kernels, chosen per layer by routes.valid (through model/retrieval.py:_ConvPatchEncoder._conv), with an fp32 output (no split
                hand-over between layers in grad mode)
      backward  rf_conv3d_valid_leaky_backward (dz from the saved output, db in float64) -> rf_conv3d_valid_dgrad (fp32 MFMA per parity phase; skipped
                when x needs no gradient: the first layer's input is data) and rf_conv3d_valid_wgrad (fp32 MFMA, split K, float64 slice sum).  fp32
                operands throughout, so NT-Xent's small gradients (1e-3 ... 1e-7) need no rescaling.
                The MLP patch encoders (Patch04 / Patch05 / Patch04V2) and every encoder's final_layer run through Linear below.

  AttnFuse     the patch attention after its encoders (reference model/attention.py:92-110): normalise, K scores, switch, softmax | Gumbel-hard, mix, blend
      forward   rf_attn_fuse (the inference kernel; only its inputs are saved)
      backward  rf_attn_fuse_backward: one launch for dx, dp and the gradients of the RAW encoder outputs; the row's decisions are recomputed with the
                forward's code; the switch's gradient goes to the first maximal score like MaxPool1d(K); Gumbel-hard as torch's straight-through form
  PointwiseTanh   y = tanh(conv1x1(x, W) + b)   the final decoder's head (reference model/refinement.py:54-55)
      forward   rf_conv1x1_tanh (the inference kernel: the same bits as the plain inference route)
      backward  rf_pointwise_tanh_backward (include/rfuse_step.h): dx, dW, db from the saved output in one pass over x, float64 sums in a fixed order
  Unfold3d / Fold3d / GatherRetrieved   rf_unfold3d <-> rf_fold3d, rf_attn_gather_retrieved -> rf_attn_scatter_retrieved (pure index maps, same bits as
                the permuted views they replace)

torch does the bookkeeping and the light per-row work: transposes / flips of weights, the activation mask of Linear, sums over the batch of
per-sample float64 pieces and the Gumbel noise draw -- together < 1 % of the FLOPs.  With
that the whole training graph of the reference (trainer/train_refinement.py:108-116 forward_full, all four networks trainable = phase 3) runs
through the drop-in modules in grad mode; loss and every parameter gradient are checked against float64 autograd of the oracle in
tests/test_autograd_gpu.py.  Not built: backward of the pre-split pair routes and the fused attention MLP (grad mode takes the plain routes), the
BatchNorm patch encoders (PatchNorm08 / PatchNorm32: no shipped config selects them) and the patch encoders' forward_grid (the database build and
the queries never train).

What follows the backward -- the parameter update -- is HIP too: ``rfuse.optim.Adam`` (rfuse/optim.py over csrc/optim.hip, declared in a ninth header,
include/rfuse_optim.h) is torch.optim.Adam's update in one pass over all parameters; it bumps the parameters' version counters like torch's in-place
update, so the images and range decisions the layers above derive from their weights follow it.
"""
import torch
import torch.nn.functional as F

from . import _lib, ops, routes

_p, _stream, _ws = ops._p, ops._stream, ops._workspace         # (the helpers below launch on the device of their tensors: ops._device_scoped)


@ops._device_scoped
def relu_backward(dy, y):
    out = torch.empty_like(y)
    _lib.load().rf_relu_backward(_p(dy), _p(y), y.numel(), _p(out), _stream())
    return out


@ops._device_scoped
def relu_backward_amax(dy, y):
    """relu_backward and max |result| (per-workgroup maxima on the device) beside it"""
    out = torch.empty_like(y)
    lib = _lib.load()
    amax = torch.empty(lib.rf_relu_backward_amax_slots(), dtype=torch.float32, device=y.device)       # per-workgroup maxima, reduced by the consumer
    lib.rf_relu_backward_amax(_p(dy), _p(y), y.numel(), _p(out), _p(amax), _stream())
    return out, amax


@ops._device_scoped
def dz_scale(amax, n, cout):
    """from the maxima of relu_backward_amax: s = the power of two that puts max |dz| into [512, 1024) (the split forms carry values as f16 pairs: a
    gradient has to be brought into their range first; a power of two is exact), decided and applied on the device.  Returns the identity GroupNorm
    affine with scale s for [n][cout] and the device pair (s, 1 / s)."""
    ident = torch.empty((n, cout, 4), dtype=torch.float32, device=amax.device)
    scales = torch.empty(2, dtype=torch.float32, device=amax.device)
    _lib.load().rf_dgrad_scale_affine(_p(amax), n * cout, _p(ident), _p(scales), _stream())
    return ident, scales


@ops._device_scoped
def dgrad_split(dz, ident, weight, cin):
    """d xn * s = conv3(dz * s, W^T with flipped taps) on the F16 matrix cores (csrc/conv3d_split.hip, split operands)"""
    n, cout, edge = dz.shape[0], dz.shape[1], dz.shape[2]
    wt = weight.flip(2, 3, 4).transpose(0, 1).contiguous()          # [cin, cout, 3,3,3]: the data-gradient conv's weight
    out = torch.empty((n, cin, edge, edge, edge), dtype=torch.float32, device=dz.device)
    _lib.load().rf_conv3d_split_k3_gn(_p(dz), cout, n, edge, _p(ident), _p(ops.pack_conv3_split_weight(wt)), cin, 0, _p(out), _stream())
    return out


@ops._device_scoped
def conv3d_wgrad_split(x, aff, dz, scales, cout):
    """dW on the F16 matrix cores (csrc/conv3d_wgrad_split.hip): dz scaled by scales[0] inside the kernel, the result rescaled in its reduction"""
    n, cin, edge = x.shape[0], x.shape[1], x.shape[2]
    lib = _lib.load()
    dw = torch.empty((cout, cin, 3, 3, 3), dtype=torch.float32, device=x.device)
    ws = _ws(x.device, lib.rf_conv3d_k3_wgrad_split_ws_bytes(cin, cout, n, edge))
    lib.rf_conv3d_k3_wgrad_split(_p(x), cin, n, edge, _p(aff), _p(dz), cout, _p(scales), _p(dw), _p(ws), ws.numel(), _stream())
    return dw


def dgrad_split_supported(dz, weight, cin):
    n, cout, edge = dz.shape[0], dz.shape[1], dz.shape[2]
    return (ops.CONV_ARITH == 'split' and dz.numel() % 4 == 0 and bool(_lib.load().rf_conv3d_split_k3_gn_supported(cout, n, edge, cin))
            and ops.split_range_ok(weight))


@ops._device_scoped
def conv3d_gn(x, aff, w_packed, cout, relu):
    n, c, edge = x.shape[0], x.shape[1], x.shape[2]
    out = torch.empty((n, cout, edge, edge, edge), dtype=torch.float32, device=x.device)
    _lib.load().rf_conv3d_k3_gn(_p(x), c, _p(None), 0, n, edge, _p(aff), _p(w_packed), cout, int(relu), _p(out), _stream())
    return out


@ops._device_scoped
def gn_backward(x, dxn, gamma, groups, eps, inv_scale=None):
    """dx, dgamma, dbeta of GroupNorm; ``inv_scale``: a device scalar when dxn arrives multiplied by 1 / inv_scale (the scaled split data gradient)"""
    n, c, edge = x.shape[0], x.shape[1], x.shape[2]
    lib = _lib.load()
    dx = torch.empty_like(x)
    dg = torch.empty(c, dtype=torch.float32, device=x.device)
    db = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = _ws(x.device, lib.rf_gn_backward_ws_bytes(n, c, edge))
    lib.rf_gn_backward(_p(x), _p(dxn), n, c, edge, _p(gamma), groups, eps, _p(inv_scale), _p(dx), _p(dg), _p(db), _p(ws), ws.numel(), _stream())
    return dx, dg, db


@ops._device_scoped
def conv3d_wgrad(x, aff, dz, cout):
    n, cin, edge = x.shape[0], x.shape[1], x.shape[2]
    lib = _lib.load()
    dw = torch.empty((cout, cin, 3, 3, 3), dtype=torch.float32, device=x.device)
    ws = _ws(x.device, lib.rf_conv3d_k3_wgrad_ws_bytes(cin, cout, n, edge))
    lib.rf_conv3d_k3_wgrad(_p(x), cin, n, edge, _p(aff), _p(dz), cout, _p(dw), _p(ws), ws.numel(), _stream())
    return dw


class ConvGnRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, weight, groups, eps, skip=None, low=None):
        """``skip`` / ``low``: for a decoder layer, the two sources x was concatenated from (full-resolution skip or None, low-resolution source):
        hints for the forward kernel only (the decoder form convolves the upsampled channels in low resolution), no gradient flows to them."""
        x = x.contiguous()
        n, cin, edge = x.shape[0], x.shape[1], x.shape[2]
        cout = weight.shape[0]
        g = 1 if cin < groups else groups
        with torch.no_grad():
            aff = ops.gn_affine(x, None, gamma, beta, g, eps)
            w = weight.contiguous()
            # the inference kernels, in routes.single's order for a written-out concatenation (one batched range check per optimiser step, ops._abs_max)
            split_ok = routes.split_arith(lambda: ops.split_range_ok(weight, gamma, beta, (cin // g) * edge ** 3))
            c1 = low.shape[1] if low is not None else 0
            route = routes.single(n, cin - c1, c1, edge, cout, None, split_ok, materialised=True)
            if route == 'e2':
                y = ops.conv3d_e2_split_gn_relu(x, aff, ops.pack_conv3_e2_split_weight(w, edge), cout)
            elif route == 'direct':
                y = ops.conv3d_gn_relu(x, None, aff, None, cout, direct_weight=w)
            elif route == 'split_box':
                y = ops.conv3d_split_gn_relu(x, aff, ops.pack_conv3_split_weight(w), cout)
            elif route == 'up_split':
                y = ops.conv3d_up_split_gn_relu(skip, low, aff, ops.pack_conv3_up_split_weight(w, cin - c1), cout)
            else:
                y = ops.conv3d_gn_relu(x, None, aff, ops.pack_conv3_weight(w), cout)
        ctx.save_for_backward(x, gamma, weight, aff, y)
        ctx.groups, ctx.eps, ctx.split_ok = g, eps, bool(split_ok) and edge > 1
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, weight, aff, y = ctx.saved_tensors
        n, cin, edge = x.shape[0], x.shape[1], x.shape[2]
        cout = weight.shape[0]
        # what nobody asked for is not computed (a frozen network inside a training step: no weight-gradient launches; an input that is data: no
        # data gradient); what is asked for keeps its bits.  GroupNorm's backward gives dx, dgamma and dbeta together and needs the data gradient.
        need_x, need_gamma, need_beta, need_w = ctx.needs_input_grad[:4]
        need_dgrad = need_x or need_gamma or need_beta
        if not (need_dgrad or need_w):
            return (None,) * 8
        with torch.no_grad():
            inv_s = scales = None
            use_dgrad = need_dgrad and edge >= 4 and dgrad_split_supported(y, weight, cin)
            use_wgrad = need_w and ctx.split_ok and y.numel() % 4 == 0 and bool(_lib.load().rf_conv3d_k3_wgrad_split_supported(cin, cout, n, edge))
            if use_dgrad or use_wgrad:
                dz, amax = relu_backward_amax(dy.contiguous(), y)
                ident, scales = dz_scale(amax, n, cout)
            else:
                dz = relu_backward(dy.contiguous(), y) if y.numel() % 4 == 0 else dy * (y > 0)
            dxn = dw = None
            if not need_dgrad:
                pass
            elif use_dgrad:
                dxn, inv_s = dgrad_split(dz, ident, weight, cin), scales[1:]
            elif edge >= 2:
                wt = weight.flip(2, 3, 4).transpose(0, 1).contiguous()          # [cin, cout, 3,3,3]: the data-gradient conv's weight
                ident = torch.zeros((n, cout, 4), dtype=torch.float32, device=x.device)
                ident[..., 1] = 1.0
                dxn = conv3d_gn(dz, ident, ops.pack_conv3_weight(wt), cin, relu=False)
            else:                                                                   # 1^3 volume: only the centre tap touches data
                dxn = ops.linear(dz.reshape(n, cout), ops.pack_linear_weight(weight[:, :, 1, 1, 1].t().contiguous()), None, cin).reshape(n, cin, 1, 1, 1)
            if not need_w:
                pass
            elif use_wgrad:
                dw = conv3d_wgrad_split(x, aff, dz, scales, cout)
            elif edge >= 4:
                dw = conv3d_wgrad(x, aff, dz, cout)
            else:
                # small volumes: dW = dz^T . im2col(GN(x)) through rf_linear (the operands are re-laid by torch, the products run on rf_linear_wgrad's split-K MFMA GEMM)
                xn = torch.addcmul(aff[..., 2, None, None, None], x - aff[..., 0, None, None, None], aff[..., 1, None, None, None])
                cols = F.pad(xn, (1, 1, 1, 1, 1, 1)).unfold(2, 3, 1).unfold(3, 3, 1).unfold(4, 3, 1)       # [n, cin, e,e,e, 3,3,3]
                cols = cols.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(n * edge ** 3, cin * 27)
                dzf = dz.permute(0, 2, 3, 4, 1).reshape(n * edge ** 3, cout)
                dw = ops.linear_wgrad(dzf.contiguous(), cols.contiguous()).reshape(cout, cin, 3, 3, 3)
            # (d xn of the split data gradient came scaled by s: GroupNorm backward is linear in it and takes 1 / s out)
            dx = dgamma = dbeta = None
            if need_dgrad:
                dx, dgamma, dbeta = gn_backward(x, dxn.contiguous(), gamma, ctx.groups, ctx.eps, inv_s)
        return (dx if need_x else None, dgamma if need_gamma else None, dbeta if need_beta else None, dw, None, None, None, None)


class Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        x = x.contiguous()
        with torch.no_grad():
            y = ops.linear(x, ops.pack_linear_weight(weight.contiguous()), bias, weight.shape[0], act, slope)
        ctx.save_for_backward(x, weight, y)
        ctx.act, ctx.slope, ctx.has_bias = act, slope, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        with torch.no_grad():
            if ctx.act == ops.ACT_NONE:
                dpre = dy.contiguous()
            else:                                                   # y > 0 <=> pre-activation > 0 for ReLU and LeakyReLU(slope > 0)
                dpre = torch.where(y > 0, dy, dy * (ctx.slope if ctx.act == ops.ACT_LEAKY else 0.0)).contiguous()
            need_x, need_w, need_b = ctx.needs_input_grad[:3]
            dx = ops.linear(dpre, ops.pack_linear_weight(weight.t().contiguous()), None, weight.shape[1]) if need_x else None
            dw = ops.linear_wgrad(dpre, x) if need_w else None
            db = dpre.double().sum(0).float() if ctx.has_bias and need_b else None
        return dx, dw, db, None, None


class PointwiseTanh(torch.autograd.Function):
    """the final decoder's head, tanh(Conv3d(nf, 1, 1)): rf_conv1x1_tanh forward (the inference kernel), rf_pointwise_tanh_backward backward.  x and the
    output are saved; nothing of the size of [B, 1, nf, 64^3] is ever materialised.  At most 64 channels and a multiple of four voxels, checked in the
    forward.  A frozen head (neither weight nor bias asks for a gradient) costs the data gradient alone: no sums, no second launch."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = x.contiguous()
        if not ops.pointwise_tanh_supported(x.shape[0], x.shape[1], x[0, 0].numel()):
            raise NotImplementedError('PointwiseTanh: %s is outside what its backward supports (1 <= channels <= 64, voxels %% 4 == 0)' % (tuple(x.shape),))
        with torch.no_grad():
            y = ops.conv1x1_tanh(x, weight, bias)
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        with torch.no_grad():
            dx, dw, db = ops.pointwise_tanh_backward(x, y, dy.contiguous(), weight, sums=need_w or need_b)
        return dx if need_x else None, dw if need_w else None, db if need_b else None


class AttnFuse(torch.autograd.Function):
    """rf_attn_fuse forward, rf_attn_fuse_backward backward: x [b,c,e,e,e]-like, p [b,K,...], xf [b,f] / pf [b*K,f] the RAW encoder outputs, noise [b,K]
    or None.  Only the inputs are saved: the backward kernel recomputes the row's scores, switch and weights with the forward's code."""

    @staticmethod
    def forward(ctx, x, p, xf, pf, noise, mode, sharpness):
        x, p, xf, pf = x.contiguous(), p.contiguous(), xf.contiguous(), pf.contiguous()
        noise = noise.contiguous() if noise is not None else None
        ctx.save_for_backward(x, p, xf, pf, noise)
        ctx.mode, ctx.sharpness = mode, sharpness
        with torch.no_grad():
            return ops.attn_fuse(x, p, xf, pf, noise, mode, sharpness)

    @staticmethod
    def backward(ctx, dout):
        x, p, xf, pf, noise = ctx.saved_tensors
        with torch.no_grad():
            dx, dp, dxf, dpf = ops.attn_fuse_backward(x, p, xf, pf, noise, dout.contiguous(), ctx.mode, ctx.sharpness, ctx.needs_input_grad[:4])
        return dx, dp, dxf, dpf, None, None, None


class Unfold3d(torch.autograd.Function):
    """rf_unfold3d forward, rf_fold3d backward (each is the other's exact inverse index map)"""

    @staticmethod
    def forward(ctx, x, e):
        ctx.r, ctx.e, ctx.c = x.shape[2] // e, e, x.shape[1]
        with torch.no_grad():
            return ops.unfold3d(x.contiguous(), e)

    @staticmethod
    def backward(ctx, drows):
        with torch.no_grad():
            return ops.fold3d(drows.contiguous(), ctx.r, ctx.e, ctx.c), None


class Fold3d(torch.autograd.Function):
    """rf_fold3d forward, rf_unfold3d backward"""

    @staticmethod
    def forward(ctx, rows, r, e, c):
        ctx.e = e
        with torch.no_grad():
            return ops.fold3d(rows.contiguous(), r, e, c)

    @staticmethod
    def backward(ctx, dx):
        with torch.no_grad():
            return ops.unfold3d(dx.contiguous(), ctx.e), None, None, None


class GatherRetrieved(torch.autograd.Function):
    """rf_attn_gather_retrieved forward (layout 0: folded volumes, 1: the retrieval backbone's patch-major output), rf_attn_scatter_retrieved backward"""

    @staticmethod
    def forward(ctx, src, layout, b, k, c, s, e, t):
        ctx.args, ctx.shape = (layout, b, k, c, s, e, t), src.shape
        with torch.no_grad():
            return ops.attn_gather_retrieved(src.contiguous(), layout, b, k, c, s, e, t)

    @staticmethod
    def backward(ctx, dp_rows):
        with torch.no_grad():
            dsrc = ops.attn_scatter_retrieved(dp_rows.contiguous(), *ctx.args)
        return dsrc.reshape(ctx.shape), None, None, None, None, None, None, None


class ConvValidLeaky(torch.autograd.Function):
    """one layer of a conv patch encoder; ``layer`` (a model.unet.Conv3dParams holding weight / bias) and ``encoder`` (its _ConvPatchEncoder) pick the
    forward kernel and hold the cached weight images, no gradient flows to them"""

    @staticmethod
    def forward(ctx, x, weight, bias, layer, encoder, slope):
        x = x.contiguous()
        with torch.no_grad():
            y = encoder._conv(layer, x)
        ctx.save_for_backward(x, weight, y)
        ctx.k, ctx.stride, ctx.slope = layer.kernel_size, layer.stride, slope
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        with torch.no_grad():
            dz, db = ops.conv3d_valid_leaky_backward(dy.contiguous(), y, ctx.slope)
            dx = None
            if ctx.needs_input_grad[0]:
                dx = ops.conv3d_valid_dgrad(dz, ops.pack_convv_dgrad_weight(weight), x.shape[1], ctx.k, ctx.stride, x.shape[2])
            dw = ops.conv3d_valid_wgrad(x, dz, ctx.k, ctx.stride) if ctx.needs_input_grad[1] else None
        return dx, dw, db if ctx.needs_input_grad[2] else None, None, None, None


@ops._device_scoped
def upsample2(x):
    ops._req(x, 'x')
    n, c, e = x.shape[0], x.shape[1], x.shape[2]
    out = torch.empty((n, c, 2 * e, 2 * e, 2 * e), dtype=torch.float32, device=x.device)
    _lib.load().rf_upsample3d_2(_p(x), n, c, e, _p(out), _stream())
    return out


@ops._device_scoped
def sumpool2(g):
    ops._req(g, 'g')
    n, c, e = g.shape[0], g.shape[1], g.shape[2]
    out = torch.empty((n, c, e // 2, e // 2, e // 2), dtype=torch.float32, device=g.device)
    _lib.load().rf_sumpool3d_2(_p(g), n, c, e, _p(out), _stream())
    return out


@ops._device_scoped
def maxpool2_backward(x, g):
    ops._req(x, 'x'), ops._req(g, 'g')
    n, c, e = x.shape[0], x.shape[1], x.shape[2]
    dx = torch.empty_like(x)
    _lib.load().rf_maxpool3d_2_backward(_p(x), _p(g), n, c, e, _p(dx), _stream())
    return dx


class _Upsample2(torch.autograd.Function):
    """nearest x2 upsample (rf_upsample3d_2) whose backward is the 2x2x2 sum pool (rf_sumpool3d_2): torch's upsample_nearest3d_backward took 0.48 ms
    per call on a [4,16,64^3] gradient, its avg_pool3d and upsample kernels launch 32 workgroups on the retrieval backbone's shapes"""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        if x.shape[2] < 2 or x.shape[2] % 2:
            return F.interpolate(x, scale_factor=2, mode='nearest')
        return upsample2(x)

    @staticmethod
    def backward(ctx, g):
        return sumpool2(g.contiguous())


class _MaxPool2(torch.autograd.Function):
    """MaxPool3d(2): forward rf_maxpool3d_2, backward rf_maxpool3d_2_backward (the gradient to the first maximum of a cell, like torch)"""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        with torch.no_grad():
            return ops.maxpool2(x)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return maxpool2_backward(x, g.contiguous())


def max_pool2(x):
    return _MaxPool2.apply(x) if x.shape[2] % 2 == 0 and x.shape[2] >= 2 else F.max_pool3d(x, 2)


def conv_gn_relu(x, upsampled, gamma, beta, weight, groups, eps):
    """grad-mode SingleConv: two-source (decoder) layers are differentiated through a materialised nearest-x2 upsample + concat"""
    skip = low = None
    if upsampled is not None:
        skip, low = (x.detach().contiguous() if x is not None else None), upsampled.detach().contiguous()
        up = _Upsample2.apply(upsampled)
        x = up if x is None else torch.cat((x, up), dim=1)
    return ConvGnRelu.apply(x, gamma, beta, weight, groups, eps, skip, low)
