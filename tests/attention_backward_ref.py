"""References for the backward of the patch attention's row route (csrc/attention_backward.hip, rfuse.autograd.AttnFuse / GatherRetrieved):

  reference_f64        the formulas of include/rfuse.h / csrc/attention_backward.hip written out in float64 torch, with the first-max rule
                       (the switch's gradient goes to the FIRST index of the maximal score, like F.max_pool1d / max(dim))
  torch_formula        the element-wise torch formula the modules used in grad mode before the HIP backward existed (amax switch), kept here as the
                       fp32 comparator of the accuracy tests and of tools/attn_backward_bench.py
  torch_patched_forward  that formula at module level: unfold / regroup / fold as permuted views around it
  gather_view / gather_view_inverse  the regroup of the retrieved features as the view / permute formula, and its inverse
"""
import torch
import torch.nn.functional as F

SOFTMAX, GUMBEL_HARD = 0, 1


def reference_f64(x, p, xf, pf, noise, dout, mode, sharpness):
    """x [R,d], p [R,K,d], xf [R,f], pf [R,K,f], noise [R,K] | None, dout [R,d] (any float dtype; evaluated in float64 on the CPU)
    -> dict(dx, dp, dxf, dpf, score_gap, logit_gap): the four gradients, and per row the distance between the two largest scores / logits
    (inf for K = 1) -- the discrete decisions' margins."""
    x, p, xf, pf, g = (t.detach().double().cpu() for t in (x, p, xf, pf, dout))
    R, K = p.shape[0], p.shape[1]
    x, g, p = x.reshape(R, -1), g.reshape(R, -1), p.reshape(R, K, -1)
    pf = pf.reshape(R, K, -1)
    xnorm, pnorm = xf.norm(dim=1, keepdim=True), pf.norm(dim=2, keepdim=True)
    xden, pden = xnorm.clamp_min(1e-12), pnorm.clamp_min(1e-12)
    xn, pn = xf / xden, pf / pden
    s = (xn[:, None, :] * pn).sum(dim=2)                                    # [R,K]
    smax, kstar = s.max(dim=1)                                              # first maximal index
    sw = smax.clamp_min(0.0)[:, None]
    if mode == SOFTMAX:
        a = float(sharpness)
        y = torch.softmax(a * s, dim=1)
        w = y
        logits = a * s
    else:
        a = 25.0
        logits = a * s + noise.detach().double().cpu()
        y = torch.softmax(logits, dim=1)
        w = torch.zeros_like(y).scatter_(1, y.argmax(dim=1, keepdim=True), 1.0)
    dx = g * (1.0 - sw)
    dp = g[:, None, :] * (w * sw)[:, :, None]
    dsw = (g * ((w[:, :, None] * p).sum(dim=1) - x)).sum(dim=1)             # [R]
    dw = sw * (g[:, None, :] * p).sum(dim=2)                                # [R,K]
    ds = a * y * (dw - (y * dw).sum(dim=1, keepdim=True))
    ds[torch.arange(R), kstar] += torch.where(smax > 0, dsw, torch.zeros_like(dsw))
    dxn = (ds[:, :, None] * pn).sum(dim=1)
    dpn = ds[:, :, None] * xn[:, None, :]
    dxf = torch.where(xnorm > 1e-12, dxn - xn * (xn * dxn).sum(dim=1, keepdim=True), dxn) / xden
    dpf = torch.where(pnorm > 1e-12, dpn - pn * (pn * dpn).sum(dim=2, keepdim=True), dpn) / pden

    def gap(v):
        if K == 1:
            return torch.full((R,), float('inf'), dtype=torch.float64)
        top = v.topk(2, dim=1).values
        return top[:, 0] - top[:, 1]
    return dict(dx=dx, dp=dp, dxf=dxf, dpf=dpf, score_gap=gap(s), logit_gap=gap(logits))


def torch_formula(x, p, xf, pf, noise, mode, sharpness, first_max=False):
    """The grad-mode formula of model/attention.py before rf_attn_fuse_backward: differentiable torch ops in the dtype and on the device of the
    inputs; x [R,...], p [R,K,...], xf [R,f], pf [R*K,f] or [R,K,f] RAW encoder outputs -> out shaped like x.  ``first_max``: the switch through
    max(dim) as the oracle writes it (gradient to the first maximal score) in place of the formula's amax (gradient split among ties)."""
    b, k = p.shape[0], p.shape[1]
    xn = F.normalize(xf, dim=1)
    pn = F.normalize(pf.reshape(b * k, -1), dim=1).reshape(b, k, -1)
    scores = (xn.unsqueeze(1) * pn).sum(dim=2)                                   # [b, K]
    switch = (scores.max(dim=1, keepdim=True).values if first_max else scores.amax(dim=1, keepdim=True)).clamp_min(0.0)
    if mode == GUMBEL_HARD:
        soft = torch.softmax(scores * 25.0 + noise, dim=1)
        hard = torch.zeros_like(soft).scatter_(1, soft.argmax(dim=1, keepdim=True), 1.0)
        weights = hard - soft.detach() + soft                                    # straight-through estimator of gumbel_softmax(hard=True)
    else:
        weights = torch.softmax(scores * float(sharpness), dim=1)
    mixed = (weights.unsqueeze(2) * p.reshape(b, k, -1)).sum(dim=1)
    flat = x.reshape(b, -1)
    return (flat * (1.0 - switch) + mixed * switch).reshape(x.shape)


def torch_formula_grads(x, p, xf, pf, noise, dout, mode, sharpness, first_max=False):
    """(dx, dp, dxf, dpf) of torch_formula by autograd, in the dtype and on the device of the inputs"""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, p, xf, pf)]
    out = torch_formula(*leaves, noise, mode, sharpness, first_max)
    return torch.autograd.grad(out, leaves, dout.reshape(out.shape))


def unfold_view(v, e):
    n, c, s = v.shape[0], v.shape[1], v.shape[2]
    r = s // e
    return v.reshape(n, c, r, e, r, e, r, e).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(-1, c, e, e, e)


def fold_view(rows, r, e, c):
    return rows.reshape(-1, r, r, r, c, e, e, e).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(-1, c, r * e, r * e, r * e)


def gather_view(src, layout, b, k, c, s, e, t=0):
    """rf_attn_gather_retrieved as views: src = folded volumes [b*k, c, s,s,s] (layout 0) or patch-major [(b*k*q^3), c, t,t,t] (layout 1)
    -> rows [(b*r^3), k, c, e,e,e]"""
    r = s // e
    vols = src if layout == 0 else fold_view(src, s // t, t, c)
    rows = vols.reshape(b * k, c, r, e, r, e, r, e).permute(0, 2, 4, 6, 1, 3, 5, 7)                   # [bk, r,r,r, c, e,e,e]
    return rows.reshape(b, k, r, r, r, c, e, e, e).permute(0, 2, 3, 4, 1, 5, 6, 7, 8).reshape(-1, k, c, e, e, e)


def gather_view_inverse(rows, layout, b, k, c, s, e, t=0):
    """the inverse index map of gather_view (= its backward: the map is a bijection)"""
    r = s // e
    v = rows.reshape(b, r, r, r, k, c, e, e, e).permute(0, 4, 1, 2, 3, 5, 6, 7, 8).reshape(b * k * r ** 3, c, e, e, e)
    vols = fold_view(v, r, e, c)
    return vols if layout == 0 else unfold_view(vols, t)


def torch_patched_forward(block, x_predicted, retrieved, layout, patch_edge, noise):
    """PatchedAttentionBlock's grad-mode route before the HIP backward: views around torch_formula; the encoders run as the module runs them"""
    att = block.attention_blocks_layer
    b, c, s = x_predicted.shape[0], x_predicted.shape[1], x_predicted.shape[-1]
    e, k = block.patch_extent, block.num_nearest_neighbors
    r = s // e
    x_rows = unfold_view(x_predicted, e)
    p_rows = gather_view(retrieved, layout, b, k, c, s, e, patch_edge)
    xf = att.theta(x_rows)
    pf = att.phi(p_rows.reshape((x_rows.shape[0] * k,) + tuple(p_rows.shape[2:])))
    mode = GUMBEL_HARD if att.retrieval_mode else SOFTMAX
    out = torch_formula(x_rows, p_rows, xf, pf, noise, mode, float((att.cf_feat * e ** 3) * 4))
    return fold_view(out, r, e, c)


def make_inputs(R, K, d, f, seed, device='cpu'):
    """the accuracy tests' inputs: features spread so that the softmax weights are neither uniform nor one-hot"""
    g = torch.Generator().manual_seed(seed)
    xf = torch.randn(R, f, generator=g)
    pf = xf[:, None] * (1 + 0.3 * torch.rand(R, K, 1, generator=g)) + 0.1 * torch.randn(R, K, f, generator=g)
    x = torch.randn(R, d, generator=g)
    p = torch.randn(R, K, d, generator=g)
    dout = torch.randn(R, d, generator=g)
    noise = -torch.empty(R, K).exponential_(generator=g).log()
    return tuple(t.to(device).contiguous() for t in (x, p, xf, pf, noise, dout))


def tie_inputs(K=4, f=32, d=16):
    """rows whose two best slots (1 and 2) hold bit-identical pf: the duplicate-retrieval tie"""
    x, p, xf, pf, noise, dout = make_inputs(32, K, d, f, seed=5)
    gen = torch.Generator().manual_seed(6)
    pf = pf + 1.0 * torch.randn(pf.shape, generator=gen)                   # the other slots: cosine about 0.75
    pf[:, 1] = xf * 1.25 + 0.5 * torch.randn(xf.shape, generator=gen)      # the tied pair: about 0.93, so the switch is well inside (0, 1)
    pf[:, 2] = pf[:, 1]
    return x, p, xf, pf.contiguous(), noise, dout


def dead_inputs(K=4, f=32, d=16):
    """every score negative: the switch relu(max score) is 0 and passes no gradient"""
    x, p, xf, pf, noise, dout = make_inputs(32, K, d, f, seed=9)
    return x, p, xf, (-pf).contiguous(), noise, dout


def rel_err(a, ref):
    """max-abs error over the tensor divided by the reference's max-abs"""
    a, ref = a.detach().double().cpu().reshape(ref.shape), ref.detach().double().cpu()
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
