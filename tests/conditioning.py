"""Ill-conditioned inputs for the GroupNorm-conv kernels (plain torch, importable without a GPU).

Every other kernel test of the conv stack draws relu(randn): mean 0.4, deviation 0.6, no structure.  The data the product exists for is a TSDF chunk
(mostly the truncation constant, a thin band of smaller values), exactly constant empty patches and post-ReLU feature maps with whole dead groups.  On
those the two-term form  x * scale' + shift'  of GroupNorm loses 10x .. 100x the bar of the kernel tests, the centre-first form
(x - fl32(mean)) * scale + shift  with float64 statistics (csrc/common.h: gn_affine) does not: tests/test_conditioning_cpu.py asserts both, so the
families below separate a correct kernel from one that folded the centre into the shift or summed its statistics in fp32.
"""
import torch

FAMILIES = ('relu_randn', 'saturated', 'near_constant', 'constant', 'big_mean', 'spike', 'dead_groups', 'scaled_up', 'scaled_down')


def gn_groups(c, groups):
    return 1 if c < groups else groups                                  # model/unet.py:62-63


def make(family, gen, n, c, edge, groups):
    """one fp32 source [n, c, edge, edge, edge] of ``family``; ``groups`` as the layer is configured (one group when c < groups)"""
    shape = (n, c, edge, edge, edge)
    g = gn_groups(c, groups)
    randn = lambda: torch.randn(*shape, generator=gen)
    if family == 'relu_randn':                                          # today's input, as the control
        x = randn().relu()
    elif family == 'saturated':                                         # truncation-saturated TSDF: the constant, ~2 % of the voxels in [0, 3)
        band = torch.rand(*shape, generator=gen) < 0.02
        x = torch.where(band, 3.0 * torch.rand(*shape, generator=gen), torch.full(shape, 3.0))
    elif family == 'near_constant':                                     # var << eps: rstd near its 1 / sqrt(eps) = 316 ceiling
        x = 3.0 + 1e-4 * randn()
    elif family == 'constant':                                          # var == 0 exactly: the output is the conv of beta
        x = torch.full(shape, 3.0)
    elif family == 'big_mean':
        x = 1000.0 + randn()
    elif family == 'spike':                                             # one voxel of 5.0 in the first channel of each group, zeros elsewhere:
        x = torch.zeros(shape)                                          # |x - mean| rstd attains the sqrt(group elements) bound of ops.split_range_ok
        pos = torch.randint(0, edge ** 3, (n, g), generator=gen)
        first = x.view(n, g, c // g, edge ** 3)[:, :, 0]
        first.scatter_(2, pos[..., None], 5.0)
    elif family == 'dead_groups':                                       # post-ReLU feature maps: the channels of the first half of the groups all zero
        x = randn().relu()
        if g < 2:
            x.zero_()
        else:
            x[:, :(g // 2) * (c // g)] = 0.0
    elif family == 'scaled_up':
        x = randn().relu() * 2.0 ** 40
    elif family == 'scaled_down':
        x = randn().relu() * 2.0 ** -40
    else:
        raise ValueError('unknown family %r' % (family,))
    return x.float().contiguous()


def mixed(gen, n, c, edge, groups, families=FAMILIES):
    """-> (x [n, c, edge^3] fp32, family of each sample): sample i is of family i mod F, so one launch of a many-sample form covers them all"""
    x = torch.empty(n, c, edge, edge, edge)
    nf = len(families)
    for i, fam in enumerate(families[:n]):
        idx = torch.arange(i, n, nf)
        x[idx] = make(fam, gen, len(idx), c, edge, groups)
    return x, [families[i % nf] for i in range(n)]


def mixed_pair(gen, n, c0, c1, edge, groups, families=FAMILIES):
    """a decoder layer's two sources (skip [n, c0, edge^3] or None, low resolution [n, c1, (edge/2)^3] or None), the same family for both in every
    sample; each source is drawn with ``groups`` of its own (the layer's groups run over the concatenation and may straddle the two)"""
    src0 = mixed(gen, n, c0, edge, groups, families)[0] if c0 else None
    src1 = mixed(gen, n, c1, edge // 2, groups, families)[0] if c1 else None
    return src0, src1, [families[i % len(families)] for i in range(n)]


def reference_subset(n, nfam=len(FAMILIES)):
    """samples on which a many-sample case computes its float64 reference: the first two of every family and the last ``nfam`` (the ragged last
    workgroup)"""
    return sorted(set(range(min(n, 2 * nfam))) | set(range(max(0, n - nfam), n)))


TABLE = {}                                                              # (what, family) -> worst error / max(floor, |ref|max) seen in this process


def per_sample_errors(got, ref64, floor=1.0):
    got, ref = got.detach().cpu().double(), ref64.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    n = got.shape[0]
    err = (got - ref).abs().reshape(n, -1).max(dim=1).values
    err = torch.where(torch.isfinite(got).reshape(n, -1).all(dim=1), err, torch.full_like(err, float('inf')))
    return err / ref.abs().reshape(n, -1).max(dim=1).values.clamp_min(floor)


def per_sample_close(got, ref64, tol, families, what, floor=1.0):
    """every sample within  tol * max(floor, |ref_sample|max)  of the float64 reference: floor = 1 for forward outputs (like ``close`` of the kernel tests),
    1e-30 for gradients.  The worst error of each family goes into TABLE and, on failure, into the message.  -> {family: worst}"""
    rel = per_sample_errors(got, ref64, floor)
    assert len(families) == len(rel), (len(families), len(rel))
    worst = {}
    for fam, r in zip(families, rel.tolist()):
        worst[fam] = max(worst.get(fam, 0.0), r)
    for fam, r in worst.items():
        TABLE[(what, fam)] = max(TABLE.get((what, fam), 0.0), r)
    bad = {fam: '%.2e' % r for fam, r in worst.items() if not r <= tol}
    assert not bad, '%s: per-sample error above %.1e of max(%g, |ref|max) on %s (all families: %s)' % (
        what, tol, floor, bad, {fam: '%.1e' % r for fam, r in worst.items()})
    return worst


def tensor_close(got, ref64, tol, what, floor=1e-30):
    """one bound for the whole tensor (dW, dgamma, dbeta, affine columns): max error <= tol * max(floor, |ref|max); recorded in TABLE under 'all'"""
    got, ref = got.detach().cpu().double(), ref64.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = float((got - ref).abs().max() / ref.abs().max().clamp_min(floor)) if bool(torch.isfinite(got).all()) else float('inf')
    TABLE[(what, 'all')] = max(TABLE.get((what, 'all'), 0.0), r)
    assert r <= tol, '%s: error %.2e of max(%g, |ref|max) > %.1e' % (what, r, floor, tol)
    return r


def format_table():
    lines = ['%-78s %-14s %s' % ('form', 'family', 'worst error / max(floor, |ref|max) per sample')]
    for (what, fam), r in sorted(TABLE.items()):
        lines.append('%-78s %-14s %.2e' % (what, fam, r))
    return '\n'.join(lines)


# ---- CPU emulations of the two ways a kernel can apply GroupNorm in fp32 (statistics in float64 in both)

def group_stats64(x, g):
    n, c = x.shape[0], x.shape[1]
    xg = x.double().reshape(n, g, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    return mean.repeat_interleave(c // g, 1), rstd.repeat_interleave(c // g, 1)          # [n, c] each


def affine_centre_form(x, gamma, beta, groups):
    """[n, c, 3] float32 (centre, scale, shift) as csrc/common.h: gn_affine defines them"""
    mean, rstd = group_stats64(x, gn_groups(x.shape[1], groups))
    sc = gamma.double()[None] * rstd
    centre = mean.float()
    return torch.stack([centre, sc.float(), (beta.double()[None] - (mean - centre.double()) * sc).float()], -1)


def gn_centre_form_fp32(x, gamma, beta, groups):
    a = affine_centre_form(x, gamma, beta, groups)[..., None, None, None]
    return (x - a[:, :, 0]) * a[:, :, 1] + a[:, :, 2]                                     # fp32 throughout


def gn_two_term_fp32(x, gamma, beta, groups):
    mean, rstd = group_stats64(x, gn_groups(x.shape[1], groups))
    sc = gamma.double()[None] * rstd
    scale, shift = sc.float()[..., None, None, None], (beta.double()[None] - mean * sc).float()[..., None, None, None]
    return x * scale + shift
