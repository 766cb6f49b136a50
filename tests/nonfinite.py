"""Helpers of the non-finite parity tests (tests/test_nonfinite_gpu.py, tests/test_nonfinite_cpu.py).

A kernel fed a NaN or an infinity must hand it on the way the float64 reference does: the comparators below check the
non-finite masks first and the finite values second, and the dependency cones say -- combinatorially, without running the
op -- which outputs an injected input position can reach, so that a reference which skips a product by zero (NaN * 0 must
stay NaN) is caught too."""
import torch
import torch.nn.functional as F


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def bit_equal_nan(a, b):
    """same NaN mask, and the same bits (signed zeros and infinities included) everywhere else; NaN payloads are not compared"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(_bits(a)[~na], _bits(b)[~nb])


def assert_bit_equal_nan(a, b, what=''):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), f'{what}: NaN masks differ at {int((na != nb).sum())} positions, first {_first(na != nb)}'
    diff = _bits(a) != _bits(b)
    diff &= ~na
    assert not diff.any(), f'{what}: {int(diff.sum())} positions with other bits, first {_first(diff)}: {a[diff][:4].tolist()} vs {b[diff][:4].tolist()}'


def _first(mask):
    idx = mask.nonzero()
    return tuple(idx[0].tolist()) if idx.numel() else None


def assert_close_nonfinite(got, ref, tol, what=''):
    """NaN / +inf / -inf masks equal, then the finite positions within ``tol * max(1, max |finite ref|)``"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for name, fn in (('NaN', torch.isnan), ('+inf', torch.isposinf), ('-inf', torch.isneginf)):
        mg, mr = fn(got), fn(ref)
        assert torch.equal(mg, mr), (f'{what}: {name} masks differ: {int((mg & ~mr).sum())} extra (first {_first(mg & ~mr)}), '
                                     f'{int((mr & ~mg).sum())} missing (first {_first(mr & ~mg)}) of {int(mr.sum())}')
    assert_close_finite(got, ref, torch.isfinite(ref), tol, what)


def assert_close_finite(got, ref, where, tol, what=''):
    """|got - ref| within the bar on the positions ``where`` (which must be finite in both)"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not where.any():
        return
    g, r = got[where], ref[where]
    assert torch.isfinite(g).all() and torch.isfinite(r).all(), f'{what}: non-finite values among the positions compared'
    err = (g - r).abs().max().item()
    bound = tol * max(1.0, r.abs().max().item())
    assert err <= bound, f'{what}: max abs err {err:.3e} > {bound:.3e} on the finite positions'


# ---- dependency cones: bool masks [n, C, D, H, W] of the positions an injected input set can reach

def cone_conv(mask, cout, k=3, stride=1, padding=1):
    """outputs of a dense Conv3d(k, stride, padding) -- every output channel -- that read a marked input position of any channel"""
    m = mask.any(dim=1, keepdim=True).float()
    hit = F.max_pool3d(m, k, stride, padding) > 0 if padding == 0 else _dilate(m, k, stride, padding)
    return hit.expand(-1, cout, -1, -1, -1).clone()


def _dilate(m, k, stride, padding):
    # max_pool3d pads with -inf, which a 0 / 1 mask reads as "not marked": the zero padding of the conv adds no dependency
    return F.max_pool3d(m, k, stride, padding) > 0


def cone_up2(mask):
    """positions of a 2x nearest upsample that copy a marked position"""
    return F.interpolate(mask.float(), scale_factor=2, mode='nearest') > 0


def cone_pool2(mask):
    """outputs of MaxPool3d(2) whose window holds a marked position"""
    return F.max_pool3d(mask.float(), 2) > 0


def point_mask(shape, points):
    """bool mask of ``shape`` [n, C, D, H, W] with the (sample, channel, z, y, x) ``points`` set"""
    m = torch.zeros(shape, dtype=torch.bool)
    for p in points:
        m[p] = True
    return m
