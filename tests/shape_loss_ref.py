"""The shape loss restated from its formulas in plain torch (any dtype, float64 in the tests), independent of both the reference's code and the kernels:
used by tests/test_shape_loss_cpu.py to check the fixture and by tests/test_shape_loss_gpu.py as the float64 side of the end-to-end test.

    df(p) = (p + 1) * trunc / 2,  den(T) = T * std + mean
    W = 1 + float(T < trunc) * (w_occ - 1),  E = T >= trunc                       (the NORMALISED T against trunc, as the reference does)
    normals(v) = g / sqrt(|g|^2 + 1e-5),  g = the three Sobel stencils on v padded with trunc
    l1 = mean |p - (2 * (den(T) / trunc) - 1)| * W',  W' = W except 0 where E and df(p) >= trunc
    normal = 1 - mean over valid voxels of cos(normals(df(p)), normals(den(T))),  valid = both Sobel gradients non-zero
"""
import numpy as np
import torch
import torch.nn.functional as F


def load_fixture(golden_dir):
    z = np.load(golden_dir / 'shape_loss.npz')
    cases = {}
    for name in z['cases']:
        name = str(name)
        cases[name] = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + '_')}
    return cases


def stencils(dtype):
    s, d = torch.tensor([1., 2., 1.], dtype=dtype), torch.tensor([1., 0., -1.], dtype=dtype)
    outer = lambda a, b, c: a[:, None, None] * b[None, :, None] * c[None, None, :]
    return torch.stack([outer(d, s, s), outer(s, d, s), outer(s, s, -d)])[:, None]       # [3, 1, 3, 3, 3]: along D (+ - ), along H (+ -), along W (- +)


def sobel(v, pad):
    return F.conv3d(F.pad(v, (1,) * 6, value=pad), stencils(v.dtype))


def normals(v, trunc):
    g = sobel(v, trunc)
    return g / torch.sqrt((g * g).sum(1, keepdim=True) + 1e-5)


def augment(target, trunc, mean, std, w_occ):
    """-> weights, empty, normals of the denormalised target"""
    return 1 + (target < trunc).to(target.dtype) * (w_occ - 1), target >= trunc, normals(target * std + mean, trunc)


def loss(pred, target, trunc, mean, std, w_occ=8, lam_rec=1, lam_n=0.5):
    """differentiable in pred -> total, l1, normal, (valid count, empty-on-both-sides count)"""
    weights, empty, nt = augment(target, trunc, mean, std, w_occ)
    df = (pred + 1) * trunc / 2
    both = empty & (df >= trunc)
    l1 = ((pred - (2 * ((target * std + mean) / trunc) - 1)).abs() * torch.where(both, torch.zeros_like(weights), weights)).mean()
    g = sobel(df, trunc)
    valid = ((g != 0).any(1) & (nt != 0).any(1))
    gn = torch.where(valid[:, None], g, torch.ones_like(g))                # keep the division away from 0 / 0 where the voxel is masked anyway
    tn = torch.where(valid[:, None], nt, torch.ones_like(nt))
    cos = ((gn / gn.norm(dim=1, keepdim=True)) * (tn / tn.norm(dim=1, keepdim=True))).sum(1)
    normal = 1 - (cos * valid).sum() / valid.sum()
    return lam_rec * l1 + lam_n * normal, l1, normal, (int(valid.sum()), int(both.sum()))


def grad_by_formula(pred, target, trunc, mean, std, w_occ=8, a=1.0, b=0.5):
    """d (a * l1 + b * normal) / d pred written out: sign(p - t) W' / N for the L1 term; for the normal term d cos / d g = (t^ - g^ (g^ . t^)) / |g| on
    valid voxels over their count, pulled back through the transposed stencils (= the negated ones, zero padding) and d df / d p = trunc / 2."""
    weights, empty, nt = augment(target, trunc, mean, std, w_occ)
    df = (pred + 1) * trunc / 2
    both = empty & (df >= trunc)
    out = a * torch.sign(pred - (2 * ((target * std + mean) / trunc) - 1)) * torch.where(both, torch.zeros_like(weights), weights) / pred.numel()
    g = sobel(df, trunc)
    valid = ((g != 0).any(1) & (nt != 0).any(1))
    if int(valid.sum()) == 0:
        return out
    gn = torch.where(valid[:, None], g, torch.ones_like(g))
    tn = torch.where(valid[:, None], nt, torch.ones_like(nt))
    gl = gn.norm(dim=1, keepdim=True)
    gh, th = gn / gl, tn / tn.norm(dim=1, keepdim=True)
    dcos = torch.where(valid[:, None], (th - gh * (gh * th).sum(1, keepdim=True)) / gl, torch.zeros_like(g))
    pulled = sum(F.conv3d(F.pad(dcos[:, c:c + 1], (1,) * 6), stencils(pred.dtype)[c:c + 1]) for c in range(3))
    return out + b * (trunc / 2) / int(valid.sum()) * pulled


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def within(x_hip, x_ref32, x_f64, what=''):
    """The tolerance rule: err_hip <= max(2 * err_ref, 4 float32 ulps); for tensors max-abs errors, ulps of max |x_f64|.  Prints the figures first."""
    x_f64 = np.asarray(x_f64, np.float64)
    e_hip = float(np.abs(np.asarray(x_hip, np.float64) - x_f64).max())
    e_ref = float(np.abs(np.asarray(x_ref32, np.float64) - x_f64).max())
    floor = 4 * ulp32(np.abs(x_f64).max())
    print('%s: err_hip %.3e  err_ref %.3e  floor %.3e  (max |x| %.3e)' % (what, e_hip, e_ref, floor, np.abs(x_f64).max()))
    return e_hip <= max(2 * e_ref, floor)
