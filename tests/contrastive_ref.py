"""NT-Xent and the sliced attention contrastive loss restated from their formulas in plain torch (any dtype, float64 in the tests), independent of both
the reference's code and the kernels: used by tests/test_contrastive_cpu.py to check the fixture and by tests/test_contrastive_gpu.py as the float64 side
of the end-to-end tests.

    one group of n pairs, rows stacked [zjs; zis]:  w = z / max(|z|, 1e-8) (cosine) or z (dot),  s_ij = w_i . w_j,  pos(i) = (i + n) mod 2n
    l_ij = s_ij / tau_ij,  tau_ij = tau for the positive; for a negative tau, or tau + (1 - tau) sigmoid(iou_ij sig_scale + sig_shift)
    loss = (1 / 2n) sum_i (logsumexp_{j != i} l_ij - l_{i,pos(i)})
    sliced: split = N // num_slices; slice s is taken iff count_s > 0 and taken + count_s <= max_rows; the SUM of the taken groups' losses
"""
import numpy as np
import torch

from shape_loss_ref import ulp32, within      # noqa: F401  (the tolerance rule: err_hip <= max(2 * err_ref, 4 float32 ulps))


def load_fixture(golden_dir):
    """-> {case: {key: array}}; feature arrays and IoU matrices stored as float16 (exactly representable values) come back as float32"""
    z = np.load(golden_dir / 'contrastive_loss.npz')
    cases = {}
    for name in z['cases']:
        name = str(name)
        c = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + '_')}
        cases[name] = {k: v.astype(np.float32) if v.dtype == np.float16 else v for k, v in c.items()}
    return cases


def ntxent(zis, zjs, tau, cosine=True, iou=None, sig_scale=80, sig_shift=-65):
    n = zis.shape[0]
    z = torch.cat([zjs, zis], 0)
    w = z / z.norm(dim=1, keepdim=True).clamp_min(1e-8) if cosine else z
    s = w @ w.T
    idx = torch.arange(2 * n)
    pos = (idx + n) % (2 * n)
    t = torch.full_like(s, tau)
    if iou is not None:
        t = tau + (1 - tau) * torch.sigmoid(iou.to(s.dtype) * sig_scale + sig_shift)
        t[idx, pos] = tau
    logits = (s / t).masked_fill(torch.eye(2 * n, dtype=torch.bool), float('-inf'))
    return (torch.logsumexp(logits, 1) - logits[idx, pos]).sum() / (2 * n)


def select(occupancy, num_slices, max_rows=1280):
    """-> (the row indices of each taken group, in slice order; counts = occupied rows over all slices, selected rows, selected groups)"""
    occ = np.asarray(occupancy).reshape(-1) > 0
    split = occ.shape[0] // num_slices
    groups, taken, occupied = [], 0, 0
    for s in range(num_slices):
        rows = np.flatnonzero(occ[s * split:(s + 1) * split]) + s * split
        occupied += len(rows)
        if len(rows) > 0 and taken + len(rows) <= max_rows:
            groups.append(rows)
            taken += len(rows)
    return groups, (occupied, taken, len(groups))


def sliced(num_slices, fpred, ftgt, occupancy, tau=0.05, max_rows=1280):
    """-> (loss of shape (), counts); differentiable in fpred / ftgt"""
    groups, counts = select(occupancy.detach().cpu().numpy() if isinstance(occupancy, torch.Tensor) else occupancy, num_slices, max_rows)
    total = fpred.new_zeros(())
    for rows in groups:
        r = torch.from_numpy(rows).to(fpred.device)
        total = total + ntxent(fpred[r], ftgt[r], tau)
    return total, counts
