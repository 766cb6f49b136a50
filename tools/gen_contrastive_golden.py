"""Fixture generator for the contrastive loss (CPU; needs the reference checkout, as tools/gen_shape_loss_golden.py does): runs the reference's own
``NTXentLoss.forward`` (model/loss.py:48-69) and ``RefinementTrainingModule.compute_sliced_attn_nt_xent_loss`` (trainer/train_refinement.py:208-221) as
written, in float32 and again in float64, with the loss and the gradients of both feature tensors, and writes tests/golden/contrastive_loss.npz (arrays only).

    python tools/gen_contrastive_golden.py

The trainer's method is called unbound on a ``types.SimpleNamespace`` (``log`` stubbed, ``loss_ntxent`` the reference's NTXentLoss); ``Tensor.cuda`` is mapped
to ``Tensor.to`` for the call, as oracle/gen_golden.py does.  Two things the method cannot give as it stands:
  * its row cap is the literal 1280.  Case ``cap20`` needs 20: the method's own source is compiled again with that one literal replaced.
  * in a float64 run ``zeros(1, float32) + loss64`` rounds the accumulator to float32 (the dimensioned tensor wins the promotion).  The float64 record is
    therefore the float64 sum, made here, of the reference's ``forward`` over the slices the method takes (the same greedy rule, tests/contrastive_ref.select);
    the float32 run of the method itself must select exactly those rows (asserted on its gradient).

Cases, each aimed at one way to go wrong:
    n1  n = 1: no negative, loss 0 and gradient 0          n2  n = 2, dim 5               n67  n = 67, dim 32: a ragged tile
    iou96  n = 96, dim 64, a random non-symmetric IoU matrix;  iou96sym  the symmetric repeat(2, 2) one of get_iou_matrix
    dot30  dot mode, rows scaled by 30                      zero  cosine, one all-zero row: the eps clamp
    cap20  16 slices of 8 rows, empty slices, max_rows = 20: one slice skipped for the cap, a later one taken
    ragged  50 rows in 4 slices: the last two rows belong to no slice          empty  every slice empty
    trainer  8 slices of 512 rows, dim 32, max_rows = 1280, tau = 0.05: a full slice of 512 pairs and a small one (rows of the other slices are zeros, and
                 the gradients are stored for the selected rows only: the file has to stay under the size limit of a committed file)

Layout: ``cases`` (names); per case ``<case>_params`` float64 = (tau, cosine, sig_scale, sig_shift) or (tau, num_slices, max_rows); features ``_zis`` / ``_zjs``
or ``_fpred`` / ``_ftgt`` (+ ``_occ`` uint8, ``_rows`` int32 = the selected rows in order, ``_counts`` int64 [3]); ``_iou``; per precision p in (f32, f64)
``_loss_p`` and ``_grad_<tensor>_p`` (sliced cases: the selected rows' gradients [len(rows), dim]; every other row's gradient is zero, asserted here).  Feature
and IoU values are multiples of 1 / 1024 in [-1, 1] and stored as float16 where that is exact.  The two views of a pair differ by clipped noise of 0.25 to 1.5 times
the range: with closer pairs the loss at tau = 0.05 is of the order 1e-6, and the float32 reference's own relative error of the order 1e-2.
"""
import inspect
import sys
import textwrap
import types
from pathlib import Path
from unittest import mock

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
from oracle.gen_golden import REF, save_fixture                 # noqa: E402
from tools.gen_shape_loss_golden import import_reference_trainer      # noqa: E402
import contrastive_ref as cr                                    # noqa: E402

LIMIT = 1 << 20


def grid(rng, shape):
    return (rng.integers(-1024, 1025, shape) / 1024.0).astype(np.float32)


def pairs(rng, n, dim, noise=0.25):
    zjs = grid(rng, (n, dim))
    zis = np.round((zjs + noise * grid(rng, (n, dim))).clip(-1, 1) * 1024) / 1024
    return zis.astype(np.float32), zjs


def compact(a):
    return a.astype(np.float16) if np.array_equal(a.astype(np.float16).astype(np.float32), a) else a


def run_single(NTXentLoss, zis, zjs, iou, tau, cosine, dtype):
    crit = NTXentLoss(tau, cosine)
    zi, zj = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (zis, zjs))
    loss = crit(zi, zj, None if iou is None else torch.from_numpy(iou).to(dtype))
    loss.backward()
    return loss.detach().numpy(), zi.grad.numpy(), zj.grad.numpy()


def sliced_method(Module, max_rows):
    src = textwrap.dedent(inspect.getsource(Module.compute_sliced_attn_nt_xent_loss))
    assert src.count('<= 1280') == 1, 'the reference method changed'
    if max_rows == 1280:
        return Module.compute_sliced_attn_nt_xent_loss
    ns = {'torch': torch}
    exec(compile(src.replace('<= 1280', '<= %d' % max_rows), 'compute_sliced_attn_nt_xent_loss (cap %d)' % max_rows, 'exec'), ns)
    return ns['compute_sliced_attn_nt_xent_loss']


def run_sliced(Module, NTXentLoss, fpred, ftgt, occ, num_slices, tau, max_rows):
    logged = []
    mod = types.SimpleNamespace(log=lambda name, value, **kw: logged.append(value), loss_ntxent=NTXentLoss(tau, True))
    fp, ft = (torch.from_numpy(a).requires_grad_(True) for a in (fpred, ftgt))
    loss32 = sliced_method(Module, max_rows)(mod, num_slices, fp, ft, torch.from_numpy(occ))
    assert loss32.shape == (1,) and loss32.dtype == torch.float32
    if loss32.requires_grad:
        loss32.sum().backward()
    g32 = [np.zeros_like(fpred) if t.grad is None else t.grad.numpy() for t in (fp, ft)]
    groups, counts = cr.select(occ, num_slices, max_rows)
    fp64, ft64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (fpred, ftgt))
    loss64 = torch.zeros((), dtype=torch.float64)
    for rows in groups:
        r = torch.from_numpy(rows)
        loss64 = loss64 + mod.loss_ntxent(fp64[r], ft64[r])
    if groups:
        loss64.backward()
    g64 = [np.zeros(fpred.shape, np.float64) if t.grad is None else t.grad.numpy() for t in (fp64, ft64)]
    rows = np.concatenate(groups).astype(np.int32) if groups else np.zeros(0, np.int32)
    rest = np.setdiff1d(np.arange(fpred.shape[0]), rows)
    for g in g32 + g64:
        assert not g[rest].any(), 'a row that was not selected has a gradient'
    if all(len(r) > 1 for r in groups):          # (a group of one pair has a zero gradient)
        assert np.array_equal(np.flatnonzero(np.abs(g32[0]).sum(1) > 0), np.sort(rows)), 'the float32 run of the method selected other rows'
    assert logged == [counts[0] + int((occ[num_slices * (len(occ) // num_slices):] > 0).sum())]       # the method logs the occupancy of ALL rows
    return loss32.detach().numpy()[0], loss64.detach().numpy(), g32, g64, rows, np.array(counts, np.int64), groups


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def main():
    Module, _ = import_reference_trainer()
    import model.loss as ref_loss
    assert str(REF) in ref_loss.__file__, ref_loss.__file__
    NTXentLoss = ref_loss.NTXentLoss
    rng = np.random.default_rng(2026)
    out, names = {}, []

    def single(name, zis, zjs, tau, cosine=True, iou=None):
        names.append(name)
        with mock.patch.object(torch.Tensor, 'cuda', lambda self, device=None, **kw: self.to(device)):
            l32, gi32, gj32 = run_single(NTXentLoss, zis, zjs, iou, tau, cosine, torch.float32)
            l64, gi64, gj64 = run_single(NTXentLoss, zis, zjs, iou, tau, cosine, torch.float64)
        out[name + '_params'] = np.array([tau, float(cosine), 80, -65], np.float64)
        out[name + '_zis'], out[name + '_zjs'] = compact(zis), compact(zjs)
        if iou is not None:
            out[name + '_iou'] = compact(iou)
        for tag, l, gi, gj in (('f32', l32, gi32, gj32), ('f64', l64, gi64, gj64)):
            out['%s_loss_%s' % (name, tag)], out['%s_grad_zis_%s' % (name, tag)], out['%s_grad_zjs_%s' % (name, tag)] = np.asarray(l), gi, gj
        print('%-9s n %4d dim %3d  loss %.9g   err_ref: loss %.3e (relative)  grad zis %.3e  zjs %.3e (max-abs / max|f64|)' % (
            name, zis.shape[0], zis.shape[1], float(l64), abs(float(l32) - float(l64)) / max(abs(float(l64)), 1e-300), rel(gi32, gi64), rel(gj32, gj64)))
        return float(l64), gi64

    def sliced(name, fpred, ftgt, occ, num_slices, tau, max_rows=1280):
        names.append(name)
        with mock.patch.object(torch.Tensor, 'cuda', lambda self, device=None, **kw: self.to(device)):
            l32, l64, g32, g64, rows, counts, groups = run_sliced(Module, NTXentLoss, fpred, ftgt, occ, num_slices, tau, max_rows)
        out[name + '_params'] = np.array([tau, num_slices, max_rows], np.float64)
        out[name + '_fpred'], out[name + '_ftgt'], out[name + '_occ'] = compact(fpred), compact(ftgt), occ
        out[name + '_rows'], out[name + '_counts'] = rows, counts
        for tag, l, g in (('f32', l32, g32), ('f64', l64, g64)):
            out['%s_loss_%s' % (name, tag)] = np.asarray(l)
            out['%s_grad_fpred_%s' % (name, tag)], out['%s_grad_ftgt_%s' % (name, tag)] = g[0][rows], g[1][rows]
        print('%-9s N %4d dim %3d slices %2d cap %4d  counts %s groups %s  loss %.9g   err_ref: loss %.3e  grad fpred %.3e  ftgt %.3e' % (
            name, fpred.shape[0], fpred.shape[1], num_slices, max_rows, counts.tolist(), [len(g) for g in groups], float(l64),
            abs(float(l32) - float(l64)) / max(abs(float(l64)), 1e-300), rel(g32[0], g64[0]) if len(rows) else 0.0, rel(g32[1], g64[1]) if len(rows) else 0.0))
        return groups, counts

    l, g = single('n1', *pairs(rng, 1, 4), 0.5)
    assert l == 0.0 and not g.any()
    single('n2', *pairs(rng, 2, 5), 0.5)
    single('n67', *pairs(rng, 67, 32, 1.0), 0.07)
    zis, zjs = pairs(rng, 96, 64)
    single('iou96', zis, zjs, 0.2, iou=grid(rng, (192, 192)) * 0.5 + 0.5)
    half = grid(rng, (96, 96)) * 0.5 + 0.5
    half = np.maximum(half, half.T)
    np.fill_diagonal(half, 1.0)
    single('iou96sym', zis, zjs, 0.2, iou=np.tile(half, (2, 2)))
    # independent rows: the positive is one logit among the others, and the logits are of the order of thousands
    l, g = single('dot30', 30 * grid(rng, (8, 16)), 30 * grid(rng, (8, 16)), 0.5, cosine=False)
    assert l > 100 and g.any()
    zis, zjs = pairs(rng, 5, 8)
    zis[3] = 0
    l, g = single('zero', zis, zjs, 0.5)
    print('          gradient of the all-zero row: max |.| %.3e, of the others %.3e' % (np.abs(g[3]).max(), np.abs(np.delete(g, 3, 0)).max()))

    # cap20: occupied rows per slice; 6 + 7 + 5 = 18, the 8 of slice 4 do not fit, the 2 of slice 5 do, nothing after that fits
    want = [6, 0, 7, 5, 8, 2, 0, 3, 1, 0, 8, 4, 0, 0, 2, 5]
    occ = np.zeros(128, np.uint8)
    for s, c in enumerate(want):
        occ[s * 8 + rng.permutation(8)[:c]] = 1
    groups, counts = sliced('cap20', *pairs(rng, 128, 32, 1.5), occ, 16, 0.05, max_rows=20)
    assert [len(g) for g in groups] == [6, 7, 5, 2] and [int(g[0]) // 8 for g in groups] == [0, 2, 3, 5] and counts.tolist() == [sum(want), 20, 4]
    occ = (rng.random(50) < 0.6).astype(np.uint8)
    occ[48:] = 1
    groups, counts = sliced('ragged', *pairs(rng, 50, 7, 1.5), occ, 4, 0.05)
    assert len(groups) == 4 and counts[0] == occ[:48].sum() == counts[1]
    groups, counts = sliced('empty', *pairs(rng, 32, 32), np.zeros(32, np.uint8), 4, 0.05)
    assert counts.tolist() == [0, 0, 0] and out['empty_loss_f32'] == 0
    occ = np.zeros(8 * 512, np.uint8)
    occ[:512] = 1
    occ[3 * 512 + rng.permutation(512)[:24]] = 1
    fpred, ftgt = pairs(rng, 8 * 512, 32, 1.5)
    fpred[occ == 0], ftgt[occ == 0] = 0, 0
    groups, counts = sliced('trainer', fpred, ftgt, occ, 8, 0.05)
    assert [len(g) for g in groups] == [512, 24]

    out['cases'] = np.array(names)
    save_fixture('contrastive_loss', **out)
    size = (REPO / 'tests' / 'golden' / 'contrastive_loss.npz').stat().st_size
    print('tests/golden/contrastive_loss.npz: %d bytes' % size)
    assert size <= LIMIT


if __name__ == '__main__':
    main()
