"""GPU: the loss kernels (csrc/ntxent.hip, csrc/shape_loss.hip behind rfuse/losses.py) on every tiling path, on the generated cases of tests/loss_cases.py:
NT-Xent with 65 to 256 features (two to four feature chunks, ragged last chunks, up to 128 row tiles and 38 column steps), the sliced loss at the trainer's
own geometry, with a partial second ballot word and with one group of 1200 pairs, and the shape loss on 260 partials (the second round of the finish loop),
on 3 x 3 x 3 tiles (an interior tile), ragged on all axes, and with many tiles along each single axis.  tests/test_loss_sweep_cpu.py checks what each case
reaches and that the float32 and float64 restatements agree on every mask entry, so that no voxel and no row is left out of a comparison here.

Tolerance rule (shape_loss_ref.within, as in tests/test_contrastive_gpu.py and tests/test_shape_loss_gpu.py): err_hip <= max(2 * err_ref, 4 float32 ulps), both
errors against the float64 restatement (tests/contrastive_ref.py, tests/shape_loss_ref.py), err_ref that of the same restatement evaluated in float32 on the
CPU; tensors by max-abs errors and ulps of max |x_f64|.  Counts, the selection, weights, empty masks and exact-zero patterns are compared exactly.
profiles/loss_sweep_errors.txt holds the figures of one MI355X."""
import numpy as np
import pytest
import torch

import loss_cases as lc
import shape_loss_ref as slr

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ contrastive loss
def run_single(name, dev):
    from rfuse.losses import NTXent
    r = lc.single_reference(name)
    n, dim, cosine, tau, _ = lc.SINGLE[name]
    ntx = NTXent(tau, cosine, lc.SIG_SCALE, lc.SIG_SHIFT)
    zis, zjs = (torch.from_numpy(r[k]).to(dev).requires_grad_(True) for k in ('zis', 'zjs'))
    loss = ntx(zis, zjs, None if r['iou'] is None else torch.from_numpy(r['iou']).to(dev))
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device == zis.device
    loss.backward()
    assert zis.grad.shape == zjs.grad.shape == (n, dim) and zis.grad.dtype == zjs.grad.dtype == torch.float32
    return loss.detach(), zis.grad, zjs.grad


def run_sliced(name, dev):
    from rfuse.losses import AttnContrastiveLoss
    r = lc.sliced_reference(name)
    rows, slices, dim, max_rows = lc.SLICED[name]
    acl = AttnContrastiveLoss(lc.SLICED_TAU, max_rows)
    fpred, ftgt = (torch.from_numpy(r[k]).to(dev).requires_grad_(True) for k in ('fpred', 'ftgt'))
    loss = acl(slices, fpred, ftgt, torch.from_numpy(r['occ']).to(dev))
    assert loss.shape == (1,) and loss.dtype == torch.float32
    loss.sum().backward()
    assert fpred.grad.shape == ftgt.grad.shape == (rows, dim) and fpred.grad.dtype == ftgt.grad.dtype == torch.float32
    return loss.detach(), fpred.grad, ftgt.grad, acl.last_counts


@pytest.mark.parametrize('name', list(lc.SINGLE))
def test_ntxent_above_64_features_and_over_many_tiles(gpu, name):
    r = lc.single_reference(name)
    loss, gi, gj = run_single(name, gpu)
    if name == 'w256n1':          # no negative: the loss and both gradients are exactly 0, through four chunks
        assert loss.item() == 0 and not gi.any() and not gj.any()
        return
    assert slr.within(loss.item(), r['loss_f32'], r['loss_f64'], name + ' loss')
    for g, k in ((gi, 'zis'), (gj, 'zjs')):
        g = g.cpu().numpy()
        assert slr.within(g, r['grad_%s_f32' % k], r['grad_%s_f64' % k], '%s grad_%s' % (name, k))
        if name == 'w100zero' and k == 'zis':         # the clamped row's gradient is 1e8 times the others': those on their own
            rest = [i for i in range(g.shape[0]) if i != lc.ZERO_ROW]
            assert slr.within(g[rest], r['grad_zis_f32'][rest], r['grad_zis_f64'][rest], 'w100zero grad_zis_other_rows')


@pytest.mark.parametrize('name', list(lc.SLICED))
def test_sliced_loss_at_the_trainers_geometry_and_beyond(gpu, name):
    r = lc.sliced_reference(name)
    loss, gp, gt, counts = run_sliced(name, gpu)
    np.testing.assert_array_equal(counts.cpu().numpy(), r['counts'])
    assert slr.within(loss.item(), r['loss_f32'], r['loss_f64'], name + ' loss')
    rows = r['rows']
    rest = np.setdiff1d(np.arange(lc.SLICED[name][0]), rows)
    assert len(rest) > 0
    for g, k in ((gp, 'fpred'), (gt, 'ftgt')):
        g = g.cpu().numpy()
        assert not g[rest].any(), 'a row that was not selected has a gradient'
        assert g[rows].any(1).all(), 'a selected row has no gradient'               # the selection itself, row by row
        assert slr.within(g[rows], r['grad_%s_f32' % k][rows], r['grad_%s_f64' % k][rows], '%s grad_%s' % (name, k))


# ------------------------------------------------------------------------------------------------ shape loss
def setup(shape_name, stats_name, dev, grad=True):
    from rfuse.losses import ShapeLoss
    r = lc.shape_reference(shape_name, stats_name)
    trunc, mean, std = r['params']
    sl = ShapeLoss(trunc, mean, std, weight_occupied=lc.W_OCC, loss_reconstruction=lc.LAM_REC, loss_normal=lc.LAM_N)
    batch = {'target': torch.from_numpy(r['target']).to(dev)}
    sl.augment_batch_data(batch)
    pred = torch.from_numpy(r['pred']).to(dev).requires_grad_(grad)
    return r, sl, batch, pred


@pytest.mark.parametrize('shape_name,stats_name', lc.SHAPE_CASES)
def test_augment_batch_data_on_every_tiling(gpu, shape_name, stats_name):
    r, sl, batch, _ = setup(shape_name, stats_name, gpu)
    what = '%s/%s' % (shape_name, stats_name)
    assert batch['weights'].dtype == torch.float32 and batch['empty'].dtype == torch.bool and batch['normals'].dtype == torch.float32
    assert batch['weights'].shape == batch['empty'].shape == batch['target'].shape and batch['normals'].shape == r['normals_f64'].shape
    np.testing.assert_array_equal(batch['weights'].cpu().numpy(), r['weights_f64'])
    np.testing.assert_array_equal(batch['empty'].cpu().numpy(), r['empty_f64'])
    normals = batch['normals'].cpu().numpy()
    np.testing.assert_array_equal(normals == 0, r['normals_f64'] == 0)
    assert slr.within(normals, r['normals_f32'], r['normals_f64'], what + ' normals')


@pytest.mark.parametrize('shape_name,stats_name', lc.SHAPE_CASES)
def test_loss_shape_scalars_counts_and_gradient_on_every_tiling(gpu, shape_name, stats_name):
    r, sl, batch, pred = setup(shape_name, stats_name, gpu)
    what = '%s/%s' % (shape_name, stats_name)
    total, l1, normal = sl.loss_shape(pred, batch)
    assert total.shape == l1.shape == normal.shape == () and total.dtype == torch.float32
    total.backward()
    np.testing.assert_array_equal(sl.last_counts.cpu().numpy(), r['counts'])
    for k, (v, label) in enumerate(((total, 'total'), (l1, 'l1'), (normal, 'normal'))):
        assert slr.within(v.item(), r['scalars_f32'][k], r['scalars_f64'][k], '%s %s' % (what, label))
    assert pred.grad.shape == pred.shape and pred.grad.dtype == torch.float32
    assert slr.within(pred.grad.cpu().numpy(), r['grad_f32'], r['grad_f64'], what + ' grad')


@pytest.mark.parametrize('shape_name,stats_name', [c for c in lc.SHAPE_CASES if c[0] in lc.FORMULA_SHAPES])
def test_upstream_gradient_of_total_plus_3_l1(gpu, shape_name, stats_name):
    """(total + 3 l1).backward() against the written-out gradient with a = 4, b = 0.5: both coefficients read from the device, over 260 samples and over an interior tile"""
    r, sl, batch, pred = setup(shape_name, stats_name, gpu)
    total, l1, normal = sl.loss_shape(pred, batch)
    (total + 3 * l1).backward()
    assert slr.within(pred.grad.cpu().numpy(), r['grad4_f32'], r['grad4_f64'], '%s/%s grad_total_plus_3_l1' % (shape_name, stats_name))


# ------------------------------------------------------------------------------------------------ the same bits on every call
def test_two_calls_give_identical_bits_on_the_new_reduction_rounds(gpu):
    """w200iou: four feature chunks and five column steps behind every sum; the 260-sample shape loss: the second round of the finish loop"""
    first, second = (torch.cat([o.reshape(-1) for o in run_single('w200iou', gpu)]) for _ in range(2))
    assert torch.equal(first, second)

    def shape_once():
        r, sl, batch, pred = setup('b260', 'C1', gpu)
        total, l1, normal = sl.loss_shape(pred, batch)
        total.backward()
        return torch.cat([torch.stack([total.detach(), l1.detach(), normal.detach()]), sl.last_counts.float(), pred.grad.reshape(-1), batch['normals'].reshape(-1)])
    first, second = shape_once(), shape_once()
    assert torch.isfinite(first).all() and torch.equal(first, second)
