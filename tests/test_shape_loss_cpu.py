"""CPU: the shape loss's host side (rfuse/losses.py, include/rfuse_train.h; reference trainer/train_refinement.py:175-183, :231-253) -- the third
header's binding and its status rule, the other two tables untouched by it, the refusal of CPU input, and the reference-generated fixture
(tools/gen_shape_loss_golden.py) against the float64 restatement of tests/shape_loss_ref.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import shape_loss_ref as slr

REPO = Path(__file__).resolve().parents[1]
NAMES = {'rf_train_sobel_normals', 'rf_train_shape_loss', 'rf_train_shape_loss_backward', 'rf_train_shape_loss_ws_bytes'}


def declared(header):
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / header).read_text(), flags=re.S)
    return set(re.findall(r'\b(rf_[a-z0-9_]+)\s*\(', text))


def test_train_header_is_bound_and_exported():
    from rfuse import _lib
    assert declared('rfuse_train.h') == NAMES == set(_lib.TRAIN_SIGNATURES)
    lib = _lib.load_train()
    for n in NAMES:
        assert hasattr(lib, n), '%s declared in include/rfuse_train.h but not exported by librfuse_hip.so' % n
    assert lib is _lib.load_train() and lib._cdll is _lib.load()._cdll                      # one shared object
    assert ctypes.c_double not in {a for _, args, _ in _lib.TRAIN_SIGNATURES.values() for a in args}       # no double scalar
    assert all(params[-1] == 'stream' for n, (_, _, params) in _lib.TRAIN_SIGNATURES.items() if not n.endswith('_ws_bytes'))
    assert _lib.TRAIN_SIGNATURES['rf_train_shape_loss_ws_bytes'][0] is ctypes.c_size_t


def test_the_other_two_tables_are_unchanged_and_disjoint():
    from rfuse import _lib
    assert set(_lib.SIGNATURES) == declared('rfuse.h') and set(_lib.EVAL_SIGNATURES) == declared('rfuse_eval.h')
    assert not set(_lib.TRAIN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES))
    assert not any(n.startswith('rf_train_') for n in list(_lib.SIGNATURES) + list(_lib.EVAL_SIGNATURES))
    main, tr = _lib.load(), _lib.load_train()
    assert set(main._direct) == set(_lib.SIGNATURES) and set(tr._direct) == set(_lib.TRAIN_SIGNATURES)
    records = []
    main.start_profile(records)                      # the profiling wrapper covers rfuse.h only
    try:
        assert all(getattr(tr, n) is tr._direct[n] for n in _lib.TRAIN_SIGNATURES)
    finally:
        main.stop_profile()
    for header in ('rfuse.h', 'rfuse_eval.h'):
        assert 'rfuse_train.h' not in (REPO / 'include' / header).read_text()


def test_train_status_functions_raise_under_their_own_name():
    """refused arguments, before any device is touched"""
    from rfuse import _lib
    lib = _lib.load_train()
    status = {n for n in _lib.TRAIN_SIGNATURES if _lib.is_status(n, _lib.TRAIN_SIGNATURES)}
    assert status == NAMES - {'rf_train_shape_loss_ws_bytes'}
    assert {n for n, fn in lib._direct.items() if fn.errcheck is not None} == status
    one = ctypes.c_void_p(256)                       # a non-null pointer that the argument checks never follow
    big = 1 << 30
    with pytest.raises(RuntimeError, match=r'^rf_train_sobel_normals failed \(rc=-1\): .*bad arguments'):
        lib.rf_train_sobel_normals(None, 1, 4, 4, 4, 1.0, 0.0, 0.0, 0.0, 0.0, None, None, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_train_sobel_normals failed \(rc=-1\): .*bad arguments'):
        lib.rf_train_sobel_normals(one, 1, 4, 0, 4, 1.0, 0.0, 0.0, 0.0, 0.0, one, None, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_train_sobel_normals failed \(rc=-2\): .*2\^31 - 1'):
        lib.rf_train_sobel_normals(one, 1, 2048, 2048, 2048, 1.0, 0.0, 0.0, 0.0, 0.0, one, None, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_train_shape_loss failed \(rc=-1\): .*bad arguments'):
        lib.rf_train_shape_loss(None, None, None, None, None, 1, 4, 4, 4, 1.0, 0.0, 1.0, 1.0, 0.5, None, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match=r'^rf_train_shape_loss failed \(rc=-1\): .*come together'):
        lib.rf_train_shape_loss(one, one, one, one, one, 1, 4, 4, 4, 1.0, 0.0, 1.0, 1.0, 0.5, one, one, one, None, one, 1 << 20, None)
    with pytest.raises(RuntimeError, match=r'^rf_train_shape_loss failed \(rc=-2\): .*2\^31 - 1'):
        lib.rf_train_shape_loss(one, one, one, one, one, big, 64, 64, 64, 1.0, 0.0, 1.0, 1.0, 0.5, one, one, None, None, one, 1 << 20, None)
    with pytest.raises(RuntimeError, match=r'^rf_train_shape_loss failed \(rc=-4\): .*workspace of 16 bytes'):
        lib.rf_train_shape_loss(one, one, one, one, one, 4, 64, 64, 64, 1.0, 0.0, 1.0, 1.0, 0.5, one, one, None, None, one, 16, None)
    with pytest.raises(RuntimeError, match=r'^rf_train_shape_loss_backward failed \(rc=-1\): .*bad arguments'):
        lib.rf_train_shape_loss_backward(one, one, None, None, 1, 4, 4, 4, 1.0, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_train_shape_loss_backward failed \(rc=-2\): .*2\^31 - 1'):
        lib.rf_train_shape_loss_backward(one, one, one, one, 1, 1 << 20, 1 << 20, 1, 1.0, one, None)
    # the value function: 0 is an answer; one partial of 4 float64 per 8 x 8 x 32 tile, rounded up to 256 bytes
    assert lib.rf_train_shape_loss_ws_bytes(0, 4, 4, 4) == 0 and lib.rf_train_shape_loss_ws_bytes(1, 2048, 2048, 2048) == 0
    assert lib.rf_train_shape_loss_ws_bytes(big, 64, 64, 64) == 0
    assert lib.rf_train_shape_loss_ws_bytes(1, 1, 1, 1) == 256 and lib.rf_train_shape_loss_ws_bytes(32, 64, 64, 64) == 32 * 128 * 32
    assert lib.rf_train_shape_loss_ws_bytes(1, 9, 17, 33) == 2 * 3 * 2 * 32 + 128


def test_cpu_tensors_have_no_fallback():
    from rfuse.losses import ShapeLoss
    from rfuse import configs
    sl = ShapeLoss.from_config(configs.get_config('C1'))
    assert sl.target_trunc == 0.0625 and (sl.weight_occupied, sl.loss_reconstruction, sl.loss_normal) == (8, 1, 0.5)
    v = torch.rand(1, 1, 4, 4, 4)
    batch = {'target': v}
    for call in (lambda: sl.compute_normals(v), lambda: sl.augment_batch_data(batch),
                 lambda: sl.loss_shape(v, {'target': v, 'weights': v, 'empty': v > 0, 'normals': torch.rand(1, 3, 4, 4, 4)})):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    assert set(batch) == {'target'}
    with pytest.raises(RuntimeError, match='forward only'):
        sl.compute_normals(v.clone().requires_grad_(True))


def test_fixture_agrees_with_the_float64_restatement(golden_dir):
    """What the reference's functions returned (through the generator's stand-ins) is what the formulas give: masks and counts exactly, float32 values
    within float32 rounding of the float64 restatement, the float64 record to 1e-12, and the gradient also from the written-out formula."""
    cases = slr.load_fixture(golden_dir)
    assert list(cases) == ['sn16', 'odd', 'mp16', 'tiny', 'flat4', 'flat1']
    assert (golden_dir / 'shape_loss.npz').stat().st_size <= (golden_dir / 'mesh_metrics.npz').stat().st_size
    assert [cases[c]['target'].shape for c in cases] == [(2, 1, 16, 16, 16), (1, 1, 9, 17, 33), (2, 1, 16, 16, 16), (3, 1, 2, 3, 5), (1, 1, 4, 4, 4), (1, 1, 1, 1, 1)]
    for name, c in cases.items():
        trunc, mean, std, w_occ, lam_rec, lam_n = (float(x) for x in c['params'])
        target = torch.from_numpy(c['target']).double()
        pred = torch.from_numpy(c['pred']).double().requires_grad_(True)
        weights, empty, nt = slr.augment(target, trunc, mean, std, w_occ)
        np.testing.assert_array_equal(weights.numpy(), c['weights_f32'])
        np.testing.assert_array_equal(empty.numpy(), c['empty'])
        np.testing.assert_array_equal(nt.numpy() == 0, c['normals_f32'] == 0)
        np.testing.assert_allclose(nt.numpy(), c['normals_f64'], rtol=0, atol=1e-12)
        np.testing.assert_allclose(nt.numpy(), c['normals_f32'], rtol=0, atol=1e-6)
        total, l1, normal, counts = slr.loss(pred, target, trunc, mean, std, w_occ, lam_rec, lam_n)
        assert counts == tuple(int(x) for x in c['counts']), name
        degenerate = counts[0] == 0
        assert degenerate == name.startswith('flat')
        if not degenerate:
            assert 0.3 <= counts[0] / pred.numel() or name == 'tiny'
        np.testing.assert_allclose(l1.item(), c['scalars_f64'][1], rtol=1e-12)
        np.testing.assert_allclose(l1.item(), c['scalars_f32'][1], rtol=1e-6)
        if degenerate:
            assert np.isnan(c['scalars_f32'][[0, 2]]).all() and np.isnan(c['scalars_f64'][[0, 2]]).all() and np.isnan(normal.item())
            (lam_rec * l1).backward()
        else:
            np.testing.assert_allclose([total.item(), normal.item()], c['scalars_f64'][[0, 2]], rtol=1e-10)
            np.testing.assert_allclose([total.item(), normal.item()], c['scalars_f32'][[0, 2]], rtol=1e-5)
            total.backward()
        scale = np.abs(c['grad_f64']).max()
        assert np.isfinite(c['grad_f32']).all() and np.isfinite(c['grad_f64']).all()
        by_formula = slr.grad_by_formula(pred.detach(), target, trunc, mean, std, w_occ, lam_rec, lam_n).numpy()
        for got in (pred.grad.numpy(), by_formula):
            assert np.abs(got - c['grad_f64']).max() <= 1e-9 * scale, name
            assert np.abs(got - c['grad_f32']).max() <= 1e-4 * scale, name
        if name == 'sn16':
            assert ((c['pred'] == 2 * (c['target'] * np.float32(std) + np.float32(mean)) / np.float32(trunc) - 1) & (c['weights_f32'] == 8)).sum() > 100      # the subgradient at 0
            assert (c['grad_f32'] == 0).sum() > 100
