"""CPU: the contrastive loss's host side (rfuse/losses.py NTXent / AttnContrastiveLoss, include/rfuse_contrastive.h; reference model/loss.py:48-69,
trainer/train_refinement.py:208-221) -- the fourth header's binding and its status rule, the other three tables untouched by it, the refusal of CPU input,
and the reference-generated fixture (tools/gen_contrastive_golden.py) against the float64 restatement of tests/contrastive_ref.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import contrastive_ref as cr

REPO = Path(__file__).resolve().parents[1]
NAMES = {'rf_ntx_ws_bytes', 'rf_ntx_plan', 'rf_ntx_forward', 'rf_ntx_backward'}
CASES = ['n1', 'n2', 'n67', 'iou96', 'iou96sym', 'dot30', 'zero', 'cap20', 'ragged', 'empty', 'trainer']


def declared(header):
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / header).read_text(), flags=re.S)
    return set(re.findall(r'\b(rf_[a-z0-9_]+)\s*\(', text))


def test_contrastive_header_is_bound_and_exported():
    from rfuse import _lib
    assert declared('rfuse_contrastive.h') == NAMES == set(_lib.CONTRASTIVE_SIGNATURES)
    lib = _lib.load_contrastive()
    for n in NAMES:
        assert hasattr(lib, n), '%s declared in include/rfuse_contrastive.h but not exported by librfuse_hip.so' % n
    assert lib is _lib.load_contrastive() and lib._cdll is _lib.load()._cdll                      # one shared object
    assert ctypes.c_double not in {a for _, args, _ in _lib.CONTRASTIVE_SIGNATURES.values() for a in args}       # no double scalar
    assert all(params[-1] == 'stream' for n, (_, _, params) in _lib.CONTRASTIVE_SIGNATURES.items() if not n.endswith('_ws_bytes'))
    assert _lib.CONTRASTIVE_SIGNATURES['rf_ntx_ws_bytes'][0] is ctypes.c_size_t


def test_the_four_tables_are_disjoint_and_the_other_three_unchanged():
    from rfuse import _lib
    tables = {'rfuse.h': _lib.SIGNATURES, 'rfuse_eval.h': _lib.EVAL_SIGNATURES, 'rfuse_train.h': _lib.TRAIN_SIGNATURES,
              'rfuse_contrastive.h': _lib.CONTRASTIVE_SIGNATURES}
    for header, table in tables.items():
        assert set(table) == declared(header)
    names = [n for t in tables.values() for n in t]
    assert len(names) == len(set(names))
    assert [n for n in names if n.startswith('rf_ntx_')] == list(_lib.CONTRASTIVE_SIGNATURES)
    main, ntx = _lib.load(), _lib.load_contrastive()
    assert set(main._direct) == set(_lib.SIGNATURES) and set(_lib.load_eval()._direct) == set(_lib.EVAL_SIGNATURES)
    assert set(_lib.load_train()._direct) == set(_lib.TRAIN_SIGNATURES) and set(ntx._direct) == set(_lib.CONTRASTIVE_SIGNATURES)
    records = []
    main.start_profile(records)                      # the profiling wrapper covers rfuse.h only
    try:
        assert all(getattr(ntx, n) is ntx._direct[n] for n in _lib.CONTRASTIVE_SIGNATURES)
    finally:
        main.stop_profile()
    for header in ('rfuse.h', 'rfuse_eval.h', 'rfuse_train.h'):
        assert 'rfuse_contrastive.h' not in (REPO / 'include' / header).read_text()


def test_contrastive_status_functions_raise_under_their_own_name():
    """refused arguments, before any device is touched"""
    from rfuse import _lib
    lib = _lib.load_contrastive()
    status = {n for n in _lib.CONTRASTIVE_SIGNATURES if _lib.is_status(n, _lib.CONTRASTIVE_SIGNATURES)}
    assert status == NAMES - {'rf_ntx_ws_bytes'}
    assert {n for n, fn in lib._direct.items() if fn.errcheck is not None} == status
    one = ctypes.c_void_p(256)                       # a non-null pointer that the argument checks never follow
    big = 1 << 24
    # null pointers and non-positive sizes
    with pytest.raises(RuntimeError, match=r'^rf_ntx_plan failed \(rc=-1\): .*bad arguments'):
        lib.rf_ntx_plan(None, 64, 1, 64, 32, None, big, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_ntx_plan failed \(rc=-1\): .*bad arguments'):
        lib.rf_ntx_plan(one, 64, 0, 64, 32, one, big, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_ntx_forward failed \(rc=-1\): .*bad arguments'):
        lib.rf_ntx_forward(None, one, None, 64, 1, 64, 32, 1, 0.05, 80.0, -65.0, one, big, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_ntx_forward failed \(rc=-1\): .*one slice'):
        lib.rf_ntx_forward(one, one, one, 64, 2, 64, 32, 1, 0.05, 80.0, -65.0, one, big, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_ntx_backward failed \(rc=-1\): .*bad arguments'):
        lib.rf_ntx_backward(None, None, 64, 1, 64, 32, 1, 0.05, 80.0, -65.0, one, big, one, one, None)
    # the group size (min(rows // slices, max_rows)) and the feature count out of range
    for call, args in (('rf_ntx_plan', lambda n, s, m, d, ws=big: (one, n, s, m, d, one, ws, one, None)),
                       ('rf_ntx_forward', lambda n, s, m, d, ws=big: (one, one, None, n, s, m, d, 1, 0.05, 80.0, -65.0, one, ws, one, None)),
                       ('rf_ntx_backward', lambda n, s, m, d, ws=big: (None, one, n, s, m, d, 1, 0.05, 80.0, -65.0, one, ws, one, one, None))):
        for n, s, m, d in ((4097, 1, 4097, 32), (64, 1, 64, 257), (3, 4, 1280, 32), (8192, 4097, 1280, 32)):
            with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-2\): .*features <= 256' % call):
                getattr(lib, call)(*args(n, s, m, d))
        with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-4\): .*workspace of 16 bytes' % call):
            getattr(lib, call)(*args(64, 1, 64, 32, 16))
    # the value function: 0 is an answer
    assert lib.rf_ntx_ws_bytes(0, 1, 1, 1) == 0 and lib.rf_ntx_ws_bytes(4097, 1, 4097, 32) == 0 and lib.rf_ntx_ws_bytes(64, 1, 64, 257) == 0
    assert lib.rf_ntx_ws_bytes(3, 4, 1280, 32) == 0 and lib.rf_ntx_ws_bytes(8192, 4097, 1280, 32) == 0
    # a long slice is fine as long as max_rows bounds the group; the stacked float64 rows dominate the size
    assert lib.rf_ntx_ws_bytes(1 << 20, 2, 1280, 32) > 0
    n = lib.rf_ntx_ws_bytes(4096, 8, 1280, 32)
    # header 256, row list 1280 * 4, 160 + 8 tiles of 16 bytes (rounded up to 256), a flag per row, float64 [2][1280][32] and three float64 [2][1280]
    assert n == 256 + 5120 + 2816 + 4096 + 655360 + 3 * 20480


def test_cpu_tensors_have_no_fallback():
    from rfuse.losses import NTXent, AttnContrastiveLoss
    z = torch.rand(8, 32)
    ntx, acl = NTXent(0.2), AttnContrastiveLoss()
    assert (ntx.temperature, ntx.use_cosine_similarity, ntx.sig_scale, ntx.sig_shift) == (0.2, True, 80, -65)
    assert (acl.temperature, acl.max_rows, acl.last_counts) == (0.05, 1280, None)
    for call in (lambda: ntx(z, z), lambda: ntx(z, z, torch.rand(16, 16)), lambda: acl(2, z, z, torch.ones(8))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    assert acl.last_counts is None


def test_fixture_agrees_with_the_float64_restatement(golden_dir):
    """What the reference's functions returned (through the generator's stand-ins) is what the formulas give: the float64 record to 1e-12, the float32 one
    within float32 rounding, the selection exactly."""
    cases = cr.load_fixture(golden_dir)
    assert list(cases) == CASES
    assert (golden_dir / 'contrastive_loss.npz').stat().st_size <= 1 << 20
    for name, c in cases.items():
        sliced = 'occ' in c
        a, b = ('fpred', 'ftgt') if sliced else ('zis', 'zjs')
        assert c[a].dtype == c[b].dtype == np.float32
        x, y = (torch.from_numpy(c[k]).double().requires_grad_(True) for k in (a, b))
        if sliced:
            tau, num_slices, max_rows = float(c['params'][0]), int(c['params'][1]), int(c['params'][2])
            loss, counts = cr.sliced(num_slices, x, y, c['occ'], tau, max_rows)
            groups, _ = cr.select(c['occ'], num_slices, max_rows)
            assert counts == tuple(int(v) for v in c['counts']), name
            np.testing.assert_array_equal(np.concatenate(groups) if groups else np.zeros(0), c['rows'])
        else:
            tau, cosine, sig_scale, sig_shift = (float(v) for v in c['params'])
            iou = torch.from_numpy(c['iou']).double() if 'iou' in c else None
            loss = cr.ntxent(x, y, tau, bool(cosine), iou, sig_scale, sig_shift)
        np.testing.assert_allclose(loss.item(), c['loss_f64'], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(loss.item(), c['loss_f32'], rtol=1e-5, atol=1e-7)
        if loss.requires_grad:
            loss.backward()
        for t, k in ((x, a), (y, b)):
            g = np.zeros(t.shape) if t.grad is None else t.grad.numpy()
            if sliced:
                rest = np.setdiff1d(np.arange(g.shape[0]), c['rows'])
                assert not g[rest].any()
                g = g[c['rows']]
            g64, g32 = c['grad_%s_f64' % k], c['grad_%s_f32' % k]
            assert g64.dtype == np.float64 and g32.dtype == np.float32 and g.shape == g64.shape == g32.shape
            scale = max(np.abs(g64).max(), 1e-300) if g64.size else 1.0
            if g64.size:
                assert np.abs(g - g64).max() <= 1e-9 * scale, name
                assert np.abs(g - g32).max() <= 1e-4 * scale, name
    # what each case is there for
    assert cases['n1']['loss_f64'] == 0 and not cases['n1']['grad_zis_f64'].any() and not cases['n1']['grad_zjs_f32'].any()
    assert cases['dot30']['loss_f64'] > 100 and cases['dot30']['params'][1] == 0 and np.abs(cases['dot30']['zis']).max() > 25
    assert not cases['zero']['zis'][3].any() and np.abs(cases['zero']['grad_zis_f64'][3]).max() > 1e6       # d (z / 1e-8) / d z
    assert not np.array_equal(cases['iou96']['iou'], cases['iou96']['iou'].T) and np.array_equal(cases['iou96sym']['iou'], cases['iou96sym']['iou'].T)
    assert np.array_equal(cases['iou96sym']['iou'][:96, :96], cases['iou96sym']['iou'][96:, 96:])
    assert cases['empty']['counts'].tolist() == [0, 0, 0] and cases['empty']['loss_f32'] == 0 and cases['empty']['rows'].size == 0
    assert cases['ragged']['occ'][48:].all() and cases['ragged']['rows'].max() < 48
    assert cases['trainer']['fpred'].shape == (4096, 32) and cases['trainer']['params'].tolist() == [0.05, 8, 1280]


def test_the_cap_case_skips_a_slice_and_takes_a_later_one(golden_dir):
    """cap20: 16 slices of 8 rows, max_rows = 20.  6 + 7 + 5 = 18 rows are taken, the 8 of slice 4 do not fit, the 2 of slice 5 do; the generator asserts it."""
    c = cr.load_fixture(golden_dir)['cap20']
    per_slice = c['occ'].reshape(16, 8).sum(1).tolist()
    assert per_slice[:6] == [6, 0, 7, 5, 8, 2] and sum(per_slice) == c['counts'][0] > 20
    groups, counts = cr.select(c['occ'], 16, 20)
    assert [int(g[0]) // 8 for g in groups] == [0, 2, 3, 5] and counts[1:] == (20, 4)
    src = (REPO / 'tools' / 'gen_contrastive_golden.py').read_text()
    assert "assert [len(g) for g in groups] == [6, 7, 5, 2] and [int(g[0]) // 8 for g in groups] == [0, 2, 3, 5]" in src
