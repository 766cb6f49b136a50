"""CPU: the host side of the retrieval trainer's IoU matrix (rfuse/losses.py iou_matrix / target_iou_matrix / RetrievalStepLoss, include/rfuse_pairs.h;
reference util/misc.py:51-59, trainer/train_retrieval.py:77-88) -- the fifth header's binding and its status rule, the other four tables untouched by it,
the refusals of the Python entry points, and the reference-generated fixture (tools/gen_iou_matrix_golden.py) against the count formula of
tests/iou_matrix_ref.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import iou_matrix_ref as ir

REPO = Path(__file__).resolve().parents[1]
NAMES = {'rf_iou_ws_bytes', 'rf_iou_pack', 'rf_iou_matrix'}
OTHERS = ('rfuse.h', 'rfuse_eval.h', 'rfuse_train.h', 'rfuse_contrastive.h')


def declared(header):
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / header).read_text(), flags=re.S)
    return set(re.findall(r'\b(rf_[a-z0-9_]+)\s*\(', text))


def test_pairs_header_is_bound_and_exported():
    from rfuse import _lib
    assert declared('rfuse_pairs.h') == NAMES == set(_lib.PAIRS_SIGNATURES)
    lib = _lib.load_pairs()
    for n in NAMES:
        assert hasattr(lib, n), '%s declared in include/rfuse_pairs.h but not exported by librfuse_hip.so' % n
    assert lib is _lib.load_pairs() and lib._cdll is _lib.load()._cdll                      # one shared object
    assert ctypes.c_double not in {a for _, args, _ in _lib.PAIRS_SIGNATURES.values() for a in args}       # no double scalar
    assert all(params[-1] == 'stream' for n, (_, _, params) in _lib.PAIRS_SIGNATURES.items() if not n.endswith('_ws_bytes'))
    assert _lib.PAIRS_SIGNATURES['rf_iou_ws_bytes'][0] is ctypes.c_size_t
    assert 'extern "C"' in (REPO / 'include' / 'rfuse_pairs.h').read_text()


def test_the_five_tables_are_disjoint_and_the_other_four_do_not_know_the_fifth():
    from rfuse import _lib
    tables = {'rfuse.h': _lib.SIGNATURES, 'rfuse_eval.h': _lib.EVAL_SIGNATURES, 'rfuse_train.h': _lib.TRAIN_SIGNATURES,
              'rfuse_contrastive.h': _lib.CONTRASTIVE_SIGNATURES, 'rfuse_pairs.h': _lib.PAIRS_SIGNATURES}
    for header, table in tables.items():
        assert set(table) == declared(header)
    names = [n for t in tables.values() for n in t]
    assert len(names) == len(set(names))
    assert [n for n in names if n.startswith('rf_iou')] == list(_lib.PAIRS_SIGNATURES)
    assert all(n.startswith('rf_iou_') for n in _lib.PAIRS_SIGNATURES)
    assert not [n for n in _lib.PAIRS_SIGNATURES if any(p in n for p in ('rf_ntx_', 'rf_train_', 'rf_eval_'))]
    assert set(_lib.load_pairs()._direct) == set(_lib.PAIRS_SIGNATURES)
    for header in OTHERS:
        assert 'rfuse_pairs' not in (REPO / 'include' / header).read_text()
    build_py = (REPO / 'retrieval-fuse_amd' / 'csrc' / 'build.py').read_text()
    assert "'iou_matrix.hip'" in build_py and "'iou_matrix.hip': ['-ffp-contract=off']" in build_py and "'rfuse_pairs.h'" in build_py


def test_pairs_status_functions_raise_under_their_own_name():
    """refused arguments, before any device is touched"""
    from rfuse import _lib
    lib = _lib.load_pairs()
    status = {n for n in _lib.PAIRS_SIGNATURES if _lib.is_status(n, _lib.PAIRS_SIGNATURES)}
    assert status == NAMES - {'rf_iou_ws_bytes'}
    assert {n for n, fn in lib._direct.items() if fn.errcheck is not None} == status
    one = ctypes.c_void_p(256)                       # a non-null pointer that the argument checks never follow
    v = 32 ** 3
    # null pointers and non-positive sizes
    for args in ((None, 0, 0.0, 0.0, 0.0, 4, v, one, one, None), (one, 0, 0.0, 0.0, 0.0, 4, v, None, one, None), (one, 0, 0.0, 0.0, 0.0, 4, v, one, None, None),
                 (one, 0, 0.0, 0.0, 0.0, 0, v, one, one, None), (one, 0, 0.0, 0.0, 0.0, 4, 0, one, one, None), (one, 2, 0.0, 0.0, 0.0, 4, v, one, one, None)):
        with pytest.raises(RuntimeError, match=r'^rf_iou_pack failed \(rc=-1\): .*bad arguments'):
            lib.rf_iou_pack(*args)
    for args in ((None, one, 4, None, None, 4, v, 1, one, None), (one, None, 4, None, None, 4, v, 1, one, None), (one, one, 4, None, None, 4, v, 1, None, None),
                 (one, one, 0, None, None, 0, v, 1, one, None), (one, one, 4, one, one, -1, v, 1, one, None), (one, one, 4, None, None, 4, 0, 1, one, None),
                 (one, one, 4, None, None, 4, v, 0, one, None)):
        with pytest.raises(RuntimeError, match=r'^rf_iou_matrix failed \(rc=-1\): .*bad arguments'):
            lib.rf_iou_matrix(*args)
    with pytest.raises(RuntimeError, match=r'^rf_iou_matrix failed \(rc=-1\): .*b needs its counts'):
        lib.rf_iou_matrix(one, one, 4, one, None, 4, v, 1, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_iou_matrix failed \(rc=-1\): .*n_b = n_a'):
        lib.rf_iou_matrix(one, one, 4, None, None, 5, v, 1, one, None)
    # outside the supported range: the message carries it
    rng = r'1 <= samples <= 8192, 1 <= voxels <= 2\^24, repeat 1 or 2'
    for n, vox in ((8193, v), (4, (1 << 24) + 1)):
        with pytest.raises(RuntimeError, match=r'^rf_iou_pack failed \(rc=-2\): .*' + rng):
            lib.rf_iou_pack(one, 1, 1.0, 0.0, 0.0, n, vox, one, one, None)
    for n_a, n_b, vox, rep in ((8193, 8193, v, 1), (4, 8193, v, 1), (4, 4, (1 << 24) + 1, 1), (4, 4, v, 3)):
        with pytest.raises(RuntimeError, match=r'^rf_iou_matrix failed \(rc=-2\): .*' + rng):
            lib.rf_iou_matrix(one, one, n_a, one, one, n_b, vox, rep, one, None)
    # the value function: 0 is an answer
    for n_a, n_b, vox in ((0, 4, v), (4, 0, v), (8193, 4, v), (4, 8193, v), (4, 4, 0), (4, 4, (1 << 24) + 1), (-1, -1, -1)):
        assert lib.rf_iou_ws_bytes(n_a, n_b, vox) == 0
    # 512 windows of 32^3: 512 words each, twice (a and b), plus the counts; 125 voxels are two words
    assert lib.rf_iou_ws_bytes(512, 512, v) == 2 * (512 * 512 * 8 + 512 * 4)
    assert lib.rf_iou_ws_bytes(7, 1, 125) == 256 + 256 + 256 + 256
    assert lib.rf_iou_ws_bytes(8192, 8192, 1 << 24) > 0


def test_python_entry_points_refuse_what_they_cannot_take():
    from rfuse.losses import iou_matrix, target_iou_matrix, RetrievalStepLoss
    grid = torch.zeros(4, 1, 8, 8, 8, dtype=torch.bool)
    for call in (lambda: iou_matrix(grid), lambda: iou_matrix(grid, grid), lambda: target_iou_matrix(grid.float(), 0.06, 0.01, 0.0156)):
        with pytest.raises(RuntimeError, match='iou_matrix: .*no CPU fallback'):
            call()
    step = RetrievalStepLoss(0.2, 0.06, 0.01, 0.020834)
    with pytest.raises(RuntimeError, match='RetrievalStepLoss: features_in.*no CPU fallback'):
        step(torch.zeros(4, 64, 1, 1, 1), torch.zeros(4, 64, 1, 1, 1), grid.float())
    with pytest.raises(TypeError, match='iou_matrix: batch_shapes: expected a torch.Tensor'):
        iou_matrix(np.zeros((4, 1, 8, 8, 8), bool))
    # rank, dtype and window are what a tensor says about itself: refused before the question where it lives
    g = grid
    for bad in (g[:, 0], g.reshape(4, 1, 8, 64), g.expand(4, 2, 8, 8, 8), g[:0]):
        with pytest.raises(ValueError, match=r'iou_matrix: batch_shapes: expected a non-empty \[n, 1, D, H, W\] tensor'):
            iou_matrix(bad)
    for dtype in (torch.float16, torch.int64, torch.float32):
        with pytest.raises(TypeError, match='iou_matrix: batch_shapes: expected torch.bool or torch.uint8, got %s' % dtype):
            iou_matrix(g.to(dtype))
    with pytest.raises(TypeError, match='iou_matrix: other: expected torch.bool or torch.uint8, got torch.float16'):
        iou_matrix(g, g.to(torch.float16))
    with pytest.raises(ValueError, match=r'iou_matrix: other has windows of \(8, 8, 4\), batch_shapes of \(8, 8, 8\)'):
        iou_matrix(g, g[..., :4])
    # a threshold belongs to float32 targets: a bool grid (or float16 / int64) is refused
    for dtype in (torch.bool, torch.uint8, torch.float16, torch.int64):
        with pytest.raises(TypeError, match='target_iou_matrix: target: expected torch.float32, got %s' % dtype):
            target_iou_matrix(g.to(dtype), 0.06, 0.01, 0.0156)
    with pytest.raises(ValueError, match=r'target_iou_matrix: target: expected a non-empty \[n, 1, D, H, W\] tensor'):
        target_iou_matrix(g.float()[0], 0.06, 0.01, 0.0156)
    with pytest.raises(ValueError, match=r'RetrievalStepLoss: features_in: expected a \[B, dim, d, h, w\] tensor'):
        step(torch.zeros(4, 64), torch.zeros(4, 64, 1, 1, 1), g.float())


def test_step_loss_constructor_and_from_config():
    from rfuse import configs
    from rfuse.losses import RetrievalStepLoss
    cfg = configs.get_config('C2')
    d = cfg['dataset_train']
    step = RetrievalStepLoss.from_config(cfg, temperature=0.2)
    assert (step.temperature, step.target_mean, step.target_std) == (0.2, d['target_mean'], d['target_std'])
    assert (step.iou_scaling, step.contrastive_weight, step.code_noise) == (True, 1.0, 0.0)
    assert step.threshold == 0.75 * 0.020834 != 0.75 * configs._f16(0.020834)           # the raw config value, as in the trainer
    assert (step.ntxent.temperature, step.ntxent.use_cosine_similarity, step.ntxent.sig_scale, step.ntxent.sig_shift) == (0.2, True, 80, -65)
    # the reference's retrieval_training section as it stands (config/base/retrieval_superresolution.yaml and the shipped retrieval_008_064.yaml)
    section = {'temprature': 0.2, 'lr': 0.0001, 'batch_size': 512, 'num_workers': 8, 'scheduler': [50, 75], 'iou_scaling': False, 'code_noise': 0.01,
               'input_noise': 0, 'loss': {'contrastive': 0.5}}
    step = RetrievalStepLoss.from_config(cfg, **section)
    assert (step.temperature, step.iou_scaling, step.contrastive_weight, step.code_noise) == (0.2, False, 0.5, 0.01)
    with pytest.raises(TypeError, match='temperature'):
        RetrievalStepLoss.from_config(cfg, iou_scaling=True)
    f = torch.arange(2 * 3 * 2 * 1 * 1, dtype=torch.float32).reshape(2, 3, 2, 1, 1)
    z = RetrievalStepLoss.reshape_features(f)
    assert z.shape == (4, 3) and torch.equal(z, torch.nn.functional.normalize(f.permute(0, 2, 3, 4, 1).reshape(-1, 3), dim=1))


def test_fixture_agrees_with_the_count_formula(golden_dir):
    """What the reference's get_iou_matrix returned is float32(inter) / (float32(union) + float32(1e-5)) of the integer counts, bit for bit; the float
    case's occupancy is the float32 expression of the trainer.  Guards the fixture and the formula the GPU tests use for the cases that are not in it."""
    cases = ir.load_fixture(golden_dir)
    assert list(cases) == list(ir.GRID_CASES) + [ir.FLOAT_CASE]
    assert (golden_dir / 'iou_matrix.npz').stat().st_size <= 1 << 20
    with np.load(golden_dir / 'iou_matrix.npz', allow_pickle=False) as z:
        assert all(z[k].dtype in (np.uint8, np.float16, np.float32, np.float64) for k in z.files)
    for name, (n, win) in ir.GRID_CASES.items():
        c = cases[name]
        assert c['occ'].shape == (n, 1) + win and c['occ'].dtype == torch.bool and c['iou'].dtype == torch.float32
        assert torch.equal(c['iou'], ir.count_formula(c['occ'])), name
        assert torch.equal(c['iou'], c['iou'].t())
    # the same formula by hand, in numpy, on one case
    occ = cases['n7_5']['occ'].numpy().reshape(7, -1)
    inter = occ.astype(np.int64) @ occ.astype(np.int64).T
    union = occ.sum(1)[:, None] + occ.sum(1)[None, :] - inter
    assert np.array_equal(cases['n7_5']['iou'].numpy(), inter.astype(np.float32) / (union.astype(np.float32) + np.float32(1e-5)))
    # what each case is there for
    assert cases['n1_empty']['iou'].item() == 0.0 and cases['n1_full']['iou'].item() == np.float32(64) / (np.float32(64) + np.float32(1e-5))
    m = cases['n7_5']['iou']
    assert not cases['n7_5']['occ'][1].any() and cases['n7_5']['occ'][3].all() and torch.equal(cases['n7_5']['occ'][5], cases['n7_5']['occ'][2])
    assert not m[1].any() and m[3, 3] == np.float32(125) / (np.float32(125) + np.float32(1e-5)) and m[2, 5] == m[2, 2] and torch.equal(m[2], m[5])
    block = cases['other']['iou'][:ir.OTHER_SPLIT, ir.OTHER_SPLIT:]
    assert block.shape == (5, 19) and torch.equal(block, ir.count_formula(cases['other']['occ'][:5], cases['other']['occ'][5:]))
    c = cases[ir.FLOAT_CASE]
    mean, std, voxel = (float(x) for x in c['params'])
    assert c['target'].shape == (20, 1, 32, 32, 32) and c['target'].dtype == torch.float32 and c['iou'].shape == (40, 40)
    occ = ir.occupied(c['target'], mean, std, 0.75 * voxel)
    assert torch.equal(c['iou'], ir.count_formula(occ).repeat(2, 2))
    frac = occ.reshape(20, -1).float().mean(1)
    assert frac.min() > 0 and frac.max() > 0.2 and frac.max() / frac.min() > 20           # a real spread of occupancies
    # the float32 rule: the scalars act as float32 values, not as the doubles they are in Python
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    assert torch.equal(occ, c['target'] * f32(std) + f32(mean) <= f32(0.75 * voxel))
