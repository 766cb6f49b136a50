"""CPU: the mesh metrics' host side (rfuse/mesh_metrics.py, include/rfuse_eval.h; reference util/mesh_metrics.py:13-120) -- the second header's
binding and its status rule, rfuse.h's table untouched by it, the .obj reader, the refusal of CPU input, and the reference-generated fixture
(tools/gen_mesh_metrics_golden.py) against a numpy float64 brute force."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parents[1]


def declared_eval_symbols():
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'rfuse_eval.h').read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(rf_[a-z0-9_]+)\s*\(', text)))


def load_fixture(golden_dir):
    z = dict(np.load(golden_dir / 'mesh_metrics.npz'))
    shape = tuple(int(s) for s in z['vox_shape'])
    for k in ('vox_pred', 'vox_tgt', 'vox_margin'):
        z[k] = np.unpackbits(z[k])[:int(np.prod(shape))].astype(bool).reshape(shape)
    for k in ('pred_t', 'tgt_t', 'pred_f', 'tgt_f'):
        z[k] = z[k].astype(np.int32)
    return z


def face_normals_f32(v, t):
    """float32(unit face normal): float64 cross product of the float32 vertices, normalised in float64 (the fixture's normals are these, per sample face)"""
    p = v.astype(np.float64)[t.astype(np.int64)]
    c = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return (c / np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])[:, None]).astype(np.float32)


def brute_nearest(src, tgt, block=256):
    """numpy float64 brute force: (d2, lowest argmin, number of targets at the minimum) with d2 = (dx dx + dy dy) + dz dz"""
    s, t = src.astype(np.float64), tgt.astype(np.float64)
    d2, idx, hits = np.empty(len(s)), np.empty(len(s), np.int64), np.empty(len(s), np.int64)
    for k in range(0, len(s), block):
        d = s[k:k + block, None, :] - t[None]
        q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        idx[k:k + block] = q.argmin(1)                      # numpy's argmin: the first (lowest) index of the minimum
        d2[k:k + block] = q.min(1)
        hits[k:k + block] = (q == q.min(1, keepdims=True)).sum(1)
    return d2, idx, hits


def test_eval_header_is_bound_and_exported():
    from rfuse import _lib
    names = declared_eval_symbols()
    assert {'rf_eval_sample_surface', 'rf_eval_nearest3', 'rf_eval_nearest3_ws_bytes', 'rf_eval_p2p_stats', 'rf_eval_voxelize'} <= set(names)
    assert set(names) == set(_lib.EVAL_SIGNATURES), 'EVAL_SIGNATURES out of sync with include/rfuse_eval.h'
    lib = _lib.load_eval()
    for n in names:
        assert hasattr(lib, n), '%s declared in include/rfuse_eval.h but not exported by librfuse_hip.so' % n
    assert lib is _lib.load_eval() and lib._cdll is _lib.load()._cdll            # one shared object
    assert _lib.EVAL_SIGNATURES['rf_eval_voxelize'][1][4] is ctypes.c_float      # pitch: the vocabulary has no double scalar
    assert ctypes.c_double not in {a for _, args, _ in _lib.EVAL_SIGNATURES.values() for a in args}


def test_rfuse_h_table_is_unchanged_by_the_second_binding():
    from rfuse import _lib
    before = dict(_lib.SIGNATURES)
    main, ev = _lib.load(), _lib.load_eval()
    assert _lib.SIGNATURES == before and not set(_lib.SIGNATURES) & set(_lib.EVAL_SIGNATURES)
    assert set(main._direct) == set(_lib.SIGNATURES) and set(ev._direct) == set(_lib.EVAL_SIGNATURES)
    assert not any(n.startswith('rf_eval_') for n in _lib.SIGNATURES) and all(n.startswith('rf_eval_') for n in _lib.EVAL_SIGNATURES)
    records = []
    main.start_profile(records)                      # the profiling wrapper covers rfuse.h only
    try:
        assert all(getattr(ev, n) is ev._direct[n] for n in _lib.EVAL_SIGNATURES)
    finally:
        main.stop_profile()
    assert 'rfuse_eval.h' not in (REPO / 'include' / 'rfuse.h').read_text()


def test_eval_status_functions_raise_under_their_own_name():
    """refused arguments, before any device is touched"""
    from rfuse import _lib
    lib = _lib.load_eval()
    status = {n for n in _lib.EVAL_SIGNATURES if _lib.is_status(n, _lib.EVAL_SIGNATURES)}
    assert status == {'rf_eval_face_areas', 'rf_eval_sample_surface', 'rf_eval_nearest3', 'rf_eval_p2p_stats', 'rf_eval_voxelize'}
    assert {n for n, fn in lib._direct.items() if fn.errcheck is not None} == status
    with pytest.raises(RuntimeError, match=r'^rf_eval_face_areas failed \(rc=-1\): .*bad arguments'):
        lib.rf_eval_face_areas(None, 0, None, 0, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_eval_sample_surface failed \(rc=-1\): .*bad arguments'):
        lib.rf_eval_sample_surface(None, None, None, 0, 0, 0, None, None, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_eval_nearest3 failed \(rc=-1\): .*bad arguments'):
        lib.rf_eval_nearest3(None, 1, None, 1, None, None, None, 0, None)
    one = ctypes.c_void_p(256)                       # a non-null pointer that the argument checks never follow
    with pytest.raises(RuntimeError, match=r'^rf_eval_nearest3 failed \(rc=-2\): .*at most 2\^24'):
        lib.rf_eval_nearest3(one, (1 << 24) + 1, one, 1, one, one, one, 0, None)
    with pytest.raises(RuntimeError, match=r'^rf_eval_nearest3 failed \(rc=-4\): .*workspace of 16 bytes'):
        lib.rf_eval_nearest3(one, 1000, one, 5000, one, one, one, 16, None)
    with pytest.raises(RuntimeError, match=r'^rf_eval_p2p_stats failed \(rc=-1\): .*bad arguments'):
        lib.rf_eval_p2p_stats(None, None, None, None, 0, 0, None, 0, None, None, None, None, None, 0, None)
    with pytest.raises(RuntimeError, match=r'^rf_eval_p2p_stats failed \(rc=-1\): .*normals without neighbour indices'):
        lib.rf_eval_p2p_stats(one, None, one, one, 5, 5, None, 0, one, one, None, one, one, 1 << 20, None)
    with pytest.raises(RuntimeError, match=r'^rf_eval_voxelize failed \(rc=-2\): .*4096 x 2 x 2'):
        lib.rf_eval_voxelize(one, 3, one, 1, 1.1875, 0, 0, 0, 4096, 2, 2, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_eval_voxelize failed \(rc=-1\): .*pitch'):
        lib.rf_eval_voxelize(one, 3, one, 1, 0.0, 0, 0, 0, 2, 2, 2, one, None)
    # value functions: 0 is an answer
    assert lib.rf_eval_nearest3_ws_bytes(0, 5) == 0 and lib.rf_eval_nearest3_ws_bytes(5, (1 << 24) + 1) == 0
    assert lib.rf_eval_nearest3_ws_bytes(1 << 24, 1 << 24) > 0 and lib.rf_eval_p2p_stats_ws_bytes(100000) > 0
    n = 100000
    assert lib.rf_eval_nearest3_ws_bytes(n, n) % 256 == 0 and lib.rf_eval_nearest3_ws_bytes(n, n) >= 12 * n


def test_load_obj_round_trips_export_obj_and_reads_polygons(tmp_path):
    from rfuse import mesh
    rng = np.random.default_rng(3)
    v = (rng.random((40, 3)) * 64).astype(np.float32)
    t = rng.integers(0, 40, (70, 3)).astype(np.int32)
    mesh.export_obj(torch.from_numpy(v), torch.from_numpy(t), tmp_path / 'a.obj')
    v2, t2 = mesh.load_obj(tmp_path / 'a.obj')
    assert v2.dtype == np.float32 and t2.dtype == np.int32
    np.testing.assert_array_equal(t2, t)
    assert np.abs(v2.astype(np.float64) - v).max() <= 0.5e-6 + 4e-6           # '%f': six decimals, then float32
    mesh.export_obj(v2, t2, tmp_path / 'b.obj')                               # what was read writes the same file again
    assert (tmp_path / 'a.obj').read_text() == (tmp_path / 'b.obj').read_text()
    (tmp_path / 'c.obj').write_text('# a comment\nmtllib x.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 0.5 1 1.0\nvn 0 0 1\nvt 0 0\n'
                                    'f 1/1/1 2/1/1 3/1/1 4/1/1\nf 1//1 2//1 5//1\nf -1 2/7 3\ns off\nf 1 2 3 4 5\n')
    v3, t3 = mesh.load_obj(tmp_path / 'c.obj')
    assert v3.shape == (5, 3) and v3[4].tolist() == [0.5, 0.5, 1.0]
    assert t3.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [4, 1, 2], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    (tmp_path / 'd.obj').write_text('v 0 0 0\nv 1 0 0\nf 1 2 3\n')
    with pytest.raises(ValueError, match='vertex 3 of 2'):
        mesh.load_obj(tmp_path / 'd.obj')
    (tmp_path / 'e.obj').write_text('v 0 0 0\n')
    v5, t5 = mesh.load_obj(tmp_path / 'e.obj')
    assert v5.shape == (1, 3) and t5.shape == (0, 3)


def test_cpu_input_has_no_fallback_and_empty_meshes_are_refused(tmp_path):
    from rfuse import mesh_metrics as mm
    v, t = torch.rand(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32)
    p, n = torch.rand(10, 3), torch.rand(10, 3)
    for call in (lambda: mm.sample_surface(v, t, 10), lambda: mm.nearest_points(p, p), lambda: mm.distance_p2p(p, n, p, n),
                 lambda: mm.distance_p2p(p, None, p, None), lambda: mm.get_threshold_percentage(torch.rand(10, dtype=torch.float64), [0.5]),
                 lambda: mm.voxel_iou(v, t, v, t), lambda: mm.mesh_metrics(v, t, v, t, n_samples=10)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    none = torch.zeros(0, 3, dtype=torch.int32)
    for call in (lambda: mm.sample_surface(v, none, 10), lambda: mm.voxel_iou(v, t, v, none), lambda: mm.mesh_metrics(v, none, v, t)):
        with pytest.raises(ValueError, match='without triangles'):
            call()
    assert mm.PITCH == 1.1875 and mm.N_SAMPLES == 100000
    np.testing.assert_array_equal(mm.THRESHOLDS, np.linspace(64. / 1000, 64, 1000))
    import inspect
    assert list(inspect.signature(mm.distance_p2p).parameters) == ['points_src', 'normals_src', 'points_tgt', 'normals_tgt']
    assert list(inspect.signature(mm.compute_metrics).parameters) == ['path_pred', 'path_target', 'n_samples', 'seed']


def test_fixture_is_self_consistent(golden_dir):
    """what the reference's functions returned is what a numpy float64 brute force over the stored samples gives: cKDTree's distances bit for bit,
    its neighbours (no ties in the fixture: the generator caps them), the threshold counts, and compute_metrics' five numbers from them"""
    z = load_fixture(golden_dir)
    assert (golden_dir / 'mesh_metrics.npz').stat().st_size < 1 << 20
    normals = {'pred': face_normals_f32(z['pred_v'], z['pred_t'])[z['pred_f']], 'tgt': face_normals_f32(z['tgt_v'], z['tgt_t'])[z['tgt_f']]}
    means = {}
    for name, src, tgt in (('completeness', 'tgt', 'pred'), ('accuracy', 'pred', 'tgt')):
        d2, idx, hits = brute_nearest(z[src + '_p'], z[tgt + '_p'])
        assert (hits > 1).mean() <= 1e-3
        np.testing.assert_array_equal(np.sqrt(d2), z[name + '_dist'])
        np.testing.assert_array_equal(idx[hits == 1], z[name + '_idx'][hits == 1])
        a, b = normals[tgt].astype(np.float64)[idx], normals[src].astype(np.float64)
        a, b = a / np.linalg.norm(a, axis=-1, keepdims=True), b / np.linalg.norm(b, axis=-1, keepdims=True)
        np.testing.assert_allclose(np.abs((a * b).sum(-1)), z[name + '_dots'], rtol=0, atol=1e-15)
        dist = z[name + '_dist']
        np.testing.assert_array_equal(np.searchsorted(np.sort(dist), z['thresholds'], side='right'), z[name + '_counts'])
        means[name] = (dist.mean(), z[name + '_dots'].mean(), z[name + '_counts'] / len(dist))
    gp, gt = z['vox_pred'], z['vox_tgt']
    assert not z['vox_margin'].any() or z['vox_margin'].sum() <= 1e-3 * (gp | gt).sum()
    f = 2 * means['accuracy'][2] * means['completeness'][2] / (means['accuracy'][2] + means['completeness'][2])
    want = [(gp & gt).sum() / (gp | gt).sum(), 0.5 * (means['completeness'][0] + means['accuracy'][0]),
            0.5 * means['completeness'][1] + 0.5 * means['accuracy'][1], f[9], f[14]]
    np.testing.assert_allclose(z['metrics'], want, rtol=1e-13)
    assert 0.3 < z['metrics'][0] < 0.95 and 0 < z['metrics'][3] < z['metrics'][4] < 1          # two different surfaces: nothing saturates
