"""CPU: the float64 transcription of the attention backward's formulas (tests/attention_backward_ref.py:reference_f64 -- what
tests/test_attention_backward_gpu.py holds rf_attn_fuse_backward against) is pinned to float64 autograd of the oracle's own
attention_block (oracle/refpath.py:140-167, the reference's model/attention.py:84-113), including the rule for tied maxima, the dead switch and
the inverse index map of the retrieved-feature regroup."""
import pytest
import torch
import torch.nn.functional as F

import attention_backward_ref as ref
from oracle import refpath


def oracle_grads(monkeypatch, x, p, xf, pf, noise, dout, mode, e):
    """float64 autograd of refpath.attention_block with its two encoders replaced by the given raw features (leaves): (dx, dp, dxf, dpf)"""
    R, K = p.shape[0], p.shape[1]
    leaves = [t.detach().double().clone().requires_grad_(True) for t in (x, p, xf, pf)]
    xl, pl, xfl, pfl = leaves
    monkeypatch.setattr(refpath, 'attention_feature_encoder', lambda v, sd, prefix: xfl if prefix.endswith('.theta') else pfl.reshape(R * K, -1))
    c = x.shape[1] // e ** 3
    out = refpath.attention_block(xl.reshape(R, c, e, e, e), pl.reshape(R, K, c, e, e, e), {}, 'a', mode == ref.GUMBEL_HARD,
                                  noise.double() if mode == ref.GUMBEL_HARD else None)
    return torch.autograd.grad(out, leaves, dout.double().reshape(out.shape))


def assert_matches(got, want, tol=1e-12):
    for name, w in zip(('dx', 'dp', 'dxf', 'dpf'), want):
        assert ref.rel_err(got[name], w) <= tol, (name, ref.rel_err(got[name], w))


@pytest.mark.parametrize('mode', [ref.SOFTMAX, ref.GUMBEL_HARD])
@pytest.mark.parametrize('K', [1, 4, 8, 16])
@pytest.mark.parametrize('f', [24, 32])
def test_transcription_equals_float64_autograd_of_the_oracle(monkeypatch, mode, K, f):
    e = 2                                                                   # the oracle's sharpness is 32 * e^3 * 4 = 1024
    x, p, xf, pf, noise, dout = ref.make_inputs(96, K, 2 * e ** 3, f, seed=K + f)
    got = ref.reference_f64(x, p, xf, pf, noise, dout, mode, 1024.0)
    assert_matches(got, oracle_grads(monkeypatch, x, p, xf, pf, noise, dout, mode, e))


@pytest.mark.parametrize('mode', [ref.SOFTMAX, ref.GUMBEL_HARD])
def test_tied_maxima_send_the_switch_gradient_to_the_lower_index(monkeypatch, mode):
    x, p, xf, pf, noise, dout = ref.tie_inputs()
    got = ref.reference_f64(x, p, xf, pf, noise, dout, mode, 1024.0)
    assert float(got['score_gap'].max()) == 0.0                            # the tie is exact in float64 too
    # F.max_pool1d (the reference's MaxPool1d(K), model/attention.py:99) in float64: the whole gradient at the lower of the two indices
    s = (F.normalize(xf.double(), dim=1)[:, None] * F.normalize(pf.double(), dim=2)).sum(dim=2).requires_grad_(True)
    F.max_pool1d(s[:, None, :], s.shape[1]).sum().backward()
    assert torch.equal(s.grad, F.one_hot(torch.full((s.shape[0],), 1), s.shape[1]).double())
    assert_matches(got, oracle_grads(monkeypatch, x, p, xf, pf, noise, dout, mode, 2))
    # the element-wise formula with amax splits that gradient among the ties: it is NOT the reference's gradient
    old = ref.torch_formula_grads(*(t.double() for t in (x, p, xf, pf, noise, dout)), mode, 1024.0)
    assert ref.rel_err(old[3], got['dpf']) > 1e-3


@pytest.mark.parametrize('mode', [ref.SOFTMAX, ref.GUMBEL_HARD])
def test_dead_switch_passes_the_gradient_to_x_alone(monkeypatch, mode):
    x, p, xf, pf, noise, dout = ref.dead_inputs()
    got = ref.reference_f64(x, p, xf, pf, noise, dout, mode, 1024.0)
    assert torch.equal(got['dx'], dout.double())
    for name in ('dp', 'dxf', 'dpf'):
        assert float(got[name].abs().max()) == 0.0, name
    want = oracle_grads(monkeypatch, x, p, xf, pf, noise, dout, mode, 2)
    assert torch.equal(want[0], dout.double()) and all(float(w.abs().max()) == 0.0 for w in want[1:])


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('geom', [(2, 3, 5, 8, 2, 4), (1, 4, 12, 8, 2, 8)])
def test_inverse_index_map_of_the_gather(layout, geom):
    b, k, c, s, e, t = geom
    gen = torch.Generator().manual_seed(3)
    shape = (b * k, c, s, s, s) if layout == 0 else (b * k * (s // t) ** 3, c, t, t, t)
    u = torch.randn(shape, generator=gen, dtype=torch.float64).requires_grad_(True)
    rows = ref.gather_view(u, layout, b, k, c, s, e, t)
    # against the oracle's own regroup (oracle/refpath.py:174-176) for folded volumes
    vols = u if layout == 0 else ref.fold_view(u, s // t, t, c)
    r = s // e
    want = refpath.unfold3d(vols, e).reshape(-1, k, r, r, r, c, e, e, e).permute(0, 2, 3, 4, 1, 5, 6, 7, 8).reshape(-1, k, c, e, e, e)
    assert torch.equal(rows, want)
    v = torch.randn(rows.shape, generator=gen, dtype=torch.float64)
    inv = ref.gather_view_inverse(v, layout, b, k, c, s, e, t)
    assert torch.equal(inv, torch.autograd.grad(rows, u, v)[0])                          # the inverse map is the backward
    assert torch.equal(ref.gather_view(inv, layout, b, k, c, s, e, t), v)
    assert torch.equal(ref.gather_view_inverse(rows.detach(), layout, b, k, c, s, e, t), u.detach())


# ------------------------------------------------------------------------------------------------------------ the sixth header

NAMES = {'rf_attn_fuse_backward', 'rf_attn_scatter_retrieved'}


def test_attn_train_header_is_bound_exported_and_refuses_bad_arguments():
    """include/rfuse_attn_train.h: declared == bound == exported, disjoint from the other five tables, every entry point a status function that
    raises under its own name on arguments the library refuses before anything reaches a device"""
    import ctypes
    import re
    from pathlib import Path
    from rfuse import _lib
    repo = Path(__file__).resolve().parents[1]
    text = re.sub(r'/\*.*?\*/', '', (repo / 'include' / 'rfuse_attn_train.h').read_text(), flags=re.S)
    assert set(re.findall(r'\b(rf_[a-z0-9_]+)\s*\(', text)) == NAMES == set(_lib.ATTN_TRAIN_SIGNATURES)
    lib = _lib.load_attn_train()
    assert lib is _lib.load_attn_train() and lib._cdll is _lib.load()._cdll and set(lib._direct) == NAMES
    others = (_lib.SIGNATURES, _lib.EVAL_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.CONTRASTIVE_SIGNATURES, _lib.PAIRS_SIGNATURES)
    assert not any(NAMES & set(t) for t in others)
    assert {n for n in NAMES if _lib.is_status(n, _lib.ATTN_TRAIN_SIGNATURES)} == NAMES
    build_py = (repo / 'retrieval-fuse_amd' / 'csrc' / 'build.py').read_text()
    assert "'attention_backward.hip': ['-ffp-contract=off']" in build_py and "'rfuse_attn_train.h'" in build_py
    one = ctypes.c_void_p(256)                       # a non-null pointer that the argument checks never follow
    with pytest.raises(RuntimeError, match=r'^rf_attn_fuse_backward failed \(rc=-1\): .*bad arguments'):
        lib.rf_attn_fuse_backward(one, one, one, one, None, None, 4, 4, 8, 32, 0, 1.0, one, one, one, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_attn_fuse_backward failed \(rc=-2\): .*K=17'):
        lib.rf_attn_fuse_backward(one, one, one, one, None, one, 4, 17, 8, 32, 0, 1.0, one, one, one, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_attn_fuse_backward failed \(rc=-2\): .*feature width 129'):
        lib.rf_attn_fuse_backward(one, one, one, one, None, one, 4, 4, 8, 129, 0, 1.0, one, one, one, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_attn_fuse_backward failed \(rc=-1\): .*needs the noise'):
        lib.rf_attn_fuse_backward(one, one, one, one, None, one, 4, 4, 8, 32, 1, 25.0, one, one, one, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_attn_scatter_retrieved failed \(rc=-1\): .*bad arguments'):
        lib.rf_attn_scatter_retrieved(one, 0, 1, 4, 16, 9, 2, 0, one, None)
    with pytest.raises(RuntimeError, match=r'^rf_attn_scatter_retrieved failed \(rc=-1\): .*bad layout 1 / patch edge 3'):
        lib.rf_attn_scatter_retrieved(one, 1, 1, 4, 16, 8, 2, 3, one, None)
