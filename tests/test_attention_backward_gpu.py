"""GPU: the backward of the patch attention's row route -- rf_attn_fuse_backward, rf_attn_scatter_retrieved (csrc/attention_backward.hip), the
Functions of rfuse/autograd.py around them (AttnFuse, Unfold3d, Fold3d, GatherRetrieved) and the grad-mode route of model/attention.py.

Accuracy bar: per tensor, the error against the float64 transcription of the formulas (tests/attention_backward_ref.py, pinned to float64 autograd of the
oracle in tests/test_attention_backward_cpu.py) evaluated on the same float32 inputs, as max-abs over the tensor / the reference's max-abs, may be at most
4 x the error of the element-wise torch formula the modules used before (run in fp32 on the GPU on the same inputs); where that comparator's own error is
below 1e-6 the bound is 4e-6.  Both are fp32 evaluations whose error is the rounding of the scores amplified by the sharpness.  A row is left out only if
a discrete decision is within rounding in float64 (two largest scores closer than 1e-6; Gumbel: two largest logits closer than 1e-4), at most 2 % of rows."""
import contextlib
import io

import numpy as np
import pytest
import torch

import attention_backward_ref as ref
import helpers
import testkit
from oracle import refpath

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NAMES = ('dx', 'dp', 'dxf', 'dpf')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    from rfuse import ops as o
    return o


def sharpness_of(mode):
    return 1024.0 if mode == ref.SOFTMAX else 25.0


_cases = {}


def case(R, K, d, f, mode, seed=0):
    """inputs (CPU, float32), the float64 reference and the rows that stay in the comparison; computed once per case and left unchanged"""
    key = (R, K, d, f, mode, seed)
    if key not in _cases:
        inp = ref.make_inputs(R, K, d, f, seed)
        want = ref.reference_f64(*inp, mode, sharpness_of(mode))
        keep = want['score_gap'] >= 1e-6
        if mode == ref.GUMBEL_HARD:
            keep &= want['logit_gap'] >= 1e-4
        _cases[key] = (inp, want, keep)
    return _cases[key]


def run_hip(ops, inp, mode, need=(True, True, True, True)):
    x, p, xf, pf, noise, dout = (t.to(DEV) for t in inp)
    return ops.attn_fuse_backward(x, p, xf, pf.reshape(-1, pf.shape[-1]), noise if mode == ref.GUMBEL_HARD else None, dout, mode, sharpness_of(mode), need)


def check_accuracy(label, got, comparator, want, keep, max_excluded=0.02):
    """the 4 x rule of the module docstring; prints both errors per tensor before it asserts"""
    excluded = int((~keep).sum())
    print('\n%s: %d of %d rows excluded' % (label, excluded, keep.numel()))
    assert excluded <= max_excluded * keep.numel(), 'too many rows with a discrete decision within rounding'
    failed = []
    for name, g, c in zip(NAMES, got, comparator):
        w = want[name][keep]
        e_hip, e_torch = ref.rel_err(g.cpu().reshape(want[name].shape)[keep], w), ref.rel_err(c.cpu().reshape(want[name].shape)[keep], w)
        bound = 4 * max(e_torch, 1e-6)
        print('  %-4s hip %.3e   torch fp32 %.3e   bound %.3e' % (name, e_hip, e_torch, bound))
        if not e_hip <= bound:
            failed.append((name, e_hip, bound))
    assert not failed, failed


SHAPES = [(1, 1, 8, 32, ref.SOFTMAX), (5, 4, 96, 32, ref.GUMBEL_HARD), (1027, 8, 128, 32, ref.SOFTMAX), (2048, 4, 128, 32, ref.SOFTMAX),
          (2048, 4, 128, 32, ref.GUMBEL_HARD), (2048, 8, 128, 32, ref.SOFTMAX), (2048, 8, 128, 32, ref.GUMBEL_HARD), (67, 16, 432, 24, ref.SOFTMAX),
          (67, 16, 432, 24, ref.GUMBEL_HARD), (16389, 2, 8, 32, ref.SOFTMAX)]


@pytest.mark.parametrize('R,K,d,f,mode', SHAPES)
def test_backward_against_float64_within_four_times_the_torch_formula(ops, R, K, d, f, mode):
    """every shape at which the kernel takes another path: one row, K = 1, fewer rows than a workgroup's four, rows that are no multiple of four, d
    below / equal to / no multiple of the wave, f = 32 (register form) and f = 24 (loop form), K = 16 = RF_MAX_K, and more rows than the capped grid
    covers in one pass (4096 workgroups x 4 rows); and the NULL-output variants against the full call bit for bit"""
    inp, want, keep = case(R, K, d, f, mode)
    got = run_hip(ops, inp, mode)
    gpu_inp = [t.to(DEV) for t in inp]
    comparator = ref.torch_formula_grads(*gpu_inp[:5], gpu_inp[5], mode, sharpness_of(mode))
    torch.cuda.synchronize()
    check_accuracy('rows %d K %d d %d f %d mode %d' % (R, K, d, f, mode), got, comparator, want, keep)
    for need in [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (True, True, False, False), (False, False, True, True), (False, True, True, False)]:
        part = run_hip(ops, inp, mode, need)
        for name, n, a, b in zip(NAMES, need, part, got):
            assert (a is None) == (not n), (need, name)
            if n:
                assert torch.equal(a, b), (need, name)


def test_gumbel_decisions_are_the_forwards(ops):
    """the slot that receives dp != 0 is the slot the forward's hard weight chose, in every row"""
    inp, _, _ = case(2048, 8, 128, 32, ref.GUMBEL_HARD)
    x, p, xf, pf, noise, dout = (t.to(DEV) for t in inp)
    _, _, weights = ops.attn_fuse(x, p, xf, pf.reshape(-1, 32), noise, ref.GUMBEL_HARD, 25.0, debug=True)
    dp = run_hip(ops, inp, ref.GUMBEL_HARD, (False, True, False, False))[1]
    hit = dp.ne(0).any(dim=2)                                               # [R,K]
    assert bool((hit.sum(dim=1) == 1).all())                                # (every score of these inputs is positive: no dead switch)
    assert torch.equal(hit.float().argmax(dim=1), weights.argmax(dim=1))
    assert bool((weights.gather(1, hit.float().argmax(dim=1, keepdim=True)) > 0.5).all()) and bool((weights.sum(dim=1) < 1.5).all())


@pytest.mark.parametrize('mode', [ref.SOFTMAX, ref.GUMBEL_HARD])
def test_exact_tie_goes_to_the_lower_index(ops, mode):
    """two retrieved slots holding the same patch: no row excluded.  The comparator is the torch formula with the oracle's max(dim) (bit-identical
    features give bit-identical scores in any evaluation, so the tie is exact in fp32 too); the formula's amax splits the gradient and is far off."""
    inp = ref.tie_inputs()
    want = ref.reference_f64(*inp, mode, sharpness_of(mode))
    assert float(want['score_gap'].max()) == 0.0
    got = run_hip(ops, inp, mode)
    gpu_inp = [t.to(DEV) for t in inp]
    comparator = ref.torch_formula_grads(*gpu_inp[:5], gpu_inp[5], mode, sharpness_of(mode), first_max=True)
    check_accuracy('tie, mode %d' % mode, got, comparator, want, torch.ones(inp[0].shape[0], dtype=torch.bool))
    split = ref.torch_formula_grads(*gpu_inp[:5], gpu_inp[5], mode, sharpness_of(mode))
    assert ref.rel_err(split[3], want['dpf']) > 1e-3


@pytest.mark.parametrize('mode', [ref.SOFTMAX, ref.GUMBEL_HARD])
def test_dead_switch(ops, mode):
    inp = ref.dead_inputs()
    dx, dp, dxf, dpf = run_hip(ops, inp, mode)
    assert torch.equal(dx.cpu(), inp[5])
    for name, t in (('dp', dp), ('dxf', dxf), ('dpf', dpf)):
        assert float(t.abs().max()) == 0.0, name


@pytest.mark.parametrize('mode', [ref.SOFTMAX, ref.GUMBEL_HARD])
def test_nonfinite_upstream_gradient_stays_in_its_row(ops, mode):
    inp, _, _ = case(1027, 8, 128, 32, mode)
    clean = run_hip(ops, inp, mode)
    dout = inp[5].clone()
    dout[513, 3], dout[513, 77] = float('nan'), float('inf')
    dirty = run_hip(ops, inp[:5] + (dout,), mode)
    others = torch.arange(1027) != 513
    for name, a, b in zip(NAMES, clean, dirty):
        a, b = a.cpu().reshape(1027, -1), b.cpu().reshape(1027, -1)
        assert torch.equal(a[others], b[others]), name
        assert not bool(torch.isfinite(b[513]).all()), name


def test_same_bits_on_every_call_and_beside_an_f16_mfma_load(ops):
    """two calls, then 20 calls on a side stream beside the testkit's F16-MFMA load (as tests/test_two_stream_gpu.py does for the other families)"""
    for mode in (ref.SOFTMAX, ref.GUMBEL_HARD):
        inp, _, _ = case(2048, 4, 128, 32, mode)
        x, p, xf, pf, noise, dout = (t.to(DEV) for t in inp)
        pf = pf.reshape(-1, 32)

        def run():
            return ops.attn_fuse_backward(x, p, xf, pf, noise if mode == ref.GUMBEL_HARD else None, dout, mode, sharpness_of(mode))
        first, second = run(), run()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, second))
        main, side = torch.cuda.current_stream(), torch.cuda.Stream(DEV)
        scratch = torch.empty(256 * 256, device=DEV)
        outs = []
        side.wait_stream(main)
        testkit.f16_mfma_load(main, scratch)
        with torch.cuda.stream(side):
            for _ in range(20):
                outs.append(run())
        torch.cuda.synchronize()
        bad = sum(0 if all(torch.equal(a, b) for a, b in zip(o, first)) else 1 for o in outs)
        assert bad == 0, '%d of 20 launches with different bits beside the F16-MFMA load (mode %d)' % (bad, mode)


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('geom', [(2, 3, 5, 8, 2, 4), (1, 4, 12, 8, 2, 8)])
def test_scatter_is_the_inverse_of_the_gather(ops, layout, geom):
    """b = 2, K = 3, c = 5, s = 8, e = 2, t = 4 and the C5 geometry (nf = 12) cut to s = 8"""
    b, k, c, s, e, t = geom
    gen = torch.Generator().manual_seed(13)
    shape = (b * k, c, s, s, s) if layout == 0 else (b * k * (s // t) ** 3, c, t, t, t)
    u = torch.randn(shape, generator=gen).to(DEV)
    rows = ops.attn_gather_retrieved(u, layout, b, k, c, s, e, t)
    v = torch.randn(rows.shape, generator=gen).to(DEV)
    dsrc = ops.attn_scatter_retrieved(v, layout, b, k, c, s, e, t)
    assert dsrc.shape == u.shape
    assert torch.equal(ops.attn_gather_retrieved(dsrc, layout, b, k, c, s, e, t), v)
    assert torch.equal(ops.attn_scatter_retrieved(rows, layout, b, k, c, s, e, t), u)
    leaf = u.clone().requires_grad_(True)
    view_rows = ref.gather_view(leaf, layout, b, k, c, s, e, t)
    assert torch.equal(view_rows, rows)
    assert torch.equal(torch.autograd.grad(view_rows, leaf, v)[0], dsrc)
    # and through the Function
    from rfuse import autograd as rf_autograd
    leaf2 = u.clone().requires_grad_(True)
    out = rf_autograd.GatherRetrieved.apply(leaf2, layout, b, k, c, s, e, t)
    assert torch.equal(out, rows) and torch.equal(torch.autograd.grad(out, leaf2, v)[0], dsrc)


@pytest.mark.parametrize('b,c,s,e', [(2, 5, 8, 2), (1, 12, 8, 4), (3, 1, 6, 3)])
def test_fold_and_unfold_functions_equal_the_views(ops, b, c, s, e):
    from rfuse import autograd as rf_autograd
    gen = torch.Generator().manual_seed(17)
    r = s // e
    x = torch.randn(b, c, s, s, s, generator=gen).to(DEV)
    g_rows = torch.randn(b * r ** 3, c, e, e, e, generator=gen).to(DEV)
    a, a_view = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    rows, rows_view = rf_autograd.Unfold3d.apply(a, e), ref.unfold_view(a_view, e)
    assert torch.equal(rows, rows_view)
    assert torch.equal(torch.autograd.grad(rows, a, g_rows)[0], torch.autograd.grad(rows_view, a_view, g_rows)[0])
    g_x = torch.randn(b, c, s, s, s, generator=gen).to(DEV)
    q, q_view = g_rows.clone().requires_grad_(True), g_rows.clone().requires_grad_(True)
    vol, vol_view = rf_autograd.Fold3d.apply(q, r, e, c), ref.fold_view(q_view, r, e, c)
    assert torch.equal(vol, vol_view)
    assert torch.equal(torch.autograd.grad(vol, q, g_x)[0], torch.autograd.grad(vol_view, q_view, g_x)[0])


# ------------------------------------------------------------------------------------------------------------ module level

def make_block(nf, K, retrieval_mode, seed, num_patch=4):
    from model.attention import AttentionBlock, PatchedAttentionBlock
    with contextlib.redirect_stdout(io.StringIO()):
        block = PatchedAttentionBlock(nf, num_patch, 2, K, AttentionBlock(nf, 2, K, True, True, retrieval_mode, True, True))
    sd = helpers.seeded_sd({n: tuple(v.shape) for n, v in block.state_dict().items()}, seed)
    block.load_state_dict(sd)
    return block.to(DEV).train(), sd


def module_inputs(nf, K, seed):
    gen = torch.Generator().manual_seed(seed)
    x_pred = torch.randn(1, nf, 8, 8, 8, generator=gen)
    x_retr = torch.randn(K, nf, 8, 8, 8, generator=gen)
    dout = torch.randn(1, nf, 8, 8, 8, generator=gen)
    noise = -torch.empty(64, K).exponential_(generator=gen).log()
    return x_pred, x_retr, dout, noise


def oracle_module_grads(sd, nf, K, retrieval_mode, x_pred, x_retr, dout, noise, dtype):
    """autograd of refpath.patched_attention_block on the CPU in ``dtype``: gradients of x_predicted, the retrieved features and every theta / phi
    parameter, by name"""
    cfg = {'nf': nf, 'K': K, 'attn_patch_extent': 4, 'attn_num_patch': 4, 'attn_retrieval_mode': retrieval_mode}
    sdo = {n: v.detach().clone().to(dtype).requires_grad_(True) for n, v in sd.items()}
    xp, xr = x_pred.detach().clone().to(dtype).requires_grad_(True), x_retr.detach().clone().to(dtype).requires_grad_(True)
    out = refpath.patched_attention_block(xp, xr, sdo, cfg, noise.to(dtype) if retrieval_mode else None)
    out.backward(dout.to(dtype))
    grads = {'x_predicted': xp.grad, 'retrieved': xr.grad}
    grads.update({n: v.grad for n, v in sdo.items() if v.grad is not None})
    return out.detach(), grads


MODULE_CASES = [(16, 4, False, 'forward'), (16, 4, True, 'forward'), (16, 8, False, 'forward'), (12, 4, False, 'forward'),
                (16, 4, False, 'patch_major'), (16, 4, True, 'patch_major'), (16, 8, False, 'patch_major')]


def run_module(block, entry, x_pred, x_retr, dout, noise):
    """one forward + backward of the module in grad mode -> (output, gradients by name); ``patch_major``: the same features in the retrieval
    backbone's patch-major layout with patch edge 4, its gradient folded back for the comparison"""
    block.zero_grad(set_to_none=True)
    xp = x_pred.to(DEV).requires_grad_(True)
    nz = noise.to(DEV) if block.attention_blocks_layer.retrieval_mode else None
    if entry == 'forward':
        xr = x_retr.to(DEV).requires_grad_(True)
        out = block(xp, xr, nz)
    else:
        xr = ref.unfold_view(x_retr, 4).contiguous().to(DEV).requires_grad_(True)
        out = block.forward_patch_major(xp, xr, 4, nz)
    out.backward(dout.to(DEV))
    grads = {'x_predicted': xp.grad, 'retrieved': xr.grad if entry == 'forward' else ref.fold_view(xr.grad, 2, 4, x_retr.shape[1])}
    grads.update({n: p.grad for n, p in block.named_parameters() if p.grad is not None})
    return out.detach(), grads


@pytest.mark.parametrize('nf,K,retrieval_mode,entry', MODULE_CASES)
def test_module_trains_like_the_oracle(ops, nf, K, retrieval_mode, entry):
    """PatchedAttentionBlock.forward / forward_patch_major in grad mode at b = 1, s = 8 (64 rows): gradients of x_predicted, the retrieved features and
    every theta / phi parameter against float64 autograd of refpath.patched_attention_block: cosine > 0.9999 over all gradients (the bar of
    tests/test_autograd_gpu.py) and per tensor the 4 x rule, with fp32 autograd of the same oracle as comparator"""
    block, sd = make_block(nf, K, retrieval_mode, 400 + nf + K)
    x_pred, x_retr, dout, noise = module_inputs(nf, K, 31 + K)
    out, grads = run_module(block, entry, x_pred, x_retr, dout, noise)
    torch.cuda.synchronize()
    out64, g64 = oracle_module_grads(sd, nf, K, retrieval_mode, x_pred, x_retr, dout, noise, torch.float64)
    out32, g32 = oracle_module_grads(sd, nf, K, retrieval_mode, x_pred, x_retr, dout, noise, torch.float32)
    print('\n  output: hip %.3e   torch fp32 %.3e' % (ref.rel_err(out, out64), ref.rel_err(out32, out64)))
    assert ref.rel_err(out, out64) <= 4 * max(ref.rel_err(out32, out64), 1e-6)
    assert set(g64) <= set(grads), sorted(set(g64) - set(grads))
    dot = n1 = n2 = 0.0
    failed = []
    for name, want in g64.items():
        g = grads[name].detach().cpu().double()
        dot, n1, n2 = dot + float((g * want).sum()), n1 + float((g * g).sum()), n2 + float((want * want).sum())
        e_hip, e_torch = ref.rel_err(g, want), ref.rel_err(g32[name], want)
        bound = 4 * max(e_torch, 1e-6)
        print('  %-46s hip %.3e   torch fp32 %.3e   bound %.3e' % (name, e_hip, e_torch, bound))
        if not e_hip <= bound:
            failed.append((name, e_hip, bound))
    cos = dot / np.sqrt(n1 * n2)
    print('  cosine over all gradients %.8f' % cos)
    assert cos > 0.9999
    assert not failed, failed


@pytest.mark.parametrize('nf,K,retrieval_mode', [(16, 4, False), (16, 4, True), (16, 8, False)])
def test_forward_and_forward_patch_major_agree_bit_for_bit(ops, nf, K, retrieval_mode):
    block, _ = make_block(nf, K, retrieval_mode, 400 + nf + K)
    inputs = module_inputs(nf, K, 31 + K)
    out_a, g_a = run_module(block, 'forward', *inputs)
    out_b, g_b = run_module(block, 'patch_major', *inputs)
    assert torch.equal(out_a, out_b)
    assert set(g_a) == set(g_b)
    for name in g_a:
        assert torch.equal(g_a[name], g_b[name]), name


@pytest.mark.parametrize('retrieval_mode', [False, True])
def test_attention_block_grad_mode_output_is_attn_fuse(ops, retrieval_mode):
    block, _ = make_block(16, 4, retrieval_mode, 77)
    att = block.attention_blocks_layer
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(64, 16, 2, 2, 2, generator=gen).to(DEV).requires_grad_(True)
    p = torch.randn(64, 4, 16, 2, 2, 2, generator=gen).to(DEV).requires_grad_(True)
    noise = (-torch.empty(64, 4).exponential_(generator=gen).log()).to(DEV) if retrieval_mode else None
    out = att(x, p, noise)
    assert out.requires_grad
    xf, pf = att.theta(x.detach()).detach(), att.phi(p.detach().reshape(256, 16, 2, 2, 2)).detach()      # the grad-mode encoders (the weights require grad)
    with torch.no_grad():
        want = ops.attn_fuse(x.detach(), p.detach(), xf, pf, noise, ref.GUMBEL_HARD if retrieval_mode else ref.SOFTMAX, 25.0 if retrieval_mode else 1024.0)
    assert torch.equal(out.detach(), want)


def test_stage_keeps_less_memory_than_the_torch_formula(ops):
    """C3 at B = 1 (4096 rows, K = 4, 16 channels x 2^3): bytes held between forward and backward, and peak allocated bytes of forward + backward of
    the stage, new route against the torch formula.

    Measured on MI355X: held after forward 46 661 632 bytes (new) against 51 724 288 (torch formula): the weighted product [rows, K, d] and the
    formula's softmax / normalise intermediates are no longer kept.  Peak 105 156 608 against 114 378 752: the peak of the stage lies in the backward
    of the phi encoder's Linear layers (16 384 rows x 128), which both routes run; the new route builds the phi branch before the theta branch, so
    theta's backward is over and its saved activations are released before that point."""
    block, _ = make_block(16, 4, False, 91, num_patch=16)
    gen = torch.Generator().manual_seed(23)
    x_pred = torch.randn(1, 16, 32, 32, 32, generator=gen).to(DEV)
    x_retr = torch.randn(4, 16, 32, 32, 32, generator=gen).to(DEV)
    dout = torch.randn(1, 16, 32, 32, 32, generator=gen).to(DEV)

    def measure(fn):
        block.zero_grad(set_to_none=True)
        xp, xr = x_pred.clone().requires_grad_(True), x_retr.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        out = fn(xp, xr)
        held = torch.cuda.memory_allocated(DEV) - base
        out.backward(dout)
        torch.cuda.synchronize()
        return held, torch.cuda.max_memory_allocated(DEV) - base
    held_new, peak_new = measure(lambda xp, xr: block(xp, xr))
    held_old, peak_old = measure(lambda xp, xr: ref.torch_patched_forward(block, xp, xr, 0, 0, None))
    print('\nstage at C3 B = 1, bytes held after forward: new %d, torch formula %d; peak over forward + backward: new %d, torch formula %d'
          % (held_new, held_old, peak_new, peak_old))
    assert held_new < held_old
    assert peak_new < peak_old
