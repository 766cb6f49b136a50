"""Kernel level: the backward of the patch encoders' valid strided conv + bias + LeakyReLU 0.2 (csrc/conv_valid_backward.hip) against float64 CPU
autograd of ``F.leaky_relu(F.conv3d(x, W, b, stride), 0.2)`` on every layer shape of the shipped encoders (rfuse/configs.py: Patch08, Patch32,
PCPatch48 nf 12 and nf 10, Patch24V2, Patch24).  dx, dW and db each within a relative max error of 1e-4; the planes of x no output reads exactly 0;
repeated calls and calls beside a foreign F16-MFMA load bit-equal; NaN in x or dy where float64 torch puts it."""
import pytest
import torch
import torch.nn.functional as F

import testkit

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# (cin, cout, k, stride, input edge)
LAYERS = sorted({
    # Patch08 nf 16 (C4 query)
    (1, 16, 3, 1, 8), (16, 64, 3, 1, 6), (64, 64, 3, 1, 4), (64, 128, 2, 1, 2),
    # Patch32 nf 8 (C1-C4 target)
    (1, 8, 5, 1, 32), (8, 16, 3, 1, 28), (16, 32, 3, 2, 26), (32, 64, 3, 1, 12), (64, 64, 3, 2, 10), (64, 64, 4, 1, 4),
    # PCPatch48 nf 12 (C5 query)
    (1, 12, 5, 1, 48), (12, 24, 3, 1, 44), (24, 48, 3, 2, 42), (48, 48, 3, 2, 20), (48, 96, 3, 2, 9), (96, 96, 3, 1, 4), (96, 96, 2, 1, 2),
    # Patch24V2 nf 12 (C5 target)
    (1, 12, 3, 1, 24), (12, 24, 3, 1, 22), (24, 24, 3, 2, 20), (24, 48, 3, 1, 9), (48, 96, 3, 1, 7), (96, 96, 3, 1, 5), (96, 96, 3, 1, 3),
    # PCPatch48 nf 10 (channels not multiples of 4)
    (1, 10, 5, 1, 48), (10, 20, 3, 1, 44), (20, 40, 3, 2, 42), (40, 40, 3, 2, 20), (40, 80, 3, 2, 9), (80, 80, 3, 1, 4), (80, 80, 2, 1, 2),
    # Patch24 nf 12
    (1, 12, 5, 1, 24), (12, 24, 3, 1, 20), (24, 24, 3, 2, 18), (24, 48, 3, 1, 8), (48, 96, 3, 1, 6), (96, 96, 3, 1, 4),
})


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    from rfuse import ops as o
    return o


def problem(cin, cout, k, stride, s, n, seed, dy_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    bound = 1.0 / (cin * k ** 3) ** 0.5
    x = torch.randn(n, cin, s, s, s, generator=g, dtype=torch.float64)
    w = (torch.rand(cout, cin, k, k, k, generator=g, dtype=torch.float64) * 2 - 1) * bound
    b = (torch.rand(cout, generator=g, dtype=torch.float64) * 2 - 1) * bound
    so = (s - k) // stride + 1
    dy = torch.randn(n, cout, so, so, so, generator=g, dtype=torch.float64) * dy_scale
    return x.float().double(), w.float().double(), b.float().double(), dy.float().double()


def reference(x, w, b, dy, stride):
    x, w, b = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = F.leaky_relu(F.conv3d(x, w, b, stride=stride), 0.2)
    y.backward(dy)
    return y.detach(), x.grad, w.grad, b.grad


def run_gpu(ops, x, w, y, dy, k, stride, need_dx=True):
    xg, yg, dyg, wg = (t.float().contiguous().to(DEV) for t in (x, y, dy, w))
    dz, db = ops.conv3d_valid_leaky_backward(dyg, yg, 0.2)
    dx = ops.conv3d_valid_dgrad(dz, ops.pack_convv_dgrad_weight(wg), x.shape[1], k, stride, x.shape[2]) if need_dx else None
    dw = ops.conv3d_valid_wgrad(xg, dz, k, stride)
    return dx, dw, db


def rel(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check_layer(ops, cin, cout, k, stride, s, n, seed, dy_scale=1.0):
    x, w, b, dy = problem(cin, cout, k, stride, s, n, seed, dy_scale)
    y, rdx, rdw, rdb = reference(x, w, b, dy, stride)
    dx, dw, db = run_gpu(ops, x, w, y, dy, k, stride, need_dx=cin > 1)
    torch.cuda.synchronize()
    what = f'{cin}->{cout} k{k} s{stride} @{s} n{n} x{dy_scale:g}'
    if dx is not None:
        assert rel(dx, rdx) < 1e-4, (what, 'dx', rel(dx, rdx))
        so = (s - k) // stride + 1
        last = (so - 1) * stride + k                     # planes at and past `last` are read by no output
        if last < s:
            dxc = dx.cpu()
            assert torch.all(dxc[:, :, last:] == 0) and torch.all(dxc[:, :, :, last:] == 0) and torch.all(dxc[..., last:] == 0), (what, 'unread planes')
            assert torch.all(rdx[:, :, last:] == 0)
    assert rel(dw, rdw) < 1e-4, (what, 'dW', rel(dw, rdw))
    assert rel(db, rdb) < 1e-4, (what, 'db', rel(db, rdb))


@pytest.mark.parametrize('cin,cout,k,stride,s', LAYERS)
def test_layer_gradients_match_float64(ops, cin, cout, k, stride, s):
    check_layer(ops, cin, cout, k, stride, s, n=2 + (cin + cout + s) % 3, seed=cin * 1000 + cout * 10 + s)


@pytest.mark.parametrize('cin,cout,k,stride,s', [(1, 12, 5, 1, 48), (12, 24, 3, 1, 44), (24, 48, 3, 2, 42), (10, 20, 3, 1, 44), (96, 96, 2, 1, 2)])
def test_single_sample(ops, cin, cout, k, stride, s):
    check_layer(ops, cin, cout, k, stride, s, n=1, seed=7)


@pytest.mark.parametrize('cin,cout,k,stride,s', [(12, 24, 3, 1, 44), (24, 48, 3, 2, 42), (8, 16, 3, 1, 28), (16, 32, 3, 2, 26)])
def test_large_batch(ops, cin, cout, k, stride, s):
    """many K slices in the weight gradient, many workgroups per channel in db"""
    check_layer(ops, cin, cout, k, stride, s, n=12, seed=11)


@pytest.mark.parametrize('scale', [1e-9, 3e7])
@pytest.mark.parametrize('cin,cout,k,stride,s', [(12, 24, 3, 1, 44), (24, 48, 3, 2, 42), (20, 40, 3, 2, 42), (64, 64, 4, 1, 4)])
def test_scaled_upstream_gradient(ops, cin, cout, k, stride, s, scale):
    """NT-Xent hands the encoders gradients of 1e-3 ... 1e-7: relative accuracy must not depend on the gradient's magnitude"""
    check_layer(ops, cin, cout, k, stride, s, n=2, seed=5, dy_scale=scale)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize('cin,cout,k,stride,s', [(12, 24, 3, 1, 44), (24, 48, 3, 2, 42), (10, 20, 3, 1, 44), (64, 64, 3, 2, 10)])
def test_backward_is_bit_reproducible(ops, cin, cout, k, stride, s):
    x, w, b, dy = problem(cin, cout, k, stride, s, 3, seed=3)
    y = reference(x, w, b, dy, stride)[0]
    first = run_gpu(ops, x, w, y, dy, k, stride)
    second = run_gpu(ops, x, w, y, dy, k, stride)
    for a, c, name in zip(first, second, ('dx', 'dW', 'db')):
        assert torch.equal(_bits(a), _bits(c)), name


def test_backward_keeps_its_bits_beside_f16_mfma(ops):
    """the backward kernels on a side stream, ten times beside testkit's F16-MFMA load, return their solo bits (the two-stream hazard family)"""
    cases = [(12, 24, 3, 1, 44, 3), (24, 48, 3, 2, 42, 2), (10, 20, 3, 1, 20, 2), (64, 64, 4, 1, 4, 8)]
    prepared = []
    for cin, cout, k, stride, s, n in cases:
        x, w, b, dy = problem(cin, cout, k, stride, s, n, seed=cin + cout)
        y = reference(x, w, b, dy, stride)[0]
        prepared.append((x, w, y, dy, k, stride, run_gpu(ops, x, w, y, dy, k, stride)))
    torch.cuda.synchronize()
    main, side = torch.cuda.current_stream(), torch.cuda.Stream(DEV)
    scratch = torch.empty(256 * 256, dtype=torch.float32, device=DEV)
    bad = []
    for rep in range(10):
        for i, (x, w, y, dy, k, stride, solo) in enumerate(prepared):
            side.wait_stream(main)
            testkit.f16_mfma_load(main, scratch, iters=4000)
            with torch.cuda.stream(side):
                out = run_gpu(ops, x, w, y, dy, k, stride)
            main.wait_stream(side)
            torch.cuda.synchronize()
            for a, c, name in zip(out, solo, ('dx', 'dW', 'db')):
                if not torch.equal(_bits(a), _bits(c)):
                    bad.append((rep, cases[i], name))
    assert not bad, bad


@pytest.mark.parametrize('where', ['x', 'dy'])
@pytest.mark.parametrize('cin,cout,k,stride,s', [(12, 24, 3, 1, 22), (24, 48, 3, 2, 20), (10, 20, 3, 2, 9)])
def test_nan_lands_where_float64_torch_puts_it(ops, cin, cout, k, stride, s, where):
    x, w, b, dy = problem(cin, cout, k, stride, s, 2, seed=9)
    if where == 'x':
        x[1, cin // 2, s // 2, 1, s - 2] = float('nan')
    else:
        dy[0, cout - 1, 1, dy.shape[3] // 2, 0] = float('nan')
        dy[1, 0, -1, -1, -1] = float('inf')
    y, rdx, rdw, rdb = reference(x, w, b, dy, stride)
    dx, dw, db = run_gpu(ops, x, w, y, dy, k, stride)
    torch.cuda.synchronize()
    for got, ref, name in ((dx, rdx, 'dx'), (dw, rdw, 'dW'), (db, rdb, 'db')):
        got = got.double().cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (name, int((torch.isnan(got) != torch.isnan(ref)).sum()))
        assert torch.equal(torch.isinf(got), torch.isinf(ref)), name
        fin = torch.isfinite(ref)
        if fin.any():
            err = float((got[fin] - ref[fin]).abs().max() / ref[fin].abs().max().clamp_min(1e-300))
            assert err < 1e-4, (name, err)
