"""GPU: the refinement step (include/rfuse_step.h, csrc/refinement_step.hip, rfuse/training.py).

Head backward: against a float64 numpy evaluation of the header's arithmetic on the same float32 inputs -- g = fl32(dout * fl32(1 - out^2)) as the header
fixes it, everything after g in float64.  numpy has no fma: 1 - out^2 is evaluated in float64 and rounded to float32, which differs from the fma's single
rounding by one ulp in rare elements (a double rounding).  Bounds, from the prescribed roundings:
    |dh - ref| <= 4 * 2^-24 |ref|                        one float32 rounding of g * w, and that rare ulp of g
    |dw - ref| <= 2^-23 |ref| + 2^-30 sum |g h|          one float32 rounding of the sum, doubled for the rare ulp of g; float64 accumulation of up to 2^21
                                                         terms (2^21 * 2^-53 = 2^-32) -- the same form for db
Occupancy rows: exact equality with the torch formula (threshold, max_pool3d, unfold, any) on the same prediction.
Steps: ``RefinementStep`` against tests/refinement_step_ref.py in float64 on the CPU, the reference side given the step's own occupancy rows (a discrete
choice); loss and logged scalars within 1e-4 relative, the cosine of all optimised parameters' gradients above 0.9999 -- the bars of
tests/test_autograd_gpu.py:test_forward_full_trains_like_the_oracle.
"""
import numpy as np
import pytest
import torch

import helpers
import refinement_step_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FIX = helpers.load_fixture('refinement_step')


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU visible')
    return DEV


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- head backward
def head_shapes():
    from rfuse import _lib
    threads = _lib.load_step().rf_pointwise_tanh_backward_grid_threads()
    return [(1, 1, 4), (2, 16, 512), (3, 5, 268), (4, 12, 4096), (1, 16, 262144),
            (3, 2, 4 * (threads // 3 + 77)),            # more quads than the grid has threads: the stride loop runs twice, across sample boundaries
            (2, 40, 1028), (1, 32, 260)]                # more than one chunk of 16 channels: a ragged last chunk, and whole chunks only


def head_inputs(n, c, vox, seed):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, c, vox, generator=g).relu()
    out = torch.tanh(1.5 * torch.randn(n, 1, vox, generator=g))
    edge = np.float32(1) - np.float32(2.0 ** -24)
    out.view(-1)[::7] = float(edge)                                  # |out| up to 1 - 2^-24
    out.view(-1)[3::11] = -float(edge)
    dout = torch.randn(n, 1, vox, generator=g) * 0.01
    w = torch.randn(1, c, 1, 1, 1, generator=g)
    return h, out, dout, w


def head_reference(h, out, dout, w):
    """float64 numpy: dh, dw, db, and sum |g h| per channel, sum |g|, from g rounded to float32 as the header prescribes"""
    h64, o64, d64, w64 = (t.numpy().astype(np.float64) for t in (h, out, dout, w.reshape(-1)))
    one_minus = (1.0 - o64 * o64).astype(np.float32).astype(np.float64)                  # out^2 is exact in float64; the fma rounds 1 - out^2 once
    g = (d64 * one_minus).astype(np.float32).astype(np.float64)                          # the product of two float32 is exact in float64: one rounding
    return {'dh': g * w64[None, :, None], 'dw': (g * h64).sum((0, 2)), 'db': g.sum(), 'abs_dw': np.abs(g * h64).sum((0, 2)), 'abs_db': np.abs(g).sum()}


@pytest.mark.parametrize('case', range(8))
def test_head_backward_against_float64(gpu, case):
    from rfuse import ops
    n, c, vox = head_shapes()[case]
    h, out, dout, w = head_inputs(n, c, vox, 100 + case)
    r = head_reference(h, out, dout, w)
    args = [t.to(gpu) for t in (h, out, dout, w)]
    dh, dw, db = ops.pointwise_tanh_backward(*args)
    dh2, dw2, db2 = ops.pointwise_tanh_backward(*args)
    assert dh.shape == h.shape and dw.shape == w.shape and db.shape == (1,)
    assert torch.equal(bits(dh), bits(dh2)) and torch.equal(bits(dw), bits(dw2)) and torch.equal(bits(db), bits(db2)), 'two calls differ'
    e_dh = np.abs(dh.cpu().numpy().astype(np.float64) - r['dh'])
    worst = float((e_dh / np.maximum(np.abs(r['dh']), 1e-300)).max())
    e_dw = np.abs(dw.cpu().numpy().astype(np.float64).reshape(-1) - r['dw'])
    bound_dw = 2.0 ** -23 * np.abs(r['dw']) + 2.0 ** -30 * r['abs_dw']
    e_db = abs(float(db.cpu().double()) - r['db'])
    bound_db = 2.0 ** -23 * abs(r['db']) + 2.0 ** -30 * r['abs_db']
    print('\n(n, c, voxels) = %s: dh worst relative %.3e (bound %.3e); dw worst error / bound %.3f; db error / bound %.3f' % (
        (n, c, vox), worst, 4 * 2.0 ** -24, float((e_dw / np.maximum(bound_dw, 1e-300)).max()), e_db / max(bound_db, 1e-300)))
    assert np.all(e_dh <= 4 * 2.0 ** -24 * np.abs(r['dh']))
    assert np.all(e_dw <= bound_dw) and e_db <= bound_db


def test_head_backward_does_not_mask_non_finite(gpu):
    from rfuse import ops
    n, c, vox = 2, 16, 512
    h, out, dout, w = head_inputs(n, c, vox, 7)
    h = h + 0.25                                                     # no zero beside the Inf: Inf * h stays Inf or becomes NaN, never finite
    dout[0, 0, 37], dout[1, 0, 300] = float('nan'), float('inf')
    dh, dw, db = ops.pointwise_tanh_backward(*[t.to(gpu) for t in (h, out, dout, w)])
    dh = dh.cpu()
    assert torch.isnan(dh[0, :, 37]).all() and torch.isinf(dh[1, :, 300]).all()
    finite = torch.isfinite(dh)
    finite[0, :, 37], finite[1, :, 300] = True, True
    assert finite.all(), 'a non-finite gradient leaked to another voxel'
    assert not torch.isfinite(dw.cpu()).any() and not torch.isfinite(db.cpu()).any()
    clean = dout.clone()
    clean[0, 0, 37], clean[1, 0, 300] = 0.0, 0.0
    _, dw0, db0 = ops.pointwise_tanh_backward(*[t.to(gpu) for t in (h, out, clean, w)])
    assert torch.isfinite(dw0).all() and torch.isfinite(db0).all()


def test_head_backward_refuses_what_it_does_not_support(gpu):
    from rfuse import _lib, ops
    lib = _lib.load_step()
    assert lib.rf_pointwise_tanh_backward_ws_bytes(1, 16, 6) == 0 and lib.rf_pointwise_tanh_backward_ws_bytes(1, 65, 8) == 0
    assert lib.rf_pointwise_tanh_backward_ws_bytes(1, 64, 8) > 0 and lib.rf_pointwise_tanh_backward_ws_bytes(0, 4, 8) == 0
    for n, c, vox in ((1, 4, 6), (1, 65, 8)):
        with pytest.raises(NotImplementedError):
            ops.pointwise_tanh_backward(torch.zeros(n, c, vox, device=gpu), torch.zeros(n, 1, vox, device=gpu), torch.zeros(n, 1, vox, device=gpu),
                                        torch.zeros(1, c, 1, 1, 1, device=gpu))
    t = torch.zeros(64, device=gpu)
    with pytest.raises(RuntimeError, match='rc=-2'):
        lib.rf_pointwise_tanh_backward(ops._p(t), ops._p(t), ops._p(t), ops._p(t), 1, 4, 6, ops._p(t), ops._p(t), ops._p(t), ops._p(t), 4096, None)
    with pytest.raises(RuntimeError, match='rc=-4'):
        lib.rf_pointwise_tanh_backward(ops._p(t), ops._p(t), ops._p(t), ops._p(t), 1, 4, 8, ops._p(t), ops._p(t), ops._p(t), ops._p(t), 8, None)


def test_pointwise_tanh_function(gpu):
    """forward: the bits of ops.conv1x1_tanh; backward: the kernel's three outputs, and only those that are asked for"""
    from rfuse import ops
    from rfuse.autograd import PointwiseTanh
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 16, 8, 8, 8, generator=g).relu().to(gpu).requires_grad_(True)
    w = torch.randn(1, 16, 1, 1, 1, generator=g).to(gpu).requires_grad_(True)
    b = torch.randn(1, generator=g).to(gpu).requires_grad_(True)
    r = torch.randn(2, 1, 8, 8, 8, generator=g).to(gpu)
    y = PointwiseTanh.apply(x, w, b)
    with torch.no_grad():
        y0 = ops.conv1x1_tanh(x.detach(), w.detach(), b.detach())
    assert torch.equal(bits(y), bits(y0))
    (y * r).sum().backward()
    dh, dw, db = ops.pointwise_tanh_backward(x.detach(), y0, r, w.detach())
    assert torch.equal(bits(x.grad), bits(dh)) and torch.equal(bits(w.grad), bits(dw)) and torch.equal(bits(b.grad), bits(db))
    # against torch's own derivative of the broadcast formula the decoder used before
    xt, wt, bt = (t.detach().clone().double().requires_grad_(True) for t in (x, w, b))
    yt = torch.tanh((xt.unsqueeze(1) * wt.view(1, 1, 16, 1, 1, 1)).sum(dim=2) + bt.view(1, -1, 1, 1, 1))
    (yt * r.double()).sum().backward()
    for got, want in ((x.grad, xt.grad), (w.grad, wt.grad), (b.grad, bt.grad)):
        assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())
    w2 = w.detach().clone().requires_grad_(True)
    y2 = PointwiseTanh.apply(x.detach(), w2, b.detach())
    (y2 * r).sum().backward()
    assert torch.equal(bits(w2.grad), bits(dw))
    # a frozen head: the data gradient alone, with the same bits, in one launch (no sums, no second launch, no workspace)
    from rfuse import _lib
    x3 = x.detach().clone().requires_grad_(True)
    y3 = PointwiseTanh.apply(x3, w.detach(), b.detach())
    (y3 * r).sum().backward()
    assert torch.equal(bits(x3.grad), bits(dh))
    dh_only, none_w, none_b = ops.pointwise_tanh_backward(x.detach(), y0, r, w.detach(), sums=False)
    assert none_w is None and none_b is None and torch.equal(bits(dh_only), bits(dh))
    t = torch.zeros(64, device=gpu)
    with pytest.raises(RuntimeError, match='rc=-1'):                 # dw without db
        _lib.load_step().rf_pointwise_tanh_backward(ops._p(t), ops._p(t), ops._p(t), ops._p(t), 1, 4, 8, ops._p(t), ops._p(t), None, ops._p(t), 4096, None)
    # a head wider than the backward supports is refused in the forward, not at backward time
    with pytest.raises(NotImplementedError):
        PointwiseTanh.apply(torch.zeros(1, 65, 2, 2, 2, device=gpu).requires_grad_(True), torch.zeros(1, 65, 1, 1, 1, device=gpu), torch.zeros(1, device=gpu))


# ---------------------------------------------------------------------------------------------------- occupancy rows
VOXEL = 0.03125
TRUNC, THR = 3 * VOXEL, 0.75 * VOXEL          # the configs' ratio (3 voxels, 0.75 voxel) in powers of two: df = thr exactly at pred = -0.5


def occupancy_constants(shape):
    """alternately the pair above and a shipped config's own (no float32 prediction need map onto its threshold exactly)"""
    if sum(shape) % 2:
        c = ref.constants(ref.rf_configs.get_config('C3'))
        return c['trunc'], c['thr']
    return TRUNC, THR


def df32(p, trunc):
    return ((np.float32(p) + np.float32(1)) * np.float32(trunc)) / np.float32(2)


def threshold_neighbours(trunc, thr):
    """float32 predictions whose df is the largest value <= thr (equal to it where one exists) and the smallest value > thr, found on the host"""
    thr32 = np.float32(thr)
    p = np.float32(2 * thr / trunc - 1)
    while df32(p, trunc) <= thr32:
        p = np.nextafter(p, np.float32(2))
    while df32(p, trunc) > thr32:
        p = np.nextafter(p, np.float32(-2))
    at_or_below, above = p, np.nextafter(p, np.float32(2))
    assert df32(at_or_below, trunc) <= thr32 < df32(above, trunc)
    return float(at_or_below), float(np.nextafter(at_or_below, np.float32(-2))), float(above)      # one ulp of pred is at most one ulp of df here


def torch_rows(pred, trunc, thr, e):
    return ref.occupancy_rows(pred, trunc, thr, e)


@pytest.mark.parametrize('shape', [(1, 4, 1), (2, 8, 2), (3, 16, 2), (1, 64, 2), (2, 32, 4), (2, 12, 3)])
def test_occupancy_rows_equal_the_torch_formula(gpu, shape):
    from rfuse import ops
    n, edge, e = shape
    trunc, thr = occupancy_constants(shape)
    g = torch.Generator().manual_seed(sum(shape))
    block, r = (2 * e) ** 3, edge // (2 * e)
    # occupied voxels with probability ~ 1 / block: about 63 % of the rows hold one
    pred = torch.where(torch.rand(n, 1, edge, edge, edge, generator=g) < 1.0 / block, -0.9, 0.9) + 0.05 * torch.randn(n, 1, edge, edge, edge, generator=g)
    flat = pred.view(n, r, 2 * e, r, 2 * e, r, 2 * e)
    big = n * r ** 3 > 8
    taken = set()
    if big:
        taken = {(0, r - 1, r - 1, r - 1), (n - 1, r - 1, r - 1, 0)}
        flat[0, r - 1, :, r - 1, :, r - 1, :] = float('nan')         # a block of NaN: unoccupied
        flat[n - 1, r - 1, :, r - 1, :, 0, :] = float('nan')
        flat[n - 1, r - 1, 1, r - 1, 0, 0, 1] = -0.9                 # NaN beside an occupied voxel: occupied
    at, below, above = threshold_neighbours(trunc, thr)
    planted = []
    total = n * r ** 3
    free = [row for row in ((i * 5 + 3) % total for i in range(total)) if ((row // r ** 3, row // r ** 2 % r, row // r % r, row % r) not in taken)]
    for i, (v, row) in enumerate(zip([at, below, above, float('nan')] * 2, free)):     # each value alone in an otherwise empty block, at varying positions
        b, px, py, pz = row // r ** 3, row // r ** 2 % r, row // r % r, row % r
        flat[b, px, :, py, :, pz, :] = 0.9
        flat[b, px, i % (2 * e), py, (i * 3) % (2 * e), pz, (i * 7) % (2 * e)] = v
        planted.append((((b * r + px) * r + py) * r + pz, v))
    assert {v for _, v in planted if v == v} == {at, below, above}
    want = torch_rows(pred, trunc, thr, e)
    rows = ops.attn_occupancy_rows(pred.to(gpu), trunc, thr, e)
    assert rows.dtype == torch.bool and rows.shape == (n * r ** 3,)
    assert torch.equal(rows.cpu(), want)
    assert torch.equal(torch_rows(pred.to(gpu), trunc, thr, e).cpu(), want)          # torch on the device agrees with torch on the host
    for row, v in planted:
        assert bool(rows[row]) == (v in (at, below)), (row, v)
    if big:
        assert bool(rows[((0 * r + r - 1) * r + r - 1) * r + r - 1]) is False and bool(rows[(((n - 1) * r + r - 1) * r + r - 1) * r]) is True
        assert 0.3 < float(want.float().mean()) < 0.9


def test_occupancy_rows_single_voxel_sweep(gpu):
    """the only occupied voxel of row r sits at position r of its 4^3 block: all 64 positions are seen; an empty volume has no row"""
    from rfuse import ops
    pred = torch.full((1, 1, 16, 16, 16), 0.9)
    assert not ops.attn_occupancy_rows(pred.to(gpu), TRUNC, THR, 2).any()
    for keep in range(64):
        one = pred.clone()
        px, py, pz = keep // 16, (keep // 4) % 4, keep % 4
        one[0, 0, 4 * px + keep // 16, 4 * py + (keep // 4) % 4, 4 * pz + keep % 4] = -0.9
        rows = ops.attn_occupancy_rows(one.to(gpu), TRUNC, THR, 2).cpu()
        assert rows.nonzero().flatten().tolist() == [keep]
    every = pred.clone()
    for keep in range(64):
        px, py, pz = keep // 16, (keep // 4) % 4, keep % 4
        every[0, 0, 4 * px + keep // 16, 4 * py + (keep // 4) % 4, 4 * pz + keep % 4] = -0.9
    assert ops.attn_occupancy_rows(every.to(gpu), TRUNC, THR, 2).all()


def test_occupancy_rows_refuse_what_they_do_not_support(gpu):
    from rfuse import _lib, ops
    with pytest.raises(ValueError):
        ops.attn_occupancy_rows(torch.zeros(1, 1, 6, 6, 6, device=gpu), TRUNC, THR, 2)
    t = torch.zeros(512, device=gpu)
    with pytest.raises(RuntimeError, match='rc=-2'):
        _lib.load_step().rf_attn_occupancy_rows(ops._p(t), 1, 6, 2, TRUNC, THR, ops._p(t), None)


# ---------------------------------------------------------------------------------------------------- needs_input_grad
def test_conv_and_linear_backward_skip_what_is_not_asked_for(gpu):
    """a frozen weight: no weight-gradient launch, the data gradient keeps its bits; an input that is data: no data gradient, the weight gradient keeps its bits"""
    from model.unet import SingleConv
    from rfuse import _lib, ops
    from rfuse import autograd as rfa
    torch.manual_seed(3)
    layer = SingleConv(8, 16, num_groups=4).to(gpu)
    x0 = torch.randn(3, 8, 8, 8, 8, device=gpu).relu()
    r = torch.randn(3, 16, 8, 8, 8, device=gpu)
    lib = _lib.load()
    wgrads = {'rf_conv3d_k3_wgrad', 'rf_conv3d_k3_wgrad_split', 'rf_linear_wgrad'}

    def run(fn, params, x_grad, frozen):
        for p in params:
            p.grad = None
            p.requires_grad_(not any(p is f for f in frozen))
        x = x0.clone().requires_grad_(x_grad) if fn is layer else xl.clone().requires_grad_(x_grad)
        records = []
        lib.start_profile(records)
        try:
            y = fn(x)
            (y * (r if fn is layer else rl)).sum().backward()
        finally:
            lib.stop_profile()
            for p in params:
                p.requires_grad_(True)
        return x.grad, [p.grad for p in params], [rec[0] for rec in records]

    params = list(layer.parameters())
    dx, grads, names = run(layer, params, True, ())
    assert wgrads & set(names) and 'rf_gn_backward' in names
    dx_f, grads_f, names_f = run(layer, params, True, [layer.conv.weight])
    assert not wgrads & set(names_f) and torch.equal(bits(dx_f), bits(dx))
    assert [g is None for g in grads_f] == [p is layer.conv.weight for p in params]
    for g0, g1 in zip(grads, grads_f):
        assert g1 is None or torch.equal(bits(g0), bits(g1))
    dx_d, grads_d, names_d = run(layer, params, False, [layer.groupnorm.weight, layer.groupnorm.bias])
    iw = [i for i, p in enumerate(params) if p is layer.conv.weight][0]
    assert dx_d is None and 'rf_gn_backward' not in names_d and torch.equal(bits(grads_d[iw]), bits(grads[iw]))

    w = torch.nn.Parameter(torch.randn(32, 24, device=gpu) * 0.2)
    b = torch.nn.Parameter(torch.randn(32, device=gpu))
    xl, rl = torch.randn(70, 24, device=gpu), torch.randn(70, 32, device=gpu)
    linear = lambda x: rfa.Linear.apply(x, w, b, ops.ACT_LEAKY, 0.01)
    dx, grads, names = run(linear, [w, b], True, ())
    assert names.count('rf_linear_wgrad') == 1 and names.count('rf_linear') == 2
    dx_f, grads_f, names_f = run(linear, [w, b], True, [w, b])
    assert 'rf_linear_wgrad' not in names_f and torch.equal(bits(dx_f), bits(dx)) and grads_f == [None, None]
    dx_d, grads_d, names_d = run(linear, [w, b], False, ())
    assert dx_d is None and names_d.count('rf_linear') == 1 and all(torch.equal(bits(a), bits(c)) for a, c in zip(grads, grads_d))


# ---------------------------------------------------------------------------------------------------- the steps
WEIGHT_GRADIENTS = {'rf_conv3d_k3_wgrad', 'rf_conv3d_k3_wgrad_split', 'rf_conv3d_valid_wgrad', 'rf_linear_wgrad'}


class Problem:
    """one config: the drop-in modules on the GPU with the fixture's weights, the fixture's batch, and every step run once"""

    def __init__(self, cfg_name):
        from rfuse import _lib
        self.cfg_name = cfg_name
        self.mods = ref.make_modules(ref.rf_configs.get_config(cfg_name))
        shapes = {k: {n: tuple(v.shape) for n, v in m.state_dict().items()} for k, m in self.mods.items()}
        self.cfg, self.sds, self.data, self.noise = ref.problem(cfg_name, shapes)
        for k, m in self.mods.items():
            m.load_state_dict(self.sds[k])
            m.to(DEV).train()
        self.libs = [_lib.load(), _lib.load_train(), _lib.load_contrastive(), _lib.load_attn_train(), _lib.load_level(), _lib.load_step()]
        self.runs = {}
        torch.set_num_threads(min(32, torch.get_num_threads()))

    def step(self, phase):
        from rfuse.training import RefinementStep
        side = {k: ref.HPARAMS[k] for k in ('loss_side_task_retr', 'loss_side_task_unet')} if phase in (3, 'val') else {}
        return RefinementStep.from_config(self.cfg, 3 if phase == 'val' else phase, self.mods, **side)

    def batch(self):
        return {k: v.to(DEV) for k, v in self.data.items()}

    def run(self, phase):
        """-> the step's outputs (CPU), its gradients by parameter name, the launch log, the float64 reference's outputs and gradients"""
        if phase in self.runs:
            return self.runs[phase]
        step = self.step(phase)
        params = [p for m in self.mods.values() for p in m.parameters()]
        for p in params:
            p.grad = None
        flags = [p.requires_grad for p in params]
        noise = self.noise.to(DEV) if self.noise is not None else None
        records = []
        for lib in self.libs:
            lib.start_profile(records)
        try:
            if phase == 'val':
                from rfuse import metrics as rm
                metrics = [torch.nn.ModuleList([rm.IoU(compute_on_step=False), rm.Chamfer3D(compute_on_step=False), rm.Precision(compute_on_step=False),
                                                rm.Recall(compute_on_step=False)]).to(DEV) for _ in range(2)]
                out = step.validation_step(self.batch(), metrics[0], metrics[1], gumbel_noise=noise)
            else:
                metrics = None
                out = step.training_step(self.batch(), gumbel_noise=noise)
                assert out['loss'].is_cuda
                out['loss'].sum().backward()
        finally:
            for lib in self.libs:
                lib.stop_profile()
        torch.cuda.synchronize()
        res = {'step': step, 'metrics': metrics, 'launches': [rec[0] for rec in records], 'flags_kept': flags == [p.requires_grad for p in params],
               'out': {k: v.detach().cpu() for k, v in out.items()}, 'out_gpu': out,
               'grads': {net + '.' + n: (None if p.grad is None else p.grad.detach().cpu().double()) for net, m in self.mods.items() for n, p in m.named_parameters()}}
        leaves = ref.leaves(self.sds, torch.float64)
        data64 = {k: v.double() for k, v in self.data.items()}
        noise64 = self.noise.double() if self.noise is not None else None
        rows = res['out']['occupancy_attn'] if 'occupancy_attn' in res['out'] else None
        if phase == 'val':
            res['ref'] = ref.validation_step(leaves, self.cfg, data64, noise=noise64, rows_override=rows)
        else:
            res['ref'] = ref.training_step(phase, leaves, self.cfg, data64, noise=noise64, rows_override=rows)
            res['ref']['loss'].sum().backward()
        res['ref_grads'] = {net + '.' + n: v.grad for net, sd in leaves.items() for n, v in sd.items()}
        self.runs[phase] = res
        return res


_problems = {}


@pytest.fixture(scope='module')
def problem(gpu):
    def get(cfg_name):
        if cfg_name not in _problems:
            _problems[cfg_name] = Problem(cfg_name)
        return _problems[cfg_name]
    yield get
    _problems.clear()


def check_scalars(res, case):
    for name, want in res['ref'].items():
        if name.startswith('pred') or name.startswith('occ'):
            continue
        got = float(res['out'][name].double().sum())
        want = float(torch.as_tensor(want).detach().double().sum())
        print('%s %-18s step %.9g  float64 reference %.9g' % (case, name, got, want))
        if name == 'attn_occupancy':
            assert got == want
        else:
            assert abs(got - want) <= 1e-4 * abs(want), (name, got, want)
    assert set(k for k in res['ref'] if not k.startswith('occ_')) <= set(res['out'])


def check_gradients(res, case):
    dot = n1 = n2 = 0.0
    for name, p in res['step'].named_parameters():
        want, got = res['ref_grads'][name], res['grads'][name]
        if want is None:                                             # sig_scale / sig_shift: serialised, unused (reference model/attention.py:62-63)
            assert got is None or float(got.abs().max()) == 0.0, name
            continue
        assert got is not None, name
        dot, n1, n2 = dot + float((got * want).sum()), n1 + float((got * got).sum()), n2 + float((want * want).sum())
    cos = dot / np.sqrt(n1 * n2)
    print('%s cosine of the optimised parameters\' gradients %.8f' % (case, cos))
    assert cos > 0.9999
    optimised = {name for name, _ in res['step'].named_parameters()}
    assert all(g is None for name, g in res['grads'].items() if name not in optimised), 'a network outside parameters() received a gradient'


def check_occupancy(p, res, case):
    c, e = ref.constants(p.cfg), p.cfg['attn_patch_extent'] // 2
    rows = res['out']['occupancy_attn']
    assert rows.dtype == torch.bool
    own = ref.occupancy_rows(res['out_gpu']['pred_back'].detach(), c['trunc'], c['thr'], e).cpu()
    assert torch.equal(rows, own), 'the rows are not the torch formula of the step\'s own pred_back'
    pred64 = res['ref']['pred_back'].detach()
    ref_rows = ref.occupancy_rows(pred64, c['trunc'], c['thr'], e)
    near = ref.margin_rows(pred64, c['trunc'], c['thr'], e, 1e-4 * c['trunc'])
    differ = rows != ref_rows
    print('%s occupancy: %d rows occupied, %d differ from the float64 reference, %d rows have a voxel within the margin' % (case, int(rows.sum()), int(differ.sum()), int(near.sum())))
    assert not (differ & ~near).any()
    assert int(near.sum()) <= 0.007 * rows.numel()


@pytest.mark.parametrize('case', [('C3', 0), ('C3', 1), ('C3', 2), ('C3', 3), ('C1', 3)])
def test_training_step_is_the_references(problem, case):
    cfg_name, phase = case
    p = problem(cfg_name)
    res = p.run(phase)
    check_scalars(res, case)
    check_gradients(res, case)
    if phase >= 2:
        check_occupancy(p, res, case)
    assert res['flags_kept']
    if phase >= 2:
        # the same problem as the CPU fixture: against the reference's own float32 rows, no more differences than voxels lie within the margin
        theirs = torch.from_numpy(np.unpackbits(FIX['%s_p%d_occ' % case]).astype(bool))
        assert int((res['out']['occupancy_attn'] != theirs).sum()) <= int(FIX['%s_p%d_stats' % case][1])


def test_phase_1_leaves_the_frozen_decoder_alone(problem):
    p = problem('C3')
    res = p.run(1)
    assert all(g is None for name, g in res['grads'].items() if name.startswith('decoder.')) and res['flags_kept']
    assert all(q.requires_grad for q in p.mods['decoder'].parameters())
    assert all(res['grads'][name] is not None for name, _ in res['step'].named_parameters())
    assert not {'rf_pointwise_tanh_backward'} - set(res['launches'])                 # the head's data gradient runs: the retrieval backbone is behind it
    # a flag that was cleared before the call stays cleared after it
    from rfuse.training import RefinementStep
    q = p.mods['decoder'].network[1].bias
    q.requires_grad_(False)
    try:
        with RefinementStep.from_config(p.cfg, 1, p.mods)._frozen():
            assert not any(t.requires_grad for t in p.mods['decoder'].parameters())
        assert not q.requires_grad and p.mods['decoder'].network[1].weight.requires_grad
    finally:
        q.requires_grad_(True)


def test_phase_2_launches_no_weight_gradient_outside_the_attention(problem):
    p = problem('C3')
    launches = p.run(2)['launches']
    assert not {'rf_conv3d_k3_wgrad', 'rf_conv3d_k3_wgrad_split', 'rf_conv3d_valid_wgrad', 'rf_gn_backward', 'rf_pointwise_tanh_backward', 'rf_relu_backward',
                'rf_relu_backward_amax'} & set(launches)
    assert launches.count('rf_linear_wgrad') == 8                    # the eight Linear layers of theta and phi, nothing else
    assert launches.count('rf_attn_occupancy_rows') == 1
    full = p.run(3)['launches']                                      # the log does see them where they run
    assert {'rf_gn_backward', 'rf_pointwise_tanh_backward'} <= set(full) and {'rf_conv3d_k3_wgrad', 'rf_conv3d_k3_wgrad_split'} & set(full)
    assert full.count('rf_pointwise_tanh_backward') == 3 and full.count('rf_attn_occupancy_rows') == 1


def test_validation_step_is_the_references(problem):
    from rfuse import metrics as rm
    p = problem('C3')
    res = p.run('val')
    check_scalars(res, ('C3', 'val'))
    check_occupancy(p, res, ('C3', 'val'))
    assert not any(v.requires_grad for v in res['out_gpu'].values())
    c = ref.constants(p.cfg)
    step, out, batch = res['step'], res['out_gpu'], p.batch()
    target_occ = batch['target'] * c['std'] + c['mean'] <= c['thr']
    by_hand = [torch.nn.ModuleList([rm.IoU(compute_on_step=False), rm.Chamfer3D(compute_on_step=False), rm.Precision(compute_on_step=False),
                                    rm.Recall(compute_on_step=False)]).to(DEV) for _ in range(2)]
    for metrics, df in ((by_hand[0], (out['pred_shape'] + 1) * c['trunc'] / 2), (by_hand[1], batch['retrieval'][:, :1] * c['std'] + c['mean'])):
        for m in metrics:
            m(df <= c['thr'], target_occ)
    for got_list, want_list in zip(res['metrics'], by_hand):
        for got, want in zip(got_list, want_list):
            for name in got._state_names():
                assert torch.equal(getattr(got, name), getattr(want, name)), (type(got).__name__, name)
    # (with the fixture's seeds the target's occupancy is empty: Chamfer3D skips the volume, IoU, Precision and Recall count it)
    assert all(float(metrics[0].total) == 1 for metrics in res['metrics'])
    # the grid fed to the fuse metrics against the float64 reference's: equal but for voxels within the margin of the threshold
    occ = ((out['pred_shape'] + 1) * c['trunc'] / 2 <= c['thr']).cpu()
    near = (ref.network_pred_to_df(res['ref']['pred_shape'], c['trunc']) - c['thr']).abs() <= 1e-4 * c['trunc']
    assert not ((occ != res['ref']['occ_full']) & ~near).any()


def test_validation_metrics_see_prediction_and_target(problem):
    """the fixture's target has no voxel under 0.75 voxel, so its metric states cannot tell a prediction from a target.  Here the target is scaled so that
    about a quarter of its voxels are occupied: the states equal rfuse.metrics called by hand, and differ from the same call with the two swapped"""
    from rfuse import metrics as rm
    p = problem('C3')
    c = ref.constants(p.cfg)
    batch = p.batch()
    batch['target'] = ((batch['target'] - c['mean']) / c['std']).contiguous()          # denormalises to rand * trunc: a quarter of it is <= 0.75 voxel = trunc / 4
    make = lambda: torch.nn.ModuleList([rm.IoU(compute_on_step=False), rm.Chamfer3D(compute_on_step=False), rm.Precision(compute_on_step=False),
                                        rm.Recall(compute_on_step=False)]).to(DEV)
    fuse, nn1, hand, swapped = make(), make(), make(), make()
    out = p.step('val').validation_step(batch, fuse, nn1, gumbel_noise=None)
    target_occ = batch['target'] * c['std'] + c['mean'] <= c['thr']
    pred_occ = (out['pred_shape'] + 1) * c['trunc'] / 2 <= c['thr']
    assert 0.15 < float(target_occ.float().mean()) < 0.35 and int(pred_occ.sum()) > 0 and int((pred_occ & target_occ).sum()) > 0
    for m, s in zip(hand, swapped):
        m(pred_occ, target_occ)
        s(target_occ, pred_occ)
    states = lambda ms: [float(getattr(m, name)) for m in ms for name in m._state_names()]
    assert states(fuse) == states(hand) and states(fuse) != states(swapped)
    assert all(float(m.total) == 1 for m in fuse) and all(float(m.total) == 1 for m in nn1)
    by_hand_nn1 = make()
    for m in by_hand_nn1:
        m(batch['retrieval'][:, :1] * c['std'] + c['mean'] <= c['thr'], target_occ)
    assert states(nn1) == states(by_hand_nn1)


def test_two_adam_steps(problem):
    """phase 3 with rfuse.optim.Adam over step.parameters(): finite losses, the parameters move (their version counters change)"""
    from rfuse.optim import Adam
    from rfuse.training import RefinementStep
    p = problem('C3')
    mods = ref.make_modules(p.cfg)
    for k, m in mods.items():
        m.load_state_dict(p.sds[k])
        m.to(DEV).train()
    step = RefinementStep.from_config(p.cfg, 3, mods, loss_side_task_retr=0.5, loss_side_task_unet=0.25)
    opt = Adam(step.parameters(), lr=1e-4)
    used = [q for n, q in step.named_parameters() if not n.endswith(('sig_scale', 'sig_shift'))]
    versions = [q._version for q in used]
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        out = step.training_step(p.batch())
        out['loss'].sum().backward()
        opt.step()
        losses.append(float(out['loss'].detach().sum()))
    print('two phase-3 steps: losses', losses)
    assert all(np.isfinite(v) for v in losses)
    assert all(q._version > v for q, v in zip(used, versions))
    assert all(torch.isfinite(q).all() for q in used)
