"""GPU: ``rfuse.optim.Adam`` (rfuse/optim.py, csrc/optim.hip, include/rfuse_optim.h) against the float64 restatement of tests/optim_ref.py.

Every case runs 7 steps and compares p, m and v after EACH step with ``optim_ref.adam_f64`` started from the kernel's own float32 state before that step.
The tolerance is not a fixed number.  For each tensor and each of p, m, v, ``diff32`` is the max-abs distance of torch's CPU float32 Adam
(``foreach=False``) from the same float64 result on the same inputs, and the kernel must stay within 4 x diff32 (``optim_ref.bar``): a correct float32
evaluation is a chain of at most eight roundings; a kernel may fuse other operations than torch's CPU kernels do, at most 2 x; both sides are maxima over
thousands of elements, another 2 x.  Where diff32 is 0 the kernel must equal the rounded float64 result.  No bit-equality with torch is
claimed (its own CPU and GPU kernels differ in the last bit), and a bar relative to |m| or |p| alone would be wrong: m + 0.1 (g - m) and g + wd p cancel.

The bar rests on maxima over thousands of elements; on a tensor of one element it compares two single rounding errors, and an evaluation that rounds
where torch's CPU kernels fuse (lerp, addcmul, add with alpha) misses it there whenever torch's errors happen to cancel.  The kernel therefore has torch's
CPU sequence of roundings, its three fused multiply-adds included (include/rfuse_optim.h): m and v come out with torch's CPU bits and p differs in the few
elements where torch's vectorised CPU sqrt is not correctly rounded, so the ratio is 1 at every size (optim_ref.opwise_f32 on the CPU, 40 seeds x 4 gradient
scales x 2 weight decays x 7 steps at 1, 3, 4, 5, 63, 64, 65 and 5000 elements).  ``test_kernel_is_the_headers_sequence_bit_for_bit`` holds every element
count, aligned or not, to the header's sequence exactly.  Where the shapes are the test's to choose the tensors have a few thousand elements.
"""
import math

import pytest
import torch

import optim_ref as oref
import testkit

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
STEPS = 7
KW = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)


@pytest.fixture(scope='module')
def Adam():
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    from rfuse.optim import Adam as cls
    return cls


@pytest.fixture(scope='module')
def limits(Adam):
    from rfuse import _lib
    lib = _lib.load_optim()
    return lib.rf_adam_step_max_tensors(), lib.rf_adam_step_segment()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def make_params(sizes, seed, device=DEV):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).to(device)) for n in sizes]


def set_grads(params, seed, scale=1.0, skip=()):
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(params):
        grad = torch.randn(p.shape, generator=g) * scale            # drawn for skipped ones too: the others' values do not depend on `skip`
        p.grad = None if i in skip else grad.to(p.device)


def snap(opt, p):
    st = opt.state.get(p, {})
    if len(st) == 0:
        return p.detach().cpu().clone(), torch.zeros(p.shape), torch.zeros(p.shape), 0
    return p.detach().cpu().clone(), st['exp_avg'].detach().cpu().clone(), st['exp_avg_sq'].detach().cpu().clone(), int(st['step'])


class Worst:
    ratio, at = 0.0, ''


def checked_step(opt, what, worst=None, misses=None):
    """one ``opt.step()`` (rfuse's class or torch's, on GPU parameters), every tensor of every group held to the bar from its own state before the step; a
    parameter without a gradient keeps its bits and its step count.  ``misses``: a list that collects the bar's failures instead of stopping at the first"""
    rows = [(grp, p) for grp in opt.param_groups for p in grp['params']]
    before = [snap(opt, p) for _, p in rows]
    grads = [None if p.grad is None else p.grad.detach().cpu().contiguous().clone() for _, p in rows]
    opt.step()
    torch.cuda.synchronize()
    for i, ((grp, p), (p0, m0, v0, t0), grad) in enumerate(zip(rows, before, grads)):
        p1, m1, v1, t1 = snap(opt, p)
        if grad is None:
            assert t1 == t0, '%s: tensor %d has no gradient, its step went from %d to %d' % (what, i, t0, t1)
            for a, b, name in ((p1, p0, 'p'), (m1, m0, 'm'), (v1, v0, 'v')):
                assert torch.equal(bits(a), bits(b)), '%s: tensor %d has no gradient, its %s changed' % (what, i, name)
            continue
        assert t1 == t0 + 1, (what, i, t0, t1)
        st = opt.state[p]
        assert st['step'].device.type == 'cpu' and st['step'].dtype == torch.float32 and st['step'].shape == ()
        args = (p0, grad, m0, v0, t0, float(grp['lr']), tuple(grp['betas']), grp['eps'], grp['weight_decay'])
        ref, cpu32 = oref.adam_f64(*args), oref.torch_adam(*args)
        for got, c, r, name in zip((p1, m1, v1), cpu32, ref, 'pmv'):
            where = '%s, tensor %d (%d elements), %s after step %d' % (what, i, p.numel(), name, t1)
            try:
                err, diff32 = oref.bar(got, c, r, where)
            except AssertionError as e:
                if misses is None:
                    raise
                misses.append(str(e))
                continue
            if worst is not None and diff32 > 0 and err / diff32 > worst.ratio:
                worst.ratio, worst.at = err / diff32, where


def run_checked(opt, params, what, seed, scale=1.0, skip_on=None, before_step=None):
    worst, misses = Worst(), []
    for step in range(STEPS):
        if before_step is not None:
            before_step(step)
        set_grads(params, seed * 100 + step, scale, skip=(skip_on or {}).get(step, ()))
        checked_step(opt, '%s, step %d' % (what, step), worst, misses)
    print('\n%s: worst error / diff32 inside the bar = %.3f (%s)' % (what, worst.ratio, worst.at))
    assert not misses, '%d of the comparisons miss the bar:\n  %s' % (len(misses), '\n  '.join(misses))
    return worst


def element_counts(limits):
    seg = limits[1]
    return [1, 3, 4, 5, 63, 64, 65, seg - 1, seg, seg + 1, 2 * seg + 1, 1000003]


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize('weight_decay', [0.0, 5e-5])
def test_every_element_count(Adam, limits, weight_decay):
    """1, 3, 4, 5, 63, 64, 65, one segment - 1 / exact / + 1, two segments + 1 and 1 000 003 elements in one parameter list: the 16-byte body, the 4-byte
    tail, one and several workgroups per tensor.

    The bar is applied tensor by tensor as everywhere else, and every miss of the 7 steps is listed, not only the first."""
    params = make_params(element_counts(limits), seed=1)
    opt = Adam(params, **dict(KW, weight_decay=weight_decay))
    run_checked(opt, params, 'element counts, weight decay %g' % weight_decay, seed=2)


def test_kernel_is_the_headers_sequence_bit_for_bit(Adam, limits):
    """include/rfuse_optim.h states the update as a sequence of correctly rounded float32 operations: the kernel returns the bits of that sequence evaluated
    with one torch CPU float32 operation each (optim_ref.opwise_f32) -- every element count, 16-byte aligned or a view at element offset 1, with and
    without weight decay, both branches of lerp"""
    sizes = element_counts(limits)[:-1] + [100003]
    for kw in (KW, dict(KW, weight_decay=5e-5), dict(KW, betas=(0.4, 0.99), eps=1e-6, weight_decay=1e-2)):
        aligned = make_params(sizes, seed=3)
        g = torch.Generator().manual_seed(4)
        bufs = [torch.randn(n + 4, generator=g).to(DEV) for n in sizes]
        views = [torch.nn.Parameter(b[1:1 + n]) for b, n in zip(bufs, sizes)]
        assert all(p.data_ptr() % 16 == 4 and p.is_contiguous() for p in views)
        params = aligned + views
        opt = Adam(params, **kw)
        for step in range(3):
            set_grads(params, 50 + step, scale=10.0 ** (-3 * step))
            before = [snap(opt, p) for p in params]
            grads = [p.grad.detach().cpu().clone() for p in params]
            opt.step()
            torch.cuda.synchronize()
            for i, (p, (p0, m0, v0, t0), grad) in enumerate(zip(params, before, grads)):
                want = oref.opwise_f32(p0, grad, m0, v0, t0, kw['lr'], kw['betas'], kw['eps'], kw['weight_decay'])
                for got, w, name in zip(snap(opt, p)[:3], want, 'pmv'):
                    assert torch.equal(bits(got), bits(w)), 'betas %s, step %d, tensor %d (%d elements, %s): %s differs at %d elements' % (
                        kw['betas'], step, i, p.numel(), 'aligned' if i < len(sizes) else 'offset 1', name, int((bits(got) != bits(w)).sum()))


def test_launch_boundaries_inside_the_list(Adam, limits):
    """3 x rf_adam_step_max_tensors() + 1 tensors: four launches, the last one of a single tensor"""
    count = 3 * limits[0] + 1
    params = make_params([2048 + 37 * (i % 29) for i in range(count)], seed=5)
    opt = Adam(params, **dict(KW, weight_decay=5e-5))
    run_checked(opt, params, '%d tensors' % count, seed=6)


@pytest.mark.parametrize('offset', [1, 2, 3])
def test_views_at_odd_element_offsets(Adam, limits, offset):
    """parameters AND gradients that are views at element offset 1, 2 or 3 of a larger buffer (4-byte accesses throughout), beside an aligned tensor in the
    same launch; the neighbours of every view in its buffer keep their bits"""
    seg = limits[1]
    sizes = [3001, 2 * seg + 5, 4099]
    g = torch.Generator().manual_seed(7 + offset)
    bufs = [torch.randn(n + 8, generator=g).to(DEV) for n in sizes]
    gbufs = [torch.zeros(n + 8, device=DEV) for n in sizes]
    guard = [b.clone() for b in bufs]
    params = [torch.nn.Parameter(b[offset:offset + n]) for b, n in zip(bufs, sizes)] + make_params([4096], seed=8)
    assert all(p.data_ptr() % 16 == 4 * offset for p in params[:3]) and params[3].data_ptr() % 16 == 0
    opt = Adam(params, **dict(KW, weight_decay=5e-5))
    worst = Worst()
    for step in range(STEPS):
        set_grads(params, 900 + step)
        for p, gb, n in zip(params[:3], gbufs, sizes):
            gb[offset:offset + n].copy_(p.grad)
            p.grad = gb[offset:offset + n]
            assert p.grad.data_ptr() % 16 == 4 * offset
        checked_step(opt, 'views at offset %d, step %d' % (offset, step), worst)
    print('\nviews at offset %d: worst error / diff32 = %.3f (%s)' % (offset, worst.ratio, worst.at))
    for b, w, n in zip(bufs, guard, sizes):
        assert torch.equal(bits(b[:offset]), bits(w[:offset])) and torch.equal(bits(b[offset + n:]), bits(w[offset + n:])), 'a write outside the view'


def test_non_contiguous_gradient_is_made_contiguous(Adam):
    params = [torch.nn.Parameter(torch.randn(64, 48, generator=torch.Generator().manual_seed(9)).to(DEV))]
    opt = Adam(params, **KW)
    for step in range(3):
        grad = torch.randn(48, 64, generator=torch.Generator().manual_seed(10 + step)).to(DEV).t()
        assert not grad.is_contiguous()
        params[0].grad = grad
        checked_step(opt, 'transposed gradient, step %d' % step)


@pytest.mark.parametrize('weight_decay', [0.0, 5e-5])
@pytest.mark.parametrize('scale', [1e-9, 1e-4, 1.0, 3e7])
def test_gradient_scales(Adam, limits, scale, weight_decay):
    """NT-Xent hands the encoders gradients of 1e-3 ... 1e-7; 3e7 squares to 1e15 in v"""
    params = make_params([4099, 2 * limits[1] + 3], seed=11)
    opt = Adam(params, **dict(KW, weight_decay=weight_decay))
    run_checked(opt, params, 'gradient scale %g, weight decay %g' % (scale, weight_decay), seed=12, scale=scale)


def test_warm_up_lr_sequence(Adam):
    """trainer/train_retrieval.py:46-49: before every step, pg['lr'] = min(1, (global_step + 1) / 1500) * lr in every group; the last steps sit across the
    end of the warm-up"""
    params = make_params([4099, 3001], seed=13)
    opt = Adam(params, lr=1e-4, weight_decay=5e-5)
    global_steps = [0, 1, 2, 3, 1498, 1499, 1500]
    seen = []

    def warm_up(step):
        lr_scale = min(1., float(global_steps[step] + 1) / 1500.)
        for pg in opt.param_groups:
            pg['lr'] = lr_scale * 1e-4
        seen.append(opt.param_groups[0]['lr'])
    run_checked(opt, params, 'warm-up', seed=14, before_step=warm_up)
    assert seen[0] == 1e-4 / 1500 and seen[-2:] == [1e-4, 1e-4] and len(set(seen)) == 6


def test_scheduler_drives_the_groups(Adam):
    params = make_params([3001], seed=15)
    opt = Adam(params, lr=1e-3)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 4], gamma=0.5)
    lrs = []
    for step in range(STEPS):
        set_grads(params, 1600 + step)
        lrs.append(opt.param_groups[0]['lr'])
        checked_step(opt, 'MultiStepLR, step %d' % step)
        sched.step()
    assert lrs == [1e-3, 1e-3, 5e-4, 5e-4, 2.5e-4, 2.5e-4, 2.5e-4]


def test_grad_none_skips_the_parameter(Adam):
    """a parameter whose grad is None on steps 2 and 5: its three tensors keep their bits, its step does not advance (checked_step), the others go on"""
    params = make_params([4099, 3001, 2053], seed=17)
    opt = Adam(params, **dict(KW, weight_decay=5e-5))
    run_checked(opt, params, 'grad None on steps 2 and 5', seed=18, skip_on={2: (1,), 5: (1,)})
    assert [int(opt.state[p]['step']) for p in params] == [7, 5, 7]
    for p in params:
        p.grad = None
    versions = [p._version for p in params]
    opt.step()                                                       # nothing has a gradient: no launch, nothing changes
    assert [p._version for p in params] == versions and [int(opt.state[p]['step']) for p in params] == [7, 5, 7]


def test_empty_parameter_keeps_torchs_bookkeeping(Adam):
    """a parameter of no elements that has a gradient gets its state and its step advances, as under torch.optim.Adam: the state dicts agree"""
    sizes = [0, 3001]
    mine, ref = make_params(sizes, seed=37), make_params(sizes, seed=37)
    opt, topt = Adam(mine, **KW), torch.optim.Adam(ref, **KW)
    for step in range(2):
        set_grads(mine, 3800 + step)
        set_grads(ref, 3800 + step)
        opt.step()
        topt.step()
    a, b = opt.state_dict()['state'], topt.state_dict()['state']
    assert set(a) == set(b) == {0, 1}
    for k in a:
        assert float(a[k]['step']) == float(b[k]['step']) == 2.0 and a[k]['exp_avg'].shape == b[k]['exp_avg'].shape and a[k]['exp_avg_sq'].shape == b[k]['exp_avg_sq'].shape
    only = make_params([0], seed=38)
    only[0].grad = torch.zeros_like(only[0])
    lone = Adam(only, **KW)
    lone.step()                                                      # nothing to launch
    assert float(lone.state[only[0]]['step']) == 1.0


def test_two_parameter_groups(Adam):
    params = make_params([4099, 3001, 2053, 2500], seed=19)
    opt = Adam([dict(params=params[:2]), dict(params=params[2:], lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=5e-5)], **KW)
    assert [g['lr'] for g in opt.param_groups] == [1e-3, 3e-4]
    run_checked(opt, params, 'two groups', seed=20)
    low = Adam(make_params([3001], seed=21), lr=1e-3, betas=(0.4, 0.9))          # 1 - beta1 >= 0.5: lerp's other branch
    run_checked(low, low.param_groups[0]['params'], 'beta1 0.4', seed=22)


@pytest.mark.parametrize('weight_decay', [0.0, 5e-5])
@pytest.mark.parametrize('where', ['g', 'p'])
def test_non_finite_values_land_where_torch_puts_them(Adam, limits, where, weight_decay):
    """NaN, +inf and -inf in single elements of the gradient (first step) or of the parameter: the NaN / +inf / -inf masks of p, m and v equal torch CPU's
    element for element after every step, every other element stays within the bar (optim_ref.bar checks both)"""
    seg = limits[1]
    sizes = [4099, seg + 7]
    spots = {0: [(5, float('nan')), (2048, float('inf')), (4098, float('-inf'))], 1: [(0, float('-inf')), (seg + 6, float('nan')), (seg - 1, float('inf'))]}
    params = make_params(sizes, seed=23)
    if where == 'p':
        with torch.no_grad():
            for i, marks in spots.items():
                for at, value in marks:
                    params[i][at] = value
    opt = Adam(params, **dict(KW, weight_decay=weight_decay))
    for step in range(STEPS):
        set_grads(params, 2400 + step)
        if where == 'g' and step == 0:
            for i, marks in spots.items():
                for at, value in marks:
                    params[i].grad[at] = value
        checked_step(opt, 'non-finite %s, weight decay %g, step %d' % (where, weight_decay, step))
    for i, marks in spots.items():
        p = params[i].detach().cpu()
        assert not torch.isfinite(p[[at for at, _ in marks]]).any() and int((~torch.isfinite(p)).sum()) == 3, 'the marks stay where they were put, and alone'


# ------------------------------------------------------------------------------------------------ the same bits on every call
def stepped(Adam, sizes, steps, stream=None, seed=25):
    params = make_params(sizes, seed=seed)
    opt = Adam(params, **dict(KW, weight_decay=5e-5))
    grads = []
    for step in range(steps):
        g = torch.Generator().manual_seed(seed * 100 + step)
        grads.append([torch.randn(p.shape, generator=g).to(DEV) for p in params])
    torch.cuda.synchronize()

    def run():
        for step in range(steps):
            for p, grad in zip(params, grads[step]):
                p.grad = grad
            opt.step()
    if stream is None:
        run()
    else:
        with torch.cuda.stream(stream):
            run()
    return params, opt


def all_bits(params, opt):
    return [bits(t) for p in params for t in (p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'])]


def test_two_fresh_optimisers_return_the_same_bits(Adam, limits):
    sizes = [1, 5, 65, limits[1] + 1, 300007]
    a, b = stepped(Adam, sizes, STEPS), stepped(Adam, sizes, STEPS)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(all_bits(*a), all_bits(*b)))
    assert not torch.equal(bits(a[0][4]), bits(make_params(sizes, seed=25)[4]))                    # and the steps did move the parameters


def test_same_bits_on_a_side_stream_beside_f16_mfma(Adam, limits):
    """two steps on a side stream, ten times beside testkit's F16-MFMA load on the main stream, return their solo bits (the two-stream hazard family, as
    tests/test_patch_encoder_backward_gpu.py).  Everything is built before the loop -- parameters, the optimiser with its state, the gradients, clones of
    p, m, v to start from -- so that inside a repetition there is nothing but wait_stream, the load, and on the side stream the restore (device copies) and
    the steps: no allocation, no copy from the host, no synchronisation between the load's launch and the last step's"""
    sizes = [5, 65, limits[1] + 1, 300007, 1000003]
    params, opt = stepped(Adam, sizes, 1)                            # one step: the state exists
    g = torch.Generator().manual_seed(26)
    grads = [[torch.randn(p.shape, generator=g).to(DEV) for p in params] for _ in range(2)]
    state = [(p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']) for p in params]
    start = [tuple(t.detach().clone() for t in row) for row in state]
    main, side = torch.cuda.current_stream(), torch.cuda.Stream(DEV)
    scratch = torch.empty(256 * 256, dtype=torch.float32, device=DEV)

    def two_steps():
        """from `start`, on the current stream; touches the host only for the step counts"""
        with torch.no_grad():
            for row, row0 in zip(state, start):
                for t, t0 in zip(row, row0):
                    t.copy_(t0)
        for p in params:
            opt.state[p]['step'].fill_(1.0)
        for step in range(2):
            for p, grad in zip(params, grads[step]):
                p.grad = grad
            opt.step()

    two_steps()
    torch.cuda.synchronize()
    solo = all_bits(params, opt)
    assert not torch.equal(solo[12], bits(start[4][0])), 'the steps move the parameters'
    bad, beside = [], []
    for rep in range(10):
        side.wait_stream(main)
        testkit.f16_mfma_load(main, scratch, iters=20000)            # about 5 ms on every CU
        loaded = torch.cuda.Event()
        loaded.record(main)
        with torch.cuda.stream(side):
            two_steps()
        beside.append(not loaded.query())                            # the load had not ended when the last step was launched
        main.wait_stream(side)
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip(all_bits(params, opt), solo)):
            if not torch.equal(x, y):
                bad.append((rep, sizes[i // 3], 'pmv'[i % 3]))
    assert not bad, bad
    print('\nside stream: steps launched while the load was still running in %d of 10 repetitions' % sum(beside))
    assert any(beside), 'the F16-MFMA load ended before the steps were launched in every repetition: nothing ran beside it'


# ------------------------------------------------------------------------------------------------ torch's state layout
@pytest.mark.parametrize('first', ['rfuse', 'torch'])
def test_state_dict_interchange_with_torch_adam(Adam, first):
    """3 steps with one class, state_dict -> load_state_dict of the other on the same GPU parameters, 2 more steps: every step within the bar"""
    params = make_params([4099, 3001], seed=27)
    make = {'rfuse': lambda: Adam(params, lr=1e-3, weight_decay=5e-5), 'torch': lambda: torch.optim.Adam(params, lr=1e-3, weight_decay=5e-5)}
    second = 'torch' if first == 'rfuse' else 'rfuse'
    opt = make[first]()
    for step in range(3):
        set_grads(params, 2800 + step)
        checked_step(opt, '%s first, step %d' % (first, step))
    sd = opt.state_dict()
    assert all(v['step'].device.type == 'cpu' and v['exp_avg'].is_cuda for v in sd['state'].values())
    other = make[second]()
    other.load_state_dict(sd)
    assert [int(other.state[p]['step']) for p in params] == [3, 3]
    assert all(other.state[p]['step'].device.type == 'cpu' and other.state[p]['exp_avg'].device == p.device for p in params)
    for step in range(3, 5):
        set_grads(params, 2800 + step)
        checked_step(other, '%s after %s, step %d' % (second, first, step))
    assert [int(other.state[p]['step']) for p in params] == [5, 5]


def test_step_refuses_a_graph_capture_and_foreign_parameters(Adam, monkeypatch):
    params = make_params([3001], seed=29)
    opt = Adam(params, **KW)
    set_grads(params, 30)
    opt.step()                                                       # the state exists: a capture would find nothing to allocate
    torch.cuda.synchronize()
    before = bits(params[0])
    set_grads(params, 31)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)      # what a capture answers; no graph is built for the refusal
    with pytest.raises(RuntimeError, match='inside a graph capture'):
        opt.step()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.equal(bits(params[0]), before) and int(opt.state[params[0]]['step']) == 1
    # a launch that raises leaves the step counts where the tensors are
    from rfuse import _lib

    def refuse(*args):
        raise RuntimeError('rf_adam_step failed (rc=-3): no launch')
    monkeypatch.setattr(_lib.load_optim(), 'rf_adam_step', refuse)
    with pytest.raises(RuntimeError, match='no launch'):
        opt.step()
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.equal(bits(params[0]), before) and int(opt.state[params[0]]['step']) == 1
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(bits(params[0]), before) and int(opt.state[params[0]]['step']) == 2
    half = torch.nn.Parameter(torch.zeros(8, device=DEV, dtype=torch.float16))
    half.grad = torch.zeros_like(half)
    with pytest.raises(ValueError, match=r'parameter 0 of group 0 \(shape \(8,\), torch.float16, cuda:0\) is not a contiguous float32 tensor'):
        Adam([half]).step()
    strided = torch.nn.Parameter(torch.zeros(8, 6, device=DEV).t())
    strided.grad = torch.zeros(6, 8, device=DEV)
    with pytest.raises(ValueError, match='is not a contiguous float32 tensor on a GPU'):
        Adam([strided]).step()


# ------------------------------------------------------------------------------------------------ what the layers derive from their parameters
def test_encoder_and_conv_layer_follow_the_step(Adam):
    """tests/test_derived_state_gpu.py's contract under this optimiser: after ``step()`` a Patch08(16, 64) encoder and a SingleConv 'gcr' layer give, under
    no_grad, the bits of a twin whose parameters were written with copy_ from the optimiser's results; the conv layer's operand images are new ones"""
    import test_derived_state_gpu as ds
    from model import retrieval

    class Encoder:
        mode = 'split'

        def make(self):
            return retrieval.Patch08(16, 64)

        def run(self, mod, xd):
            return mod(*xd)
    layer = ds.LAYERS['conv3s']
    g = torch.Generator().manual_seed(31)
    for kind, spec, xd in (('Patch08(16, 64)', Encoder(), (ds.rnd(g, 8, 1, 8, 8, 8).to(DEV),)), ('SingleConv gcr', layer, layer.to_device(None, layer.inputs(g)))):
        mod = spec.make().to(DEV).eval() if kind.startswith('Patch08') else ds.build(layer, 32)
        with ds.arith(spec.mode), torch.no_grad():
            before = spec.run(mod, xd)
            images = (mod.conv.packed_split(), mod.conv.packed()) if kind.startswith('SingleConv') else None
        params = list(mod.parameters())
        versions = [p._version for p in params]
        opt = Adam(params, lr=0.05)
        set_grads(params, 33)
        opt.step()
        for p in params:
            p.grad = None
        assert all(p._version > v for p, v in zip(params, versions)), '%s: a version counter did not move' % kind
        twin = spec.make().to(DEV).eval()
        with torch.no_grad():
            for q, p in zip(twin.parameters(), params):
                q.copy_(p)
        with ds.arith(spec.mode), torch.no_grad():
            after, want = spec.run(mod, xd), spec.run(twin, xd)
            assert ds.same_bits(after, want), '%s: not the bits of a twin holding the stepped parameters (max diff %.3e)' % (kind, float((after - want).abs().max()))
            assert not ds.same_bits(after, before), '%s: the step changed nothing' % kind
            if images is not None:
                new = (mod.conv.packed_split(), mod.conv.packed())
                for old, now, name in zip(images, new, ('packed_split', 'packed')):
                    first = lambda im: im[0] if isinstance(im, (tuple, list)) else im
                    assert now is not old, 'Conv3dParams.%s() returned the image of the old weights' % name
                    assert first(now).shape == first(old).shape and not torch.equal(first(now), first(old)), name


def test_feature_cache_turns_stale(Adam, gpu):
    import numpy as np
    import helpers
    from rfuse import configs as rf_configs
    from rfuse import synthetic
    from rfuse.database import PatchDatabase
    from rfuse.engine import RefinementEngine
    cfg = rf_configs.get_config('C3')
    db = synthetic.make_database(33, cfg, 64 * 2 + 10)
    eng = RefinementEngine(cfg, gpu, PatchDatabase(db['emb'], db['meta'], db['volumes'], gpu))
    shapes = {name: {k: tuple(v.shape) for k, v in m.state_dict().items()} for name, m in eng.modules().items()}
    eng.load_state_dicts({name: helpers.seeded_sd(shapes[name], 400 + len(name)) for name in shapes})
    eng.database.build_feature_cache(eng.retrieval_backbone, cfg, rows_per_batch=128)
    assert eng.database.feature_cache_fresh(eng.retrieval_backbone)
    params = list(eng.retrieval_backbone.parameters())
    opt = Adam(params, lr=1e-4, weight_decay=5e-5)
    opt.step()                                                       # no gradients: nothing was updated, the cache is still good
    assert eng.database.feature_cache_fresh(eng.retrieval_backbone)
    set_grads(params, 34, scale=1e-3)
    opt.step()
    assert not eng.database.feature_cache_fresh(eng.retrieval_backbone)


def test_retrieval_step_runs_without_a_host_sync_in_step(Adam):
    """one RetrievalStepLoss step with the IoU matrix on a Patch04(32, 64) / Patch08(16, 64) pair at B = 8: forward, backward and ``step()`` behind 5 ms of
    foreign work on the stream, events recorded around ``step()``.  Asserted: nothing raised.  Printed: whether ``step()`` came back before the stream
    had reached it, which a host synchronisation inside would make impossible."""
    from model import retrieval
    from rfuse.losses import RetrievalStepLoss
    b = 8
    torch.manual_seed(35)
    fq, ft = retrieval.Patch04(32, 64).to(DEV), retrieval.Patch08(16, 64).to(DEV)
    params = list(fq.parameters()) + list(ft.parameters())
    opt = Adam(params, lr=1e-4, weight_decay=5e-5)
    g = torch.Generator().manual_seed(36)
    mean, std, voxel = 0.06, 0.01, 0.020834
    xq = (torch.rand(b, 1, 4, 4, 4, generator=g) * 2 - 1).to(DEV)
    target = ((torch.rand(b, 1, 8, 8, 8, generator=g) * 3 * voxel - mean) / std).to(DEV)
    loss_mod = RetrievalStepLoss(0.2, mean, std, voxel, iou_scaling=True)
    scratch = torch.empty(256 * 256, dtype=torch.float32, device=DEV)
    returned_early = []
    for step in range(2):                                             # the first step creates the state, the second allocates nothing
        opt.zero_grad(set_to_none=True)
        total, _ = loss_mod(fq(xq), ft(target), target, train=True)
        total.backward()
        torch.cuda.synchronize()
        testkit.f16_mfma_load(torch.cuda.current_stream(), scratch, iters=20000)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        opt.step()
        e1.record()
        returned_early.append(not e1.query())
        torch.cuda.synchronize()
        assert math.isfinite(float(total.detach()))
    assert all(int(opt.state[p]['step']) == 2 for p in params) and all(torch.isfinite(p).all() for p in params)
    print('\nretrieval step: step() returned before the stream reached it: %s; step() on the GPU %.3f ms' % (returned_early, e0.elapsed_time(e1)))
