"""CPU: the host side of the HIP Adam step (rfuse/optim.py, include/rfuse_optim.h, csrc/optim.hip) -- the ninth header's binding and its status rule, what
csrc/build.py names, the float64 restatement of tests/optim_ref.py pinned to torch.optim.Adam's own float64 run, the constructor's refusals, the state
dict's way through torch.optim.Adam and back, and the refusals of ``step()`` and of ``rf_adam_step`` that come before any launch."""
import copy
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import optim_ref as oref

REPO = Path(__file__).resolve().parents[1]
NAMES = {'rf_adam_step', 'rf_adam_step_max_tensors', 'rf_adam_step_record_bytes', 'rf_adam_step_segment'}
OTHERS = ('rfuse.h', 'rfuse_eval.h', 'rfuse_train.h', 'rfuse_contrastive.h', 'rfuse_pairs.h', 'rfuse_attn_train.h', 'rfuse_level.h', 'rfuse_data.h')
OTHER_TABLES = ('SIGNATURES', 'EVAL_SIGNATURES', 'TRAIN_SIGNATURES', 'CONTRASTIVE_SIGNATURES', 'PAIRS_SIGNATURES', 'ATTN_TRAIN_SIGNATURES', 'LEVEL_SIGNATURES',
                'DATA_SIGNATURES')


def declared(header):
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / header).read_text(), flags=re.S)
    return set(re.findall(r'\b(rf_[a-z0-9_]+)\s*\(', text))


# ------------------------------------------------------------------------------------------------ the header and the build
def test_optim_header_is_bound_and_exported():
    from rfuse import _lib
    assert declared('rfuse_optim.h') == NAMES == set(_lib.OPTIM_SIGNATURES)
    assert _lib.OPTIM_HEADER_PATH == REPO / 'include' / 'rfuse_optim.h'
    lib = _lib.load_optim()
    for n in NAMES:
        assert hasattr(lib, n), '%s declared in include/rfuse_optim.h but not exported by librfuse_hip.so' % n
    assert lib is _lib.load_optim() and lib._cdll is _lib.load()._cdll
    assert ctypes.c_double not in {a for _, args, _ in _lib.OPTIM_SIGNATURES.values() for a in args}
    assert 'extern "C"' in (REPO / 'include' / 'rfuse_optim.h').read_text()
    # the status rule: rf_adam_step launches and reports, the three queries return values
    assert _lib.is_status('rf_adam_step', _lib.OPTIM_SIGNATURES)
    res, args, params = _lib.OPTIM_SIGNATURES['rf_adam_step']
    assert res is ctypes.c_int and params == ['records', 'count', 'stream'] and args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    assert {n for n, fn in lib._direct.items() if fn.errcheck is not None} == {'rf_adam_step'}
    assert not any(_lib.is_status(n, _lib.OPTIM_SIGNATURES) for n in NAMES - {'rf_adam_step'})
    # disjoint from the other eight tables and headers
    assert len(OTHER_TABLES) == len(OTHERS) == 8
    for table in OTHER_TABLES:
        assert not set(getattr(_lib, table)) & NAMES, table
    for header in OTHERS:
        assert 'rfuse_optim' not in (REPO / 'include' / header).read_text()
        assert not declared(header) & NAMES


def test_build_names_the_source_its_flag_and_the_header():
    build_py = (REPO / 'retrieval-fuse_amd' / 'csrc' / 'build.py').read_text()
    assert "'optim.hip', " in build_py and "'optim.hip': ['-ffp-contract=off']" in build_py and "'rfuse_optim.h'" in build_py
    assert "'dataset.hip']" in build_py                                           # the source list still ends where tests/test_dataset_cpu.py pins it
    import importlib.util
    spec = importlib.util.spec_from_file_location('rfuse_csrc_build', REPO / 'retrieval-fuse_amd' / 'csrc' / 'build.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert 'optim.hip' in mod.SOURCES and mod.SOURCES[-1] == 'dataset.hip' and '-ffp-contract=off' in mod.EXTRA_FLAGS['optim.hip']
    assert (REPO / 'retrieval-fuse_amd' / 'csrc' / 'optim.hip').exists()


def test_launch_capacity_and_record_layout():
    from rfuse import _lib, optim
    lib = _lib.load_optim()
    assert lib.rf_adam_step_max_tensors() >= 32
    assert lib.rf_adam_step_record_bytes() == optim._RECORD.itemsize == 72
    seg = lib.rf_adam_step_segment()
    assert seg >= 256 and seg % 4 == 0
    # the table in the kernel arguments: 4 pointers, 7 scalars and a count per tensor plus the prefix table, inside HIP's 4 KB
    assert lib.rf_adam_step_max_tensors() * 64 + (lib.rf_adam_step_max_tensors() + 1) * 4 <= 4096
    offsets = {name: optim._RECORD.fields[name][1] for name in optim._RECORD.names}
    assert offsets == {'param': 0, 'grad': 8, 'exp_avg': 16, 'exp_avg_sq': 24, 'n': 32, 'scalars': 40, 'unused': 68}


def test_adam_step_refuses_before_any_device_is_touched():
    from rfuse import _lib, optim
    lib = _lib.load_optim()
    sc = optim._scalars(1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    good = (256, 512, 768, 1024, 5, sc, 0)                       # pointers the argument checks never follow
    table = np.array([good], dtype=optim._RECORD)
    with pytest.raises(RuntimeError, match=r'^rf_adam_step failed \(rc=-1\): .*bad arguments'):
        lib.rf_adam_step(None, 1, None)
    with pytest.raises(RuntimeError, match=r'^rf_adam_step failed \(rc=-1\): .*bad arguments'):
        lib.rf_adam_step(ctypes.c_void_p(table.ctypes.data), 0, None)
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 258), (1, 513), (4, 0), (4, -3)):
        row = list(good)
        row[pos] = bad
        table = np.array([good, tuple(row)], dtype=optim._RECORD)
        with pytest.raises(RuntimeError, match=r'^rf_adam_step failed \(rc=-1\): .*record 1'):
            lib.rf_adam_step(ctypes.c_void_p(table.ctypes.data), 2, None)
    row = list(good)
    row[4] = 1 << 31
    table = np.array([tuple(row)], dtype=optim._RECORD)
    with pytest.raises(RuntimeError, match=r'^rf_adam_step failed \(rc=-2\): .*1 <= n < 2\^31'):
        lib.rf_adam_step(ctypes.c_void_p(table.ctypes.data), 1, None)


def test_scalars_are_torchs_expressions():
    from rfuse import optim
    for t, lr, b1, b2, eps, wd in ((1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0), (7.0, 1e-4 / 1500, 0.9, 0.999, 1e-8, 5e-5), (1501.0, 3e-4, 0.5, 0.9, 1e-6, 0.1)):
        neg_step, bc2, w1, beta2, w2, e, w = optim._scalars(t, lr, b1, b2, eps, wd)
        assert neg_step == -(lr / (1 - b1 ** t)) and bc2 == (1 - b2 ** t) ** 0.5 and w1 == 1 - b1 and beta2 == b2 and w2 == 1 - b2 and e == eps and w == wd


# ------------------------------------------------------------------------------------------------ the yardstick itself
def schedule(dtype, seed=0):
    """two groups (different lr / betas / eps, weight decay 0 and 5e-5), 7 steps, an lr change before steps 3 and 5, a parameter whose grad is None on
    steps 2 and 5: (groups of parameters, their keywords, per-step gradients, per-step lr scale)"""
    g = torch.Generator().manual_seed(seed)
    shapes = [[(5,), (3, 4), (1,)], [(7, 3), (2,)]]
    kws = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=5e-5)]
    params = [[torch.randn(*s, generator=g, dtype=torch.float64).to(dtype) for s in grp] for grp in shapes]
    grads = []
    for step in range(7):
        grads.append([[None if (step in (2, 5) and gi == 0 and pi == 1) else torch.randn(*s, generator=g, dtype=torch.float64).to(dtype) * 10.0 ** (step - 4)
                       for pi, s in enumerate(grp)] for gi, grp in enumerate(shapes)])
    scales = [1.0, 1.0, 1.0, 0.5, 0.5, 2.0, 2.0]
    return params, kws, grads, scales


def test_float64_restatement_is_torchs_adam():
    """tests/optim_ref.py:adam_f64 against torch.optim.Adam on float64 CPU parameters, 1e-13 relative over 7 steps: the yardstick has torch's semantics"""
    params, kws, grads, scales = schedule(torch.float64)
    live = [[torch.nn.Parameter(p.clone()) for p in grp] for grp in params]
    opt = torch.optim.Adam([dict(params=grp, **kw) for grp, kw in zip(live, kws)], foreach=False)
    mine = [[(p.clone(), torch.zeros_like(p), torch.zeros_like(p), 0) for p in grp] for grp in params]
    for step in range(7):
        for gi, grp in enumerate(live):
            opt.param_groups[gi]['lr'] = kws[gi]['lr'] * scales[step]
            for pi, p in enumerate(grp):
                p.grad = None if grads[step][gi][pi] is None else grads[step][gi][pi].clone()
        opt.step()
        for gi, grp in enumerate(live):
            kw = dict(kws[gi], lr=kws[gi]['lr'] * scales[step])
            for pi, p in enumerate(grp):
                q, m, v, t = mine[gi][pi]
                if grads[step][gi][pi] is not None:
                    q, m, v = oref.adam_f64(q, grads[step][gi][pi], m, v, t, kw['lr'], kw['betas'], kw['eps'], kw['weight_decay'])
                    t += 1
                    mine[gi][pi] = (q, m, v, t)
                    st = opt.state[p]
                    assert float(st['step']) == t
                    for got, want, name in ((q, p.detach(), 'p'), (m, st['exp_avg'], 'm'), (v, st['exp_avg_sq'], 'v')):
                        rel = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
                        assert rel <= 1e-13, (step, gi, pi, name, rel)
                else:
                    assert torch.equal(q, p.detach())
    assert mine[0][1][3] == 5 and mine[0][0][3] == 7 and float(opt.state[live[0][1]]['step']) == 5


def test_torch_cpu_kernels_fuse_what_the_header_fuses():
    """the three fused multiply-adds of include/rfuse_optim.h are torch's: on the CPU ``add(alpha)``, ``lerp_`` (both branches) and ``mul_().addcmul_()`` give
    the bits of ``optim_ref.fma32`` (exact product, exact sum, one rounding), vector body and scalar tail alike, and not those of the unfused forms.

    This is a statement about the torch build and the host it runs on (x86 with FMA, where ATen's vectorised and scalar loops contract these
    expressions), not about the project: on a host without FMA, or under a torch whose CPU kernels round differently, it fails, and what it then
    says is that torch's CPU float32 Adam -- the yardstick of the GPU tests' bar -- no longer rounds where include/rfuse_optim.h does"""
    f = lambda x: torch.tensor(x, dtype=torch.float64).float()
    g = torch.Generator().manual_seed(21)
    unfused = 0
    for n in (1, 3, 5, 7, 200003):
        p, grad, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
        v = torch.rand(n, generator=g) * 1e-3
        assert torch.equal(grad.add(p, alpha=5e-5), oref.fma32(f(5e-5), p, grad))
        unfused += int((grad.add(p, alpha=5e-5) != grad + f(5e-5) * p).sum())
        d = grad - m
        assert torch.equal(m.clone().lerp_(grad, 1 - 0.9), oref.fma32(f(1 - 0.9), d, m))
        assert torch.equal(m.clone().lerp_(grad, 1 - 0.4), oref.fma32(-d, 1 - f(1 - 0.4), grad))
        unfused += int((m.clone().lerp_(grad, 1 - 0.9) != m + f(1 - 0.9) * d).sum())
        got = v.clone().mul_(0.999).addcmul_(grad, grad, value=1 - 0.999)
        assert torch.equal(got, oref.fma32(f(1 - 0.999) * grad, grad, v * f(0.999)))
        unfused += int((got != v * f(0.999) + (f(1 - 0.999) * grad) * grad).sum())
    assert unfused > 1000                                             # the unfused forms are other functions: the comparison above can tell them apart
    # fma32 itself: a tie of the float64 sum that the exact remainder breaks, in both directions
    a = torch.tensor([1.0 + 2.0 ** -12] * 3)                                                   # a * a = 1 + 2^-11 + 2^-24: half an ulp above 1 + 2^-11
    c = torch.tensor([2.0 ** -60, -2.0 ** -60, 0.0])                                            # lost in the float64 sum, kept in its remainder
    assert oref.fma32(a, a, c).tolist() == [1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11]


def test_opwise_float32_restatement_is_inside_the_bar():
    """the kernel's operation sequence, one torch CPU float32 operation each (optim_ref.opwise_f32), against the bar the GPU tests apply -- on the CPU, so a
    bar that the specified arithmetic itself could not meet shows here first"""
    worst = 0.0
    for scale in (1e-9, 1e-4, 1.0, 3e7):
        for wd in (0.0, 5e-5):
            g = torch.Generator().manual_seed(11)
            p, m, v = torch.randn(5000, generator=g), torch.zeros(5000), torch.zeros(5000)
            for step in range(7):
                grad = torch.randn(5000, generator=g) * scale
                args = (p, grad, m, v, step, 1e-3, (0.9, 0.999), 1e-8, wd)
                ref, cpu32, got = oref.adam_f64(*args), oref.torch_adam(*args), oref.opwise_f32(*args)
                for a, b, c, name in zip(got, cpu32, ref, 'pmv'):
                    err, diff32 = oref.bar(a, b, c, 'scale %g wd %g step %d %s' % (scale, wd, step, name))
                    worst = max(worst, err / diff32 if diff32 else 0.0)
                p, m, v = got
    print('\nop-by-op float32 restatement: worst error ratio against torch CPU float32 %.3f (bar 4)' % worst)


# ------------------------------------------------------------------------------------------------ the class, as far as a CPU goes
def test_constructor_refusals_and_defaults():
    from rfuse.optim import Adam
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match='amsgrad'):
        Adam(p, amsgrad=True)
    with pytest.raises(ValueError, match='maximize'):
        Adam(p, maximize=True)
    for kw, text in ((dict(lr=-1.0), 'learning rate'), (dict(eps=-1e-8), 'epsilon'), (dict(betas=(1.0, 0.9)), 'beta parameter at index 0'),
                     (dict(betas=(0.9, -0.1)), 'beta parameter at index 1'), (dict(weight_decay=-1.0), 'weight_decay')):
        with pytest.raises(ValueError, match=text):
            Adam(p, **kw)
    opt = Adam(p)
    assert isinstance(opt, torch.optim.Optimizer)
    g = opt.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay'], g['amsgrad'], g['maximize']) == (1e-3, (0.9, 0.999), 1e-8, 0, False, False)
    assert set(g) - {'params'} == set(torch.optim.Adam(p).param_groups[0]) - {'params'}         # torch's own group keys: state dicts go both ways
    two = Adam([dict(params=p, lr=1e-2), dict(params=[torch.nn.Parameter(torch.zeros(2))], weight_decay=5e-5)], lr=1e-4)
    assert [q['lr'] for q in two.param_groups] == [1e-2, 1e-4] and [q['weight_decay'] for q in two.param_groups] == [0, 5e-5]
    sched = torch.optim.lr_scheduler.MultiStepLR(two, milestones=[1], gamma=0.5)                  # a scheduler takes it as it takes torch's
    assert sched.get_last_lr() == [1e-2, 1e-4]


def test_step_refuses_what_the_kernel_does_not_update():
    from rfuse.optim import Adam
    p = torch.nn.Parameter(torch.zeros(3))
    opt = Adam([p])
    assert opt.step() is None and len(opt.state) == 0                                              # no gradient anywhere: nothing to do, nothing raised
    assert opt.step(lambda: torch.tensor(3.0)) == 3.0
    p.grad = torch.ones(3)
    with pytest.raises(ValueError, match=r'parameter 0 of group 0 \(shape \(3,\), torch.float32, cpu\) is not a contiguous float32 tensor on a GPU'):
        opt.step()
    assert len(opt.state) == 0
    q = torch.nn.Parameter(torch.zeros(4, 3))
    q.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 3))
    with pytest.raises(RuntimeError, match='Adam does not support sparse gradients'):
        Adam([q]).step()
    named = Adam([('enc.weight', p)])
    with pytest.raises(ValueError, match=r"parameter 'enc.weight' of group 0"):
        named.step()
    opt.param_groups[0]['amsgrad'] = True
    with pytest.raises(ValueError, match='group 0 has amsgrad=True'):
        opt.step()


def test_state_dict_round_trip_through_torch_adam():
    g = torch.Generator().manual_seed(3)
    from rfuse.optim import Adam
    ps = [torch.nn.Parameter(torch.randn(4, 3, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g)), torch.nn.Parameter(torch.randn(2, generator=g))]
    groups = lambda: [dict(params=ps[:2], lr=1e-2, weight_decay=5e-5), dict(params=ps[2:], betas=(0.8, 0.99))]
    ref = torch.optim.Adam(groups(), lr=1e-4)
    for p in ps[:2]:
        p.grad = torch.randn(p.shape, generator=g)
    ref.step()
    ref.step()                                                                                      # ps[2] has no gradient: no state, as in a real checkpoint
    sd = ref.state_dict()
    saved = copy.deepcopy(sd)                                                                       # as torch.load returns it: load_state_dict shares the CPU step tensors
    mine = Adam(groups(), lr=1e-4)
    mine.load_state_dict(sd)
    back = mine.state_dict()
    assert back['param_groups'] == sd['param_groups']
    assert set(back['state']) == set(sd['state']) == {0, 1}
    for k in sd['state']:
        assert list(back['state'][k]) == ['step', 'exp_avg', 'exp_avg_sq']
        for name in back['state'][k]:
            a, b = back['state'][k][name], sd['state'][k][name]
            assert a.dtype == b.dtype == torch.float32 and a.device == b.device == torch.device('cpu') and torch.equal(a, b), (k, name)
        assert back['state'][k]['step'].shape == () and float(back['state'][k]['step']) == 2.0
    again = torch.optim.Adam(groups(), lr=1e-4)
    again.load_state_dict(back)
    again.step()
    assert float(again.state[ps[0]]['step']) == 3.0 and ps[2] not in again.state
    # a Lightning checkpoint keeps state_dict() of each optimiser in a list under 'optimizer_states'
    checkpoint = {'optimizer_states': [torch.optim.Adam(groups(), lr=1e-4).state_dict(), saved]}
    mine.load_state_dict(checkpoint['optimizer_states'][1])
    assert float(mine.state[ps[1]]['step']) == 2.0
