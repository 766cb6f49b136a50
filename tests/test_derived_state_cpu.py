"""The cached max |t| behind ops.split_range_ok follows the tensor it was computed from (CPU tensors; the HIP library is not loaded).

The range decides whether a layer may run the split-operand F16 forms or must take the fp32 kernels.  A cached value that outlives its tensor gives a
later tensor at the same address, with the same shape and version count, the dead tensor's answer: what the caching allocator produces when one model is
dropped and another of the same architecture is built and loaded.  The stand-in here is deterministic: a new Parameter on the SAME storage with a fresh
version counter, brought to the same version."""
import gc

import pytest
import torch

from rfuse import ops

IN_RANGE, OUT_WEIGHT = 0.0625, 3.0e4        # (exact in fp32) 3e4 > SPLIT_MAX_ABS_WEIGHT = 65504 / 16 / 8
OUT_GAMMA, OUT_BETA = 4.0e4, 2.0e6          # 4e4 * sqrt(1024) > SPLIT_MAX_ABS_ACT = 65504 * 16; 2e6 > it by itself
GROUP_ELEMENTS = 1024


def param_on(buf, value):
    """a new Parameter on buf's storage with a fresh version counter, filled in place: version 1 every time"""
    p = torch.nn.Parameter(buf.data)
    with torch.no_grad():
        p.fill_(value)
    assert p.data_ptr() == buf.data_ptr() and p._version == 1
    return p


def layer_ok(w, g, b):
    return ops.split_range_ok(w, g, b, GROUP_ELEMENTS)


@pytest.mark.parametrize('what,out', [('weight', OUT_WEIGHT), ('gamma', OUT_GAMMA), ('beta', OUT_BETA)])
@pytest.mark.parametrize('first_in_range', [True, False], ids=['in_then_out', 'out_then_in'])
def test_a_tensor_on_reused_storage_gets_its_own_range(what, out, first_in_range):
    bufs = {'weight': torch.empty(16, 16, 3, 3, 3), 'gamma': torch.empty(16), 'beta': torch.empty(16)}
    others = {k: param_on(torch.empty_like(v), IN_RANGE) for k, v in bufs.items() if k != what}
    values = (IN_RANGE, out) if first_in_range else (out, IN_RANGE)
    for value in values:                                      # the first tensor is dropped (rebinding `p`) before the second is made on its storage
        p = param_on(bufs[what], value)
        args = dict(others, **{what: p})
        assert layer_ok(args['weight'], args['gamma'], args['beta']) == (value == IN_RANGE), (what, value)
        assert ops._abs_max(p) == value
        if what == 'weight':
            assert ops.split_range_ok(p) == (value == IN_RANGE)
        del args, p


def test_no_entry_outlives_its_tensor():
    """after a tensor whose range was asked for is dropped and collected, nothing that describes it is left to answer for a later tensor"""
    buf = torch.empty(8, 8, 3, 3, 3)
    a = param_on(buf, IN_RANGE)
    assert ops.split_range_ok(a)
    ident = id(a)
    assert ops._range_seen.get(ident) is a
    del a
    gc.collect()
    assert ident not in ops._range_seen
    assert not any(u.data_ptr() == buf.data_ptr() for u in ops._range_seen.values())
    for name, table in vars(ops).items():                     # and no module-level table keyed by the address survives
        if isinstance(table, dict) and not name.startswith('__'):
            assert not any(isinstance(k, tuple) and buf.data_ptr() in k for k in table), name
    b = param_on(buf, OUT_WEIGHT)
    assert ops._abs_max(b) == OUT_WEIGHT and not ops.split_range_ok(b)


def test_an_in_place_edit_refreshes_the_range():
    w = torch.nn.Parameter(torch.full((4, 4, 3, 3, 3), IN_RANGE))
    assert ops.split_range_ok(w)
    with torch.no_grad():
        w[1, 2, 0, 1, 2] = -OUT_WEIGHT
    assert ops._abs_max(w) == OUT_WEIGHT and not ops.split_range_ok(w)
    with torch.no_grad():
        w.clamp_(-1.0, 1.0)
    assert ops._abs_max(w) == 1.0 and ops.split_range_ok(w)


def test_a_replaced_parameter_object_gets_its_own_range():
    m = torch.nn.Linear(8, 8, bias=False)
    with torch.no_grad():
        m.weight.fill_(IN_RANGE)
    assert ops.split_range_ok(m.weight)
    m.weight = torch.nn.Parameter(torch.full((8, 8), OUT_WEIGHT))
    assert not ops.split_range_ok(m.weight)


def test_the_cached_range_is_not_reduced_again(monkeypatch):
    """one reduction (on the GPU: one host sync) per parameter version, none while nothing changes: the point of the cache is one sync per training step"""
    calls = []
    real_abs = torch.Tensor.abs

    def counting_abs(self, *a, **kw):
        calls.append(tuple(self.shape))
        return real_abs(self, *a, **kw)
    monkeypatch.setattr(torch.Tensor, 'abs', counting_abs)
    w, g, b = (torch.nn.Parameter(torch.full(s, IN_RANGE)) for s in ((4, 4, 3, 3, 3), (4,), (4,)))
    assert layer_ok(w, g, b)
    assert sorted(calls) == sorted([(4, 4, 3, 3, 3), (4,), (4,)])
    for _ in range(3):
        assert layer_ok(w, g, b)
    assert len(calls) == 3, 'an unchanged parameter was reduced again'
    with torch.no_grad():
        g.mul_(2.0)
    assert layer_ok(w, g, b) and layer_ok(w, g, b)
    assert calls[3:] == [(4,)], 'one edit of one parameter costs one reduction of that parameter'
