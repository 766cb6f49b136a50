"""The yardsticks of the optimiser tests (rfuse/optim.py, csrc/optim.hip), plain torch only.

``adam_f64`` restates one step of ``torch/optim/adam.py:_single_tensor_adam`` (amsgrad=False, maximize=False, capturable=False) in float64:

    step += 1;  g = g + wd * p (wd != 0);  m = lerp(m, g, 1 - beta1);  v = beta2 * v + (1 - beta2) * g * g
    p = p + (-(lr / (1 - beta1^step))) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)

``torch_adam`` runs the class itself (``foreach=False``) on CPU copies from the same state, in float32 or float64; ``bar`` is the comparison every GPU
test makes: the kernel's max-abs distance from float64 against 4 x that of torch's CPU float32 run (the reasons are in tests/test_optim_gpu.py)."""
import math

import torch


def adam_f64(p, g, m, v, step, lr, betas, eps, weight_decay):
    """one step from (p, m, v) after ``step`` earlier ones along g: the new (p, m, v) in float64, scalars in Python floats (float64, never rounded to float32)"""
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    beta1, beta2 = betas
    t = step + 1
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (1 - beta1) * (g - m)
    v = beta2 * v + (1 - beta2) * g * g
    step_size = lr / (1 - beta1 ** t)
    denom = v.sqrt() / math.sqrt(1 - beta2 ** t) + eps
    return p + (-step_size) * m / denom, m, v


def torch_adam(p, g, m, v, step, lr, betas, eps, weight_decay, dtype=torch.float32):
    """the same step by torch.optim.Adam(foreach=False) on CPU copies in ``dtype``: the new (p, m, v)"""
    q = torch.nn.Parameter(p.detach().cpu().to(dtype).clone())
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    opt.state[q] = {'step': torch.tensor(float(step)), 'exp_avg': m.detach().cpu().to(dtype).clone(), 'exp_avg_sq': v.detach().cpu().to(dtype).clone()}
    q.grad = g.detach().cpu().to(dtype).clone()
    opt.step()
    assert float(opt.state[q]['step']) == step + 1
    return q.detach(), opt.state[q]['exp_avg'], opt.state[q]['exp_avg_sq']


def bar(got, cpu32, ref64, what):
    """``got`` (the kernel's float32 tensor, on the CPU) against ``ref64`` under the bar ``cpu32`` sets: NaN / +inf / -inf exactly where torch's CPU float32 run
    has them; over the elements that are finite in both references max |got - ref64| <= 4 max |cpu32 - ref64|, and where cpu32 lands on the rounded
    float64 result everywhere so must ``got``.  Returns (error, diff32) for the tests' prints."""
    got, cpu32 = got.detach().cpu().reshape(-1), cpu32.detach().reshape(-1)
    ref64 = ref64.reshape(-1)
    assert got.dtype == torch.float32 and cpu32.dtype == torch.float32 and ref64.dtype == torch.float64 and got.shape == cpu32.shape == ref64.shape, what
    for name, mask in (('NaN', torch.isnan), ('+inf', torch.isposinf), ('-inf', torch.isneginf)):
        assert torch.equal(mask(got), mask(cpu32)), '%s: %s at %d elements where torch CPU has none or the reverse' % (what, name, int((mask(got) != mask(cpu32)).sum()))
    fin = torch.isfinite(cpu32) & torch.isfinite(ref64)
    if not fin.any():
        return 0.0, 0.0
    diff32 = float((cpu32.double() - ref64)[fin].abs().max())
    err = float((got.double() - ref64)[fin].abs().max())
    if diff32 == 0.0:
        assert torch.equal(got[fin], ref64.float()[fin]), '%s: torch CPU float32 lands on the rounded float64 result, the kernel is off by %.3e' % (what, err)
    else:
        assert err <= 4 * diff32, '%s: max abs error %.3e > 4 x %.3e (torch CPU float32 against the same float64 result)' % (what, err, diff32)
    return err, diff32


def fma32(a, b, c):
    """fl32(a * b + c) of float32 tensors, one rounding, on any CPU: the product of two float32 is exact in float64, TwoSum gives the exact sum with c as
    s + e, and s is rounded to float32 with the tie that e breaks decided by e (float32 normal range)"""
    a, b, c = torch.broadcast_tensors(a.double(), b.double(), c.double())
    prod = a * b
    s = prod + c
    bb = s - prod
    e = (prod - (s - bb)) + (c - bb)
    out = s.float()
    raw = s.contiguous().view(torch.int64)
    tie = ((raw & 0x1FFFFFFF) == 0x10000000) & (e != 0)
    if tie.any():
        down = (raw & ~0x1FFFFFFF).view(torch.float64).float()                    # towards zero
        up = torch.nextafter(down, torch.where(s > 0, float('inf'), float('-inf')).float())
        out = torch.where(tie, torch.where((e > 0) == (s > 0), up, down), out)
    return out


def opwise_f32(p, g, m, v, step, lr, betas, eps, weight_decay):
    """csrc/optim.hip's sequence (include/rfuse_optim.h): one torch CPU float32 operation per kernel operation, its three fused multiply-adds through
    ``fma32`` -- what the kernel returns bit for bit if each of its operations is correctly rounded.  The scalars are rounded to float32 once, as
    rfuse/optim.py hands them over."""
    f = lambda x: torch.tensor(x, dtype=torch.float64).float()
    p, g, m, v = (t.detach().cpu().float().clone() for t in (p, g, m, v))
    beta1, beta2 = betas
    t = step + 1
    neg_step, bc2_sqrt, w1, w2 = f(-(lr / (1 - beta1 ** t))), f((1 - beta2 ** t) ** 0.5), f(1 - beta1), f(1 - beta2)
    if weight_decay != 0:
        g = fma32(f(weight_decay), p, g)
    d = g - m
    m = fma32(w1, d, m) if abs(float(w1)) < 0.5 else fma32(-d, 1 - w1, g)
    v = fma32(w2 * g, g, v * f(beta2))
    root = v.double().sqrt().float()          # the correctly rounded float32 root: torch's CPU float32 sqrt is off by one ulp on 0.7 % of its inputs
    denom = root / bc2_sqrt + f(eps)
    return p + (neg_step * m) / denom, m, v
