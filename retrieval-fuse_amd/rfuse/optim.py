"""``rfuse.optim.Adam``: ``torch.optim.Adam`` with the parameter update as one HIP pass (csrc/optim.hip, include/rfuse_optim.h) -- the drop-in at
``trainer/train_retrieval.py:37`` and ``trainer/train_refinement.py:186-200`` of the reference.

The arithmetic is ``torch/optim/adam.py:_single_tensor_adam`` with ``amsgrad=False, maximize=False, capturable=False``; the bias corrections and the step
size are computed here in Python floats exactly where torch computes them and handed to the kernel per tensor (``t``, ``lr`` and ``weight_decay`` may differ
per tensor and per group).  The state is torch's -- ``{'step': CPU float32 scalar, 'exp_avg', 'exp_avg_sq'}`` -- so state dicts go both ways between
the two classes and a Lightning checkpoint's ``optimizer_states`` load.  ``step()`` makes ``ceil(T / rf_adam_step_max_tensors())`` launches per device on the
current stream, allocates nothing after the first step (apart from the contiguous copy of a non-contiguous gradient), does not synchronise the host, and
bumps every updated parameter's version counter, so that whatever a layer derives from its parameters (packed weight images, range decisions, the
database's feature cache) follows it as it follows torch's in-place update.  There is no fallback: a parameter the kernel cannot update is an error.
"""
import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ['Adam']

# one record of the host table of rf_adam_step (include/rfuse_optim.h)
_RECORD = np.dtype([('param', '<u8'), ('grad', '<u8'), ('exp_avg', '<u8'), ('exp_avg_sq', '<u8'), ('n', '<i8'), ('scalars', '<f4', (7,)), ('unused', '<u4')])


def _scalars(t, lr, beta1, beta2, eps, weight_decay):
    """-step_size, sqrt(1 - beta2^t), 1 - beta1, beta2, 1 - beta2, eps, weight_decay: adam.py's expressions, in Python floats"""
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    return (-step_size, bias_correction2_sqrt, 1 - beta1, beta2, 1 - beta2, eps, weight_decay)


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        if amsgrad:
            raise ValueError('rfuse.optim.Adam: amsgrad=True is not implemented (torch.optim.Adam has it)')
        if maximize:
            raise ValueError('rfuse.optim.Adam: maximize=True is not implemented (torch.optim.Adam has it)')
        if isinstance(lr, torch.Tensor):
            raise ValueError('rfuse.optim.Adam: lr is a Python float (the step size is computed on the host)')
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError('Invalid beta parameter at index 0: %r' % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid beta parameter at index 1: %r' % (betas[1],))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        # torch.optim.Adam's group keys, at the only values this class implements: a state dict of either class loads into the other
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                                      differentiable=False, fused=None, decoupled_weight_decay=False))

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for key, value in (('amsgrad', False), ('maximize', False), ('foreach', None), ('capturable', False), ('differentiable', False), ('fused', None),
                               ('decoupled_weight_decay', False)):
                group.setdefault(key, value)

    @staticmethod
    def _describe(group, gi, pi, p):
        names = group.get('param_names')
        return 'parameter %s of group %d (shape %s, %s, %s)' % (repr(names[pi]) if names else pi, gi, tuple(p.shape), p.dtype, p.device)

    def _collect(self):
        """(device, parameter, gradient, state, group) of every parameter that has a gradient, refusing what the kernel does not update"""
        todo = []
        for gi, group in enumerate(self.param_groups):
            for key in ('amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay'):
                if group.get(key):
                    raise ValueError('rfuse.optim.Adam: group %d has %s=%r, which is not implemented (torch.optim.Adam has it)' % (gi, key, group[key]))
            for pi, p in enumerate(group['params']):
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError('Adam does not support sparse gradients, please consider SparseAdam instead')
                if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                    raise ValueError('rfuse.optim.Adam: %s is not a contiguous float32 tensor on a GPU (no CPU fallback)' % self._describe(group, gi, pi, p))
                if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or g.layout != torch.strided:
                    raise ValueError('rfuse.optim.Adam: the gradient of %s is %s %s on %s' % (self._describe(group, gi, pi, p), tuple(g.shape), g.dtype, g.device))
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = torch.tensor(0.0, dtype=torch.float32)                 # on the host, like torch's (capturable and fused off)
                    state['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = state['step']
                if not torch.is_tensor(step) or step.device.type != 'cpu':
                    raise ValueError('rfuse.optim.Adam: the step count of %s is not a CPU tensor (a capturable or fused state?)' % self._describe(group, gi, pi, p))
                for key in ('exp_avg', 'exp_avg_sq'):
                    s = state[key]
                    if s.dtype != torch.float32 or s.device != p.device or s.shape != p.shape or not s.is_contiguous():
                        raise ValueError('rfuse.optim.Adam: %s of %s is not a contiguous float32 tensor beside it' % (key, self._describe(group, gi, pi, p)))
                todo.append((p.device, p, g if g.is_contiguous() else g.contiguous(), state, group))
        return todo

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('rfuse.optim.Adam.step inside a graph capture: the step count lives on the host (capturable=False); step outside the capture')
        todo = self._collect()
        if not todo:
            return loss
        counts = torch.stack([state['step'] for _, _, _, state, _ in todo]).tolist()      # host tensors: no device is asked
        lib = _lib.load_optim()
        memo = {}
        by_device = {}
        for (dev, p, g, state, group), count in zip(todo, counts):
            rows, steps = by_device.setdefault(dev, ([], []))
            steps.append(state['step'])
            if p.numel() == 0:                                                               # nothing to update: the step count alone advances, as torch's
                continue
            beta1, beta2 = group['betas']
            key = (count + 1, float(group['lr']), float(beta1), float(beta2), float(group['eps']), float(group['weight_decay']))
            sc = memo.get(key)
            if sc is None:
                sc = memo[key] = _scalars(*key)
            rows.append((p.data_ptr(), g.data_ptr(), state['exp_avg'].data_ptr(), state['exp_avg_sq'].data_ptr(), p.numel(), sc, 0))
        for dev, (rows, steps) in by_device.items():
            if rows:
                table = np.array(rows, dtype=_RECORD)
                with torch.cuda.device(dev):
                    lib.rf_adam_step(ctypes.c_void_p(table.ctypes.data), len(rows), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch._foreach_add_(steps, 1)                                                    # after the launch: a launch that raises leaves the counts with the tensors
        torch.autograd.graph.increment_version([p for _, p, _, _, _ in todo])
        return loss
