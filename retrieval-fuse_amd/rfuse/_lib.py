"""ctypes binding of librfuse_hip.so (the C ABI declared in include/rfuse.h, the evaluation ABI of include/rfuse_eval.h, the training-loss ABI
of include/rfuse_train.h, the contrastive-loss ABI of include/rfuse_contrastive.h, the pairwise-occupancy ABI of include/rfuse_pairs.h, the
attention-backward ABI of include/rfuse_attn_train.h, the level ABI of include/rfuse_level.h, the dataset ABI of include/rfuse_data.h, the
optimiser ABI of include/rfuse_optim.h and the refinement-step ABI of include/rfuse_step.h).

The argument and return types are read from the header itself at import (``parse_header``): there is no second copy of the ABI to keep
in step.  There is NO fallback: if the library is missing a RuntimeError is raised, and every entry point that returns a status
(``is_status``) raises a RuntimeError with ``rf_last_error()`` when that status is not 0.  ``import torch`` must come
first so that the HIP runtime the library binds to is the one PyTorch-ROCm already loaded (same SONAME).

``load()`` binds include/rfuse.h (``SIGNATURES``; the profiling wrapper brackets these); ``load_eval()`` binds include/rfuse_eval.h
(``EVAL_SIGNATURES``: the mesh metrics, rfuse/mesh_metrics.py) and ``load_train()`` include/rfuse_train.h (``TRAIN_SIGNATURES``: the shape loss,
rfuse/losses.py) and ``load_contrastive()`` include/rfuse_contrastive.h (``CONTRASTIVE_SIGNATURES``: NT-Xent and the sliced attention contrastive
loss, rfuse/losses.py) and ``load_pairs()`` include/rfuse_pairs.h (``PAIRS_SIGNATURES``: the retrieval trainer's IoU matrix, rfuse/losses.py) and ``load_attn_train()`` include/rfuse_attn_train.h
(``ATTN_TRAIN_SIGNATURES``: the backward of the patch attention's row route, rfuse/ops.py) and ``load_level()`` include/rfuse_level.h (``LEVEL_SIGNATURES``:
a whole encoder level in one launch, rfuse/ops.py) and ``load_data()`` include/rfuse_data.h (``DATA_SIGNATURES``: the patch dataset's occupancy counts and batch
windows, rfuse/data.py) and ``load_optim()`` the ninth header include/rfuse_optim.h (``OPTIM_SIGNATURES``: the multi-tensor Adam step, rfuse/optim.py) and ``load_step()`` the tenth,
include/rfuse_step.h (``STEP_SIGNATURES``: the decoder head's backward and the attention rows' occupancy, rfuse/ops.py), all from the
same shared object, under the same status rule.
"""
import ctypes
import os
import re
from pathlib import Path

import torch  # noqa: F401  (loads libamdhip64 before we dlopen)

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get('RFUSE_LIB', _HERE / 'librfuse_hip.so'))
HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse.h'
EVAL_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_eval.h'
TRAIN_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_train.h'
CONTRASTIVE_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_contrastive.h'
PAIRS_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_pairs.h'
ATTN_TRAIN_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_attn_train.h'
LEVEL_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_level.h'
DATA_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_data.h'
OPTIM_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_optim.h'
STEP_HEADER_PATH = _HERE.parents[1] / 'include' / 'rfuse_step.h'

# every scalar type include/rfuse.h uses; any pointer is a c_void_p, and `const char*` as a return type a c_char_p
_SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t, 'int64_t': ctypes.c_int64, 'long long': ctypes.c_int64}


def parse_header(text):
    """name -> (restype, [argtypes], [parameter names]) for every function declaration of a header written in the vocabulary of
    include/rfuse.h: block comments, preprocessor lines, the ``extern "C" {`` ... ``}`` bracket and declarations ``type name(type name, ...);``
    that may span lines.  Anything else (a type outside _SCALARS, a parameter without a name, text that is no complete declaration)
    raises: a wrong guess here is a wrong foreign call."""
    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\}', ' ', text)

    def where(chunk):
        m = re.search(r'(\w+)\s*\(', chunk)
        return '%s: %r' % (m.group(1) if m else '?', ' '.join(chunk.split()))

    *decls, rest = text.split(';')
    if rest.strip():
        raise ValueError('declaration without its `;` -- %s' % where(rest))

    def ctype(decl, fn, restype=False):
        decl = ' '.join(decl.replace('*', ' * ').split())
        if restype and decl == 'const char *':
            return ctypes.c_char_p
        if decl.endswith('*'):
            return ctypes.c_void_p
        if decl not in _SCALARS:
            raise ValueError('%s: type %r is outside the vocabulary of the binding (%s, pointers)' % (fn, decl, ', '.join(_SCALARS)))
        return _SCALARS[decl]

    table = {}
    for decl in decls:
        m = re.fullmatch(r'\s*([\w\s*]+?)\b(\w+)\s*\(([\w\s*,]*)\)\s*', decl)
        if m is None:
            raise ValueError('cannot read the declaration of %s' % where(decl))
        ret, fn, params = m.groups()
        params = [] if params.strip() == 'void' else [re.fullmatch(r'\s*(\w[\w\s*]*[\s*])(\w+)\s*', q) for q in params.split(',')]
        if None in params:
            raise ValueError('%s: every parameter needs a type and a name' % fn)
        table[fn] = (ctype(ret, fn, True), [ctype(q.group(1), fn) for q in params], [q.group(2) for q in params])
    return table


# name -> (restype, argtypes, parameter names): include/rfuse.h is the only description of the ABI
SIGNATURES = parse_header(HEADER_PATH.read_text())
EVAL_SIGNATURES = parse_header(EVAL_HEADER_PATH.read_text())
TRAIN_SIGNATURES = parse_header(TRAIN_HEADER_PATH.read_text())
CONTRASTIVE_SIGNATURES = parse_header(CONTRASTIVE_HEADER_PATH.read_text())
PAIRS_SIGNATURES = parse_header(PAIRS_HEADER_PATH.read_text())
ATTN_TRAIN_SIGNATURES = parse_header(ATTN_TRAIN_HEADER_PATH.read_text())
LEVEL_SIGNATURES = parse_header(LEVEL_HEADER_PATH.read_text())
DATA_SIGNATURES = parse_header(DATA_HEADER_PATH.read_text())
OPTIM_SIGNATURES = parse_header(OPTIM_HEADER_PATH.read_text())
STEP_SIGNATURES = parse_header(STEP_HEADER_PATH.read_text())


def is_status(name, table=None):
    """The header's rule: an ``int`` function whose last parameter is ``stream`` launches and returns 0 or an RF_E_* code; every other function returns a value."""
    res, _, params = (SIGNATURES if table is None else table)[name]
    return res is ctypes.c_int and params[-1:] == ['stream']


def _raise_on_status(rc, fn, args):
    if rc != 0:
        check(rc, fn.__name__)
    return rc


_lib = None
_eval = None
_train = None
_contrastive = None
_pairs = None
_attn_train = None
_level = None
_data = None
_optim = None
_step = None


class _Library:
    """The bound entry points as plain attributes (no indirection on the hot path; the status check is the binding's own ``errcheck``).
    ``start_profile`` swaps every ``int`` entry point that takes arguments for a wrapper that brackets the call with HIP events on the launch stream and records
    (name, integer arguments, start, end, positions of the null pointer arguments) -- bench.py's per-kernel table; ``stop_profile`` restores the direct bindings."""

    def __init__(self, cdll, table=SIGNATURES):
        self._cdll = cdll
        self._table = table
        self._direct = {}
        for name, (res, args, _) in table.items():
            fn = getattr(cdll, name)      # AttributeError here == header/library mismatch
            fn.restype = res
            fn.argtypes = args
            if is_status(name, table):
                fn.errcheck = _raise_on_status      # a failed launch raises where it is made, under its own symbol
            self._direct[name] = fn
            setattr(self, name, fn)

    def start_profile(self, records, only=None):
        """``only``: a set of entry-point names -- bracket just those (the timed region of bench.py times its one dominant entry point this way)."""
        def timed(name, fn):
            def call(*args):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*args)
                e1.record()
                records.append((name, tuple(a for a in args if isinstance(a, int)), e0, e1, tuple(i for i, a in enumerate(args) if a is None or (isinstance(a, ctypes.c_void_p) and not a.value))))
                return rc
            return call
        for name, (res, args, _) in self._table.items():
            if only is not None and name not in only:
                continue
            if res is ctypes.c_int and args:     # the launches, and the *_supported / *_tiles queries made between them
                setattr(self, name, timed(name, self._direct[name]))

    def stop_profile(self):
        for name, fn in self._direct.items():
            setattr(self, name, fn)


def load():
    """dlopen the library (once) and attach argument/return types and the status check.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(
            'librfuse_hip.so not found at %s -- build it with `python retrieval-fuse_amd/csrc/build.py` '
            '(or __graft_entry__.build()).  There is no CPU fallback for the refinement hot path.' % LIB_PATH)
    _lib = _Library(ctypes.CDLL(str(LIB_PATH)))
    return _lib


def load_eval():
    """The entry points of include/rfuse_eval.h, bound from the library ``load()`` opened (one dlopen, one rf_last_error)."""
    global _eval
    if _eval is None:
        _eval = _Library(load()._cdll, EVAL_SIGNATURES)
    return _eval


def load_train():
    """The entry points of include/rfuse_train.h, bound like ``load_eval()``'s."""
    global _train
    if _train is None:
        _train = _Library(load()._cdll, TRAIN_SIGNATURES)
    return _train


def load_contrastive():
    """The entry points of include/rfuse_contrastive.h, bound like ``load_eval()``'s."""
    global _contrastive
    if _contrastive is None:
        _contrastive = _Library(load()._cdll, CONTRASTIVE_SIGNATURES)
    return _contrastive


def load_pairs():
    """The entry points of include/rfuse_pairs.h, bound like ``load_eval()``'s."""
    global _pairs
    if _pairs is None:
        _pairs = _Library(load()._cdll, PAIRS_SIGNATURES)
    return _pairs


def load_attn_train():
    """The entry points of include/rfuse_attn_train.h, bound like ``load_eval()``'s."""
    global _attn_train
    if _attn_train is None:
        _attn_train = _Library(load()._cdll, ATTN_TRAIN_SIGNATURES)
    return _attn_train


def load_level():
    """The entry points of include/rfuse_level.h, bound like ``load_eval()``'s (its ``start_profile`` brackets them: their launch log)."""
    global _level
    if _level is None:
        _level = _Library(load()._cdll, LEVEL_SIGNATURES)
    return _level


def load_data():
    """The entry points of include/rfuse_data.h, bound like ``load_eval()``'s."""
    global _data
    if _data is None:
        _data = _Library(load()._cdll, DATA_SIGNATURES)
    return _data


def load_optim():
    """The entry points of include/rfuse_optim.h, bound like ``load_eval()``'s."""
    global _optim
    if _optim is None:
        _optim = _Library(load()._cdll, OPTIM_SIGNATURES)
    return _optim


def load_step():
    """The entry points of include/rfuse_step.h, bound like ``load_eval()``'s (its ``start_profile`` brackets them)."""
    global _step
    if _step is None:
        _step = _Library(load()._cdll, STEP_SIGNATURES)
    return _step


def check(rc, what):
    """For callers that bind an entry point themselves; the bindings of ``load()`` check their own status."""
    if rc != 0:
        msg = load().rf_last_error()
        raise RuntimeError('%s failed (rc=%d): %s' % (what, rc, msg.decode() if msg else ''))
