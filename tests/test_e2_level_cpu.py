"""CPU: the host side of the one-launch 2^3 level (include/rfuse_level.h, rfuse.routes.level): the header is bound and exported, the shape query says what
its text says, the launcher refuses before anything reaches a device, and the route falls back on every switch."""
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
NAMES = {'rf_conv3d_e2_level_supported', 'rf_conv3d_e2_level'}


def test_level_header_is_bound_and_exported():
    from rfuse import _lib
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'rfuse_level.h').read_text(), flags=re.S)
    assert set(re.findall(r'\b(rf_[a-z0-9_]+)\s*\(', text)) == NAMES == set(_lib.LEVEL_SIGNATURES)
    lib = _lib.load_level()
    assert lib is _lib.load_level() and lib._cdll is _lib.load()._cdll and set(lib._direct) == NAMES
    others = (_lib.SIGNATURES, _lib.EVAL_SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.CONTRASTIVE_SIGNATURES, _lib.PAIRS_SIGNATURES, _lib.ATTN_TRAIN_SIGNATURES)
    assert not any(NAMES & set(t) for t in others)
    assert _lib.is_status('rf_conv3d_e2_level', _lib.LEVEL_SIGNATURES) and not _lib.is_status('rf_conv3d_e2_level_supported', _lib.LEVEL_SIGNATURES)
    build_py = (REPO / 'retrieval-fuse_amd' / 'csrc' / 'build.py').read_text()
    assert "'conv3d_e2_level.hip'" in build_py and "'rfuse_level.h'" in build_py


def test_supported_plans():
    from rfuse import _lib
    q = _lib.load_level().rf_conv3d_e2_level_supported
    assert q(8192, 64, 64, 128, 8, 8, 64, 1, 8) == 1 and q(8192, 64, 64, 128, 8, 8, 0, 0, 0) == 1          # C2's retrieval backbone, with and without the table
    assert q(128, 64, 64, 128, 8, 8, 64, 1, 8) == 1 and q(127, 64, 64, 128, 8, 8, 64, 1, 8) == 0            # 1024 (sample, group) units
    assert q(128, 64, 64, 128, 8, 8, 0, 0, 0) == 1 and q(127, 64, 64, 128, 8, 8, 0, 0, 0) == 0
    assert [q(1024, c, 64, 128, 1, 8, 0, 0, 0) for c in (4, 6, 8, 10, 12, 64, 68)] == [0, 0, 1, 0, 1, 1, 0]    # c = 8 .. 64 in fours
    assert [q(1024, 64, cm, 128, 8, 8, 0, 0, 0) for cm in (32, 64, 128)] == [0, 1, 0]
    assert [q(1024, 64, 64, co, 8, 8, 0, 0, 0) for co in (32, 64, 96, 128, 256)] == [0, 1, 0, 1, 0]
    assert q(1024, 64, 64, 128, 7, 8, 0, 0, 0) == 0 and q(1024, 64, 64, 128, 8, 0, 0, 0, 0) == 0            # groups divide the channels
    assert q(128, 64, 64, 128, 8, 8, 1952, 1, 16) == 0 and q(128, 64, 64, 128, 8, 8, 1920, 1, 16) == 1      # 130 / 128 statistics entries per decoder group
    assert q(128, 64, 64, 128, 8, 8, 64, 2, 8) == 1 and q(128, 64, 64, 128, 8, 8, 64, 6, 8) == 0            # ... counted in tiles
    assert q(128, 64, 64, 128, 8, 8, 64, 0, 8) == 0 and q(128, 64, 64, 128, 8, 8, 64, 1, 4) == 0 and q(128, 64, 64, 128, 8, 8, -1, 1, 8) == 0


def test_launcher_refuses_before_any_device():
    import ctypes
    from rfuse import _lib
    lib, one = _lib.load_level(), ctypes.c_void_p(256)           # a non-null pointer that the argument checks never follow
    with pytest.raises(RuntimeError, match=r'^rf_conv3d_e2_level failed \(rc=-2\): .*n=127'):
        lib.rf_conv3d_e2_level(one, 127, 64, one, one, 8, 1e-5, one, 64, one, one, 8, 1e-5, one, 128, one, one, None, 0, 0, None, None, 0, 0.0, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_conv3d_e2_level failed \(rc=-1\): .*null pointer'):
        lib.rf_conv3d_e2_level(one, 128, 64, one, one, 8, 1e-5, one, 64, one, one, 8, 1e-5, one, 128, one, None, None, 0, 0, None, None, 0, 0.0, None, None)
    with pytest.raises(RuntimeError, match=r'^rf_conv3d_e2_level failed \(rc=-1\): .*decoder table'):
        lib.rf_conv3d_e2_level(one, 128, 64, one, one, 8, 1e-5, one, 64, one, one, 8, 1e-5, one, 128, one, one, one, 64, 1, one, one, 8, 1e-5, None, None)


def test_route_and_its_switches(monkeypatch):
    from rfuse import ops, routes
    yes, calls = (lambda: True), []
    args = (8192, 64, 4, 64, 128, 8, 8, False)
    assert routes.level(*args, yes, yes) == 'e2_level' and routes.level(*args, yes, yes, skip=(64, 1, 8)) == 'e2_level'
    assert routes.level(*args, yes, yes, skip=(1952, 1, 16)) == 'plain'                      # a table the launch cannot write: the level stays as it was
    assert routes.level(8192, 64, 4, 64, 128, 8, 8, True, yes, yes) == 'plain'               # autograd is recording
    assert routes.level(8192, 64, 8, 64, 128, 8, 8, False, yes, yes) == 'plain'              # the convs would not run on 2^3 volumes
    assert routes.level(32, 64, 4, 64, 128, 8, 8, False, yes, yes) == 'plain'                # the chunk-level U-Net: n = B
    assert routes.level(*args, lambda: False, yes) == 'plain' and routes.level(*args, yes, lambda: False) == 'plain'
    counted = lambda: calls.append(1) or True
    assert routes.level(*args, counted, counted) == 'e2_level' and len(calls) == 2            # each range check once
    for name, value in (('USE_E2_LEVEL', False), ('CONV_ARITH', 'fp32')):
        monkeypatch.setattr(ops, name, value)
        assert routes.level(*args, yes, yes) == 'plain'
        monkeypatch.undo()
    assert routes.level(*args, yes, yes) == 'e2_level'
