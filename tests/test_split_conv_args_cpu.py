"""CPU: the refusals of the split-operand conv entry points (csrc/conv3d_split.hip: nine, csrc/conv3d_up_split.hip: four) -- the host layer's
observable contract: every entry point refuses an unsupported shape (rc -2) and a null pointer (rc -1) under its own name, the three with
full / pooled output pairs refuse inconsistent pairs, all before anything reaches a device."""
import ctypes

import pytest

ONE = ctypes.c_void_p(256)                           # a non-null pointer that the argument checks never follow

# name -> (call(shape, pointers...), a supported shape, an unsupported shape, fragment of the unsupported-shape text, number of pointer arguments,
#          which of them may be null at the supported shape: statistics, one of an output pair, a skip source with c0 = 0)
# The callers below put the shape integers and the pointers where each signature wants them; scalars that no check reads are fixed.
SPLIT = {      # shape = (cin, n, edge, cout[, next_groups])
    'rf_conv3d_split_k3_gn_relu': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], p[2], s[3], p[3], p[4], p[5], p[6], None),
                                   (16, 256, 8, 16), (4, 256, 8, 16), r'takes cin >= 6 .*up to 192 couts', 7, (3, 4, 5, 6)),
    'rf_conv3d_split_k3_gn': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], p[2], s[3], 1, p[3], None),
                              (16, 1024, 8, 16), (16, 256, 8, 16), r'takes cin >= 6 .*whole 4\^3 samples', 4, ()),
    'rf_conv3d_split_pre_k3_relu': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], s[3], p[2], p[3], p[4], p[5], None),
                                    (16, 256, 8, 16), (12, 256, 8, 16), r'takes cin in eights, up to 32 couts', 6, (2, 3, 4, 5)),
    'rf_conv3d_split_pre_pm_k3_relu': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], s[3], p[2], p[3], p[4], p[5], None),
                                       (16, 2048, 8, 16), (16, 256, 8, 16), r'takes whole 8\^3 samples \(n >= 2048\)', 6, (2, 3, 4, 5)),
    'rf_conv3d_split_presplit': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], p[2], s[3], p[3], p[4], s[4], 1e-5, p[5], p[6], None),
                                 (16, 256, 8, 16, 2), (16, 256, 8, 16, 3), r'8 or 16 couts in whole groups', 7, (6,)),
    'rf_conv3d_split_k3_gn_relu_pointwise_tanh': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], p[2], s[3], p[3], p[4], 1.0, 0.5, p[5], None),
                                                  (16, 256, 8, 16), (8, 256, 8, 16), r'cin >= 12 and up to 16 couts', 6, ()),
    'rf_conv3d_split_k3_gn_relu_pointwise_tanh_ch8': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], p[2], s[3], p[3], p[4], 1.0, 0.5, p[5], None),
                                                      (16, 2048, 8, 16), (16, 256, 8, 16), r'at least 2048 boxes', 6, ()),
    'rf_conv3d_split_pre_k3_relu_pool_presplit': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], s[3], p[2], p[3], p[4], p[5], s[4], 1e-5, p[6], None),
                                                  (8, 512, 16, 16, 2), (8, 512, 8, 16, 2), r'8 -> 8 or 16 channels on 16\^3 samples', 7, (3,)),
    'rf_conv3d_split_pre_presplit': (lambda f, s, p: f(p[0], s[0], s[1], s[2], p[1], s[3], p[2], p[3], s[4], 1e-5, p[4], p[5], None),
                                     (16, 2048, 8, 16, 2), (16, 256, 8, 16, 2), r'whole 8\^3 samples \(n >= 2048\)', 6, (5,)),
}
UP = {         # shape = (c0, c1, n, edge, cout[, next_groups])
    'rf_conv3d_up_split_k3_gn_relu': (lambda f, s, p: f(p[0], s[0], p[1], s[1], s[2], s[3], p[2], p[3], s[4], p[4], p[5], None),
                                      (0, 8, 256, 8, 64), (0, 8, 1, 8, 8), r'8\^3 samples', 6, (0, 5)),
    'rf_conv3d_up_split_presplit': (lambda f, s, p: f(p[0], s[0], p[1], s[1], s[2], s[3], p[2], p[3], s[4], p[4], p[5], s[5], 1e-5, p[6], p[7], None),
                                    (0, 8, 256, 8, 64, 8), (0, 8, 256, 8, 64, 5), r'cout in eights and in whole groups', 8, (0, 7)),
    'rf_conv3d_up_split_presplit_pm': (lambda f, s, p: f(p[0], s[0], p[1], s[1], s[2], s[3], p[2], p[3], s[4], p[4], p[5], s[5], 1e-5, p[6], p[7], None),
                                       (32, 8, 1024, 8, 64, 8), (0, 8, 1024, 8, 64, 8), r'c0 >= 32 in sixteens', 8, (7,)),
    'rf_conv3d_up_split_k3_gn_relu_ch8': (lambda f, s, p: f(p[0], s[0], p[1], s[1], s[2], s[3], p[2], p[3], s[4], p[4], p[5], None),
                                          (0, 8, 32, 16, 16), (0, 8, 32, 16, 12), r'box form .*cout in eights', 6, (0, 5)),
}


@pytest.mark.parametrize('name', list(SPLIT) + list(UP))
def test_split_entry_points_refuse_under_their_own_name(name):
    from rfuse import _lib
    lib = _lib.load()
    call, good, bad, text, npointers, optional = {**SPLIT, **UP}[name]
    with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-2\): %s: .*%s.*\(got ' % (name, name, text)):
        call(getattr(lib, name), bad, [ONE] * npointers)
    with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-1\): %s: null pointer$' % (name, name)):
        call(getattr(lib, name), good, [None] * npointers)
    for i in set(range(npointers)) - set(optional):       # every required pointer on its own
        with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-1\): %s: null pointer$' % (name, name)):
            call(getattr(lib, name), good, [None if k == i else ONE for k in range(npointers)])


@pytest.mark.parametrize('name', ['rf_conv3d_split_k3_gn_relu', 'rf_conv3d_split_pre_k3_relu', 'rf_conv3d_split_pre_pm_k3_relu'])
def test_output_pairs_are_consistent(name):
    """out / stats / pool_out / pool_stats are the last four pointers of these three: statistics only of an output that is written"""
    from rfuse import _lib
    lib = _lib.load()
    call, good, _, _, npointers, _ = SPLIT[name]
    lead = [ONE] * (npointers - 4)
    with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-1\): %s: null pointer$' % (name, name)):
        call(getattr(lib, name), good, lead + [None, None, None, None])
    with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-1\): %s: statistics of an output that is not written$' % (name, name)):
        call(getattr(lib, name), good, lead + [None, ONE, ONE, None])
    with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-1\): %s: pooled statistics without a pooled output$' % (name, name)):
        call(getattr(lib, name), good, lead + [ONE, None, None, ONE])


def test_the_plain_entry_point_shapes():
    from rfuse import _lib
    lib = _lib.load()
    assert lib.rf_conv3d_split_supported(16, 0, 256, 8, 16) == 1
    assert lib.rf_conv3d_split_supported(8, 0, 1024, 4, 16) == 1
    name = 'rf_conv3d_split_k3_gn_relu'
    with pytest.raises(RuntimeError, match=r'^%s failed \(rc=-2\): %s: the 4\^3 form has no fused max-pool' % (name, name)):
        SPLIT[name][0](getattr(lib, name), (8, 1024, 4, 16), [ONE] * 7)
