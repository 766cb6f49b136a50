"""CPU: rfuse/routes.py, the one place that chooses a conv layer's kernel form, as a literal table of arguments -> route.  The planner reads only
the library's host-side queries (no GPU call) and the ops switches, so the table runs wherever the library is built.  Every route name appears; every
threshold a query applies on these shapes has a neighbour row one step outside, which falls to the next form.  (The forms' arithmetic is GPU-tested:
tests/test_kernels_gpu.py, tests/test_conditioning_gpu.py.)"""
import sys
from pathlib import Path

import pytest

sys.path[:0] = [str(Path(__file__).resolve().parents[1] / 'retrieval-fuse_amd')]
from rfuse import ops, routes  # noqa: E402

YES, NO = (lambda: True), (lambda: False)


def BOOM():
    raise AssertionError('a range check was asked on a shape the form does not take')


# (n, c0, c1, edge, cout, pool, split_ok) -> route in inference, route in training (the concatenation written out)
SINGLE = [
    ((4096, 32, 0, 4, 64, None, True), 'split_box', 'split_box'),           # whole 4^3 samples: from 1024 samples on
    ((1024, 32, 0, 4, 64, None, True), 'split_box', 'split_box'),
    ((1023, 32, 0, 4, 64, None, True), 'generic', 'generic'),
    ((4096, 32, 0, 4, 64, None, False), 'generic', 'generic'),
    ((4096, 32, 0, 4, 64, 'also', False), 'pool_fp32', 'generic'),          # out of range, pooled: the fp32 kernel with the fused max-pool
    ((4096, 32, 0, 4, 64, 'also', True), 'split_box', 'split_box'),
    ((8192, 64, 0, 2, 128, None, True), 'e2', 'e2'),                        # whole 2^3 volumes as one GEMM: from 16 samples on
    ((16, 64, 0, 2, 128, None, True), 'e2', 'e2'),
    ((15, 64, 0, 2, 128, None, True), 'generic', 'generic'),
    ((8192, 64, 0, 2, 128, None, False), 'generic', 'generic'),
    ((15, 128, 0, 1, 128, None, True), 'direct', 'direct'),                 # 1^3: only the centre tap touches data
    ((16, 128, 0, 1, 128, None, True), 'e2', 'e2'),
    ((16, 128, 0, 1, 128, None, False), 'direct', 'direct'),
    ((2048, 16, 0, 8, 16, None, True), 'split_box', 'split_box'),           # 8^3 boxes, <= 32 couts: from 256 boxes on
    ((256, 16, 0, 8, 16, None, True), 'split_box', 'split_box'),
    ((255, 16, 0, 8, 16, None, True), 'generic', 'generic'),
    ((2048, 16, 0, 8, 16, None, False), 'generic', 'generic'),
    ((2048, 16, 0, 8, 16, 'only', False), 'pool_fp32', 'generic'),
    ((256, 32, 64, 8, 56, None, True), 'up_split', 'split_box'),            # THE ORDER DIFFERENCE: decoder form first in inference, box kernel first in training
    ((255, 32, 64, 8, 56, None, True), 'split_box_concat', 'split_box'),    # the decoder form on whole 8^3 samples: from 256 samples on; the box kernel takes 255 x 4 cout blocks
    ((256, 32, 64, 8, 56, None, False), 'up_fp32', 'generic'),              # the fp32 decoder form: from 256 boxes x cout blocks on
    ((255, 32, 64, 8, 56, None, False), 'generic', 'generic'),
    ((256, 32, 64, 8, 72, None, True), 'split_box_concat', 'split_box'),    # 72 couts: five blocks of 16, the decoder form has 3 or 4
    ((16, 96, 192, 16, 96, None, True), 'split_box_concat', 'split_box'),   # C5's decoder stage: 192 upsampled channels are past the decoder forms
    ((16, 96, 192, 16, 96, None, False), 'up_fp32', 'generic'),
    ((16, 64, 128, 2, 64, None, True), 'e2_concat', 'e2'),                  # decoder stage on 2^3 volumes
    ((15, 64, 128, 2, 64, None, True), 'generic', 'generic'),
    ((16, 64, 128, 2, 64, None, False), 'generic', 'generic'),
]

# (n, c0, c1, edge, cmid, cout, groups2, pool, grad), keywords -> route; both range checks pass unless the keywords say otherwise
PAIR = [
    ((2048, 1, 0, 16, 8, 16, 8, None, False), {}, 'cin1_presplit'),         # level 0 of the retrieval backbone (tests/test_kernels_gpu.py: n = 2048, 2049)
    ((2049, 1, 0, 16, 8, 16, 8, 'also', False), {}, 'cin1_presplit'),
    ((2048, 1, 0, 16, 8, 16, 8, 'only', False), {}, 'cin1_presplit'),
    ((2048, 1, 0, 8, 8, 16, 8, None, False), {}, 'plain'),                  # 16^3 samples only
    ((2048, 1, 0, 16, 8, 16, 8, None, True), {}, 'plain'),                  # the hand-overs have no backward
    ((2048, 1, 0, 16, 8, 16, 8, None, False), {'range2': NO}, 'plain'),
    ((2048, 1, 0, 16, 8, 16, 8, None, False), {'range1': BOOM}, 'cin1_presplit'),      # the 1-channel conv runs fp32 arithmetic: its range is never asked
    ((2100, 1, 0, 16, 8, 16, 8, 'only', False), {'next_takes': YES, 'next_groups': 8}, 'cin1_presplit_handed'),
    ((2100, 1, 0, 16, 8, 16, 8, 'only', False), {'next_takes': NO, 'next_groups': 8}, 'cin1_presplit'),
    ((2100, 1, 0, 16, 8, 16, 8, 'also', False), {'next_takes': BOOM, 'next_groups': 8}, 'cin1_presplit'),   # a skip level keeps its full-resolution output
    ((512, 1, 0, 16, 8, 16, 8, 'only', False), {'next_takes': YES, 'next_groups': 8}, 'cin1_presplit_handed'),       # the persistent consumer: from 512 samples on
    ((511, 1, 0, 16, 8, 16, 8, 'only', False), {'next_takes': YES, 'next_groups': 8}, 'cin1_presplit'),
    ((2100, 16, 0, 8, 16, 32, 8, None, False), {'offered': True}, 'prepooled'),        # level 1 asked by level 0 (accepts_prepooled(2100, 16, 8)): from 2048 boxes on
    ((2048, 16, 0, 8, 16, 32, 8, None, False), {'offered': True}, 'prepooled'),
    ((2047, 16, 0, 8, 16, 32, 8, None, False), {'offered': True, 'range1': BOOM, 'range2': BOOM}, 'plain'),
    ((2100, 16, 0, 8, 16, 32, 8, None, False), {'offered': True, 'range1': NO, 'range2': BOOM}, 'plain'),
    ((1030, 32, 64, 8, 56, 16, 8, None, False), {}, 'decoder_presplit'),    # StepDownDoubleConv 96 -> 56 -> 16 @8^3 (tests: 1030, 1025 linear; 2100, 2070 parity-major)
    ((1025, 32, 48, 8, 48, 16, 8, None, False), {}, 'decoder_presplit'),
    ((2100, 32, 64, 8, 56, 16, 8, None, False), {}, 'decoder_presplit_pm'),
    ((2070, 32, 48, 8, 56, 32, 8, None, False), {}, 'decoder_presplit_pm'),
    ((2048, 32, 64, 8, 56, 16, 8, None, False), {}, 'decoder_presplit_pm'), # persistent producer and persistent consumer: from 2048 samples on
    ((2047, 32, 64, 8, 56, 16, 8, None, False), {}, 'decoder_presplit'),
    ((2100, 0, 64, 8, 56, 16, 8, None, False), {}, 'decoder_presplit'),     # no skip source: linear order
    ((256, 32, 64, 8, 56, 16, 8, None, False), {}, 'decoder_presplit'),
    ((255, 32, 64, 8, 56, 16, 8, None, False), {'range1': BOOM, 'range2': BOOM}, 'plain'),
    ((1030, 32, 64, 8, 56, 16, 8, 'also', False), {'range1': BOOM, 'range2': BOOM}, 'plain'),
    ((1030, 32, 64, 8, 56, 16, 8, None, False), {'encoder_forms': False}, 'decoder_presplit'),
    ((1030, 16, 0, 8, 16, 32, 8, None, False), {}, 'box_presplit'),         # encoder level 16 -> 16 -> 32 @8^3 (tests: 1030, 2070), with every pool
    ((2070, 16, 0, 8, 16, 32, 8, 'only', False), {}, 'box_presplit'),
    ((256, 16, 0, 8, 16, 32, 8, 'also', False), {}, 'box_presplit'),
    ((255, 16, 0, 8, 16, 32, 8, None, False), {'range1': BOOM, 'range2': BOOM}, 'plain'),
    ((1030, 16, 0, 8, 16, 32, 8, None, False), {'range1': YES, 'range2': NO}, 'plain'),
    ((1030, 16, 0, 8, 16, 32, 8, None, False), {'encoder_forms': False, 'range1': BOOM, 'range2': BOOM}, 'plain'),
    ((1030, 16, 0, 8, 32, 32, 8, None, False), {'range1': BOOM, 'range2': BOOM}, 'plain'),          # the producer writes 8 or 16 couts
]

# (n, c1, edge, cmid, cout), range1, range2 -> route
HEAD = [
    ((32, 16, 64, 16, 16), YES, YES, 'ch8'),                                # C1-C4 final decoder: 16 @32^3 upsampled -> 16 -> 16 @64^3 -> 1
    ((4, 16, 64, 16, 16), YES, YES, 'ch8'),                                 # the persistent consumer: from 2048 boxes on
    ((3, 16, 64, 16, 16), BOOM, YES, 'pointwise'),
    ((32, 16, 64, 16, 16), NO, YES, 'pointwise'),
    ((32, 16, 64, 16, 16), YES, NO, 'plain'),
    ((16, 12, 64, 12, 12), BOOM, YES, 'pointwise'),                         # C5: 12 channels are no whole channel groups of 8
    ((16, 8, 64, 8, 8), BOOM, BOOM, 'plain'),                               # the pointwise epilogue: from 12 input channels on
]

L = lambda n, cin, s, cout, k, stride, ok=YES: (n, cin, s, cout, k, stride, ok)
# layer, in_split, next layer -> (form, writes_split)
VALID = [
    (L(16, 1, 144, 12, 5, 1, BOOM), False, L(16, 12, 140, 24, 3, 1), ('valu', True)),          # PCPatch48 on C5's padded chunk: VALU first layer ...
    (L(16, 12, 140, 24, 3, 1), True, L(16, 24, 138, 48, 3, 2), ('grid', True)),                # ... the persistent grid form on even edges 64..254 ...
    (L(16, 12, 141, 24, 3, 1), True, L(16, 24, 139, 48, 3, 2), ('split', True)),
    (L(16, 12, 140, 24, 3, 1), True, None, ('split', False)),
    (L(16, 12, 140, 24, 3, 1), False, L(16, 24, 138, 48, 3, 2), ('split', True)),               # (from an fp32 input: the split form is asked before the VALU form)
    (L(16, 24, 138, 48, 3, 2), False, None, ('split', False)),
    (L(16, 24, 138, 48, 3, 2, NO), False, None, ('gather', False)),
    (L(16, 12, 30, 24, 3, 1, NO), False, L(16, 24, 28, 48, 3, 2), ('valu', True)),              # a weight out of range: the VALU form (12 -> 24, edges up to 64) ...
    (L(16, 12, 30, 24, 3, 1, NO), False, L(16, 24, 28, 48, 3, 2, NO), ('valu', False)),         # ... which writes split form only for a consumer in range
    (L(16, 1, 32, 8, 5, 1, BOOM), False, L(16, 8, 28, 16, 3, 1), ('valu', True)),              # Patch32 on its 32^3 windows
    (L(16, 1, 32, 8, 5, 1, BOOM), False, L(16, 8, 28, 16, 3, 1, NO), ('valu', False)),
    (L(16, 8, 28, 16, 3, 1), False, None, ('split', False)),
    (L(16, 8, 28, 16, 3, 1, NO), False, None, ('valu', False)),
    (L(16, 16, 26, 32, 3, 2, NO), False, None, ('lds', False)),                                 # stride 2 is past the VALU form: LDS-staged fp32 MFMA (output edge >= 8)
    (L(16, 64, 10, 64, 3, 2, NO), False, None, ('gather', False)),
    (L(16, 64, 4, 64, 4, 1), False, None, ('gather', False)),                                   # in range, but a 4^3 window is below every tiled form
    (L(16, 1, 64, 8, 5, 1, BOOM), False, None, ('valu', False)),                                # the VALU form: edges up to 64, or above in fours (the wide tiling)
    (L(16, 1, 65, 8, 5, 1, BOOM), False, None, ('gather', False)),
    (L(16, 1, 68, 8, 5, 1, BOOM), False, None, ('valu', False)),
]


@pytest.mark.parametrize('args,infer,train', SINGLE)
def test_single(args, infer, train):
    assert routes.single(*args, materialised=False) == infer
    n, c0, c1, edge, cout, pool, split_ok = args
    assert routes.single(n, c0, c1, edge, cout, None, split_ok, materialised=True) == train


@pytest.mark.parametrize('args,kw,route', PAIR)
def test_pair(args, kw, route):
    kw = dict({'range1': YES, 'range2': YES}, **kw)
    assert routes.pair(*args, kw.pop('range1'), kw.pop('range2'), **kw) == route


@pytest.mark.parametrize('args,range1,range2,route', HEAD)
def test_head(args, range1, range2, route):
    assert routes.head(*args, range1, range2) == route


@pytest.mark.parametrize('layer,in_split,nxt,expect', VALID)
def test_valid(layer, in_split, nxt, expect):
    assert routes.valid(layer, in_split, nxt) == expect
    if expect[0] in ('lds', 'gather'):
        assert routes.valid(layer, in_split, nxt, fp32_forms=False) == (None, False)


def test_every_route_name_is_in_the_tables():
    assert {r for _, a, b in SINGLE for r in (a, b)} == {'split_box', 'e2', 'e2_concat', 'pool_fp32', 'direct', 'up_split', 'split_box_concat', 'up_fp32', 'generic'}
    assert {r for _, _, r in PAIR} == {'prepooled', 'cin1_presplit', 'cin1_presplit_handed', 'decoder_presplit', 'decoder_presplit_pm', 'box_presplit', 'plain'}
    assert {r for _, _, _, r in HEAD} == {'ch8', 'pointwise', 'plain'}
    assert {e[0] for _, _, _, e in VALID} == {'grid', 'split', 'valu', 'lds', 'gather'}


def test_range_checks_are_asked_once():
    calls = []
    def ask(tag, ok):
        return lambda: calls.append(tag) or ok
    for ok2 in (True, False):
        del calls[:]
        routes.head(32, 16, 64, 16, 16, ask(1, True), ask(2, ok2))           # ch8 asks both; a second layer out of range is not asked again for 'pointwise'
        assert calls == [1, 2]
    del calls[:]
    routes.pair(1030, 16, 0, 8, 16, 32, 8, None, False, ask(1, True), ask(2, True))
    assert calls == [1, 2]
    del calls[:]
    assert routes.valid(L(16, 12, 140, 24, 3, 1, ask(1, True)), True, L(16, 24, 138, 48, 3, 2, ask(2, True))) == ('grid', True)
    assert calls == [2, 1]
    assert routes.split_arith(ask(3, True)) is True and calls[-1] == 3


SWITCHED = [                                                                 # switch, value, call -> with the switch on, with it off
    ('USE_PRESPLIT', False, lambda: routes.pair(1030, 16, 0, 8, 16, 32, 8, None, False, YES, YES), 'box_presplit', 'plain'),
    ('USE_PRESPLIT', False, lambda: routes.pair(2100, 16, 0, 8, 16, 32, 8, None, False, YES, YES, offered=True), 'prepooled', 'plain'),
    ('USE_PREPOOL', False, lambda: routes.pair(2100, 1, 0, 16, 8, 16, 8, 'only', False, YES, YES, next_takes=YES, next_groups=8), 'cin1_presplit_handed', 'cin1_presplit'),
    ('USE_CH8', False, lambda: routes.head(32, 16, 64, 16, 16, YES, YES), 'ch8', 'pointwise'),
    ('USE_CONV_UP', False, lambda: routes.single(256, 32, 64, 8, 56, None, False, False), 'up_fp32', 'generic'),
    ('USE_CONV_UP', False, lambda: routes.single(1024, 32, 64, 4, 56, None, True, False), 'up_split', 'generic'),
    ('USE_FUSED_POOL', False, lambda: routes.single(2048, 16, 0, 8, 16, 'only', False, False), 'pool_fp32', 'generic'),
    ('USE_SPLIT_CHAIN', False, lambda: routes.valid(L(16, 12, 140, 24, 3, 1), True, L(16, 24, 138, 48, 3, 2)), ('grid', True), ('split', False)),
    ('USE_CONVV_VALU', False, lambda: routes.valid(L(16, 1, 32, 8, 5, 1), False, None), ('valu', False), ('lds', False)),
    ('CONV_ARITH', 'fp32', lambda: routes.split_arith(YES), True, False),
    ('CONV_ARITH', 'fp32', lambda: routes.pair(1030, 32, 64, 8, 56, 16, 8, None, False, YES, YES), 'decoder_presplit', 'plain'),
    ('CONV_ARITH', 'fp32', lambda: routes.head(32, 16, 64, 16, 16, YES, YES), 'ch8', 'plain'),
    ('CONV_ARITH', 'fp32', lambda: routes.valid(L(16, 24, 138, 48, 3, 2), False, None), ('split', False), ('gather', False)),
]


@pytest.mark.parametrize('switch,value,call,on,off', SWITCHED)
def test_switches_are_read_at_call_time(switch, value, call, on, off):
    assert call() == on
    saved = getattr(ops, switch)
    setattr(ops, switch, value)
    try:
        assert call() == off
    finally:
        setattr(ops, switch, saved)
    assert call() == on
