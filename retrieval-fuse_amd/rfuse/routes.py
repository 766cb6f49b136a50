"""Which kernel form runs a conv layer -- decided here and nowhere else.

Plain functions from ints, bools and callables to a route name; no tensors, no modules.  They read only the library's host-side queries (rf_*_supported:
no GPU call) and the ``ops.USE_*`` / ``ops.CONV_ARITH`` switches, at call time (tests flip them).  model/*.py and ConvGnRelu.forward of rfuse/autograd.py
ask, then run the form that is named.  Range checks (``ops.split_range_ok``: a host sync on a cache miss, an error inside a graph capture) arrive as zero-argument
callables, called at most once each and as late as the choice allows -- a single layer's FIRST, by its module (``split_arith``): out of range, no split form's query is needed.
"""
from . import _lib, ops


def split_arith(range_ok):
    """may this layer run split-operand (F16 matrix core) forms at all: the arithmetic is switched on and the parameters are inside the f16 pairs' range"""
    return ops.CONV_ARITH == 'split' and bool(range_ok())


def single(n, c0, c1, edge, cout, pool, split_ok, materialised):
    """GroupNorm -> conv3 -> ReLU on [n, c0 (+ c1 upsampled channels), edge^3] -> cout; ``split_ok`` from split_arith (false strikes the split forms out:
    the fp32 rows remain); pool: None / 'also' / 'only'.  The first row that takes the layer names the route, 'generic' when none does.
    Two orders, kept as they were: inference reads (skip, low-resolution) as two sources and prefers the decoder form to the split box kernel on a
    concatenation it would have to write; training (``materialised``: autograd has written it, c0 / c1 only say where it came from) tries that box
    kernel first, and has neither the fp32 pool nor the fp32 decoder form."""
    lib, up, cin = _lib.load(), c1 > 0, c0 + c1
    box = lambda: split_ok and bool(lib.rf_conv3d_split_supported(cin, 0, n, edge, cout))
    e2 = lambda: split_ok and edge <= 2 and bool(lib.rf_conv3d_e2_split_supported(cin, n, edge, cout))
    up_split = lambda: split_ok and up and ops.USE_CONV_UP and bool(lib.rf_conv3d_up_split_supported(c0, c1, n, edge, cout))
    direct = lambda: edge == 1
    if materialised:
        order = (('e2', e2), ('direct', direct), ('split_box', box), ('up_split', up_split))
    else:
        order = (('split_box', lambda: not up and box()),
                 ('e2', lambda: not up and e2()),
                 ('e2_concat', lambda: up and edge == 2 and pool is None and e2()),
                 ('pool_fp32', lambda: pool is not None and not up and edge >= 4 and ops.USE_FUSED_POOL and lib.rf_conv3d_pool_supported(c0, 0, n, edge, cout)),
                 ('direct', direct),
                 ('up_split', up_split),
                 ('split_box_concat', lambda: up and edge >= 8 and box()),
                 ('up_fp32', lambda: up and ops.USE_CONV_UP and lib.rf_conv3d_up_supported(c0, c1, n, edge, cout)))
    return next((name for name, takes in order if takes()), 'generic')


def pair(n, c0, c1, edge, cmid, cout, groups2, pool, grad, range1, range2, offered=False, encoder_forms=True, next_takes=None, next_groups=0):
    """Two such layers, [n, c0 (+ c1 upsampled), edge^3] -> cmid -> cout, the second GroupNorm with groups2 groups: can the first hand the second its
    input already normalised and split?  ``grad``: autograd is recording (the hand-overs have no backward); range1 / range2: the two layers' range
    checks, asked last.  ``offered``: the question of the block BEFORE this one, whether this pair would take an ops.PreSplit of [n, c0, edge^3]: 'prepooled' or
    'plain' (a block that then receives one runs 'prepooled' unasked).  ``encoder_forms`` False: the decoder hand-over only (StepDownDoubleConv).
    ``next_takes`` / ``next_groups``: with pool 'only', the next block's answer when offered and its first GroupNorm's groups."""
    if grad or not ops.USE_PRESPLIT or ops.CONV_ARITH != 'split':
        return 'plain'
    lib = _lib.load()
    rest = lambda: lib.rf_conv3d_split_pre_supported(cmid, n, edge, cout) and range1() and range2()
    if offered:
        return 'prepooled' if lib.rf_conv3d_split_pre_presplit_supported(c0, n, edge, cmid, groups2) and rest() else 'plain'
    if c1 == 0 and c0 == 1 and encoder_forms and lib.rf_conv3d_cin1_presplit_supported(n, edge, cmid, groups2) \
            and lib.rf_conv3d_split_pre_supported(cmid, n, edge, cout) and range2():          # (the first layer runs fp32 arithmetic: no range of its own)
        if pool == 'only' and next_takes is not None and next_takes() and ops.USE_PREPOOL \
                and lib.rf_conv3d_split_pre_pool_presplit_supported(cmid, n, edge, cout, next_groups):
            return 'cin1_presplit_handed'
        return 'cin1_presplit'
    if c1 > 0 and pool is None and lib.rf_conv3d_up_split_presplit_supported(c0, c1, n, edge, cmid, groups2) and rest():
        pm = c0 > 0 and lib.rf_conv3d_up_split_presplit_pm_supported(c0, c1, n, edge, cmid, groups2) and lib.rf_conv3d_split_pre_pm_supported(cmid, n, edge, cout)
        return 'decoder_presplit_pm' if pm else 'decoder_presplit'
    if c1 == 0 and encoder_forms and lib.rf_conv3d_split_presplit_supported(c0, n, edge, cmid, groups2) and rest():
        return 'box_presplit'
    return 'plain'


def level(n, c, edge, cmid, cout, groups1, groups2, grad, range1, range2, skip=None):
    """A pooling encoder level, MaxPool3d(2) of [n, c, edge^3] -> GroupNorm(groups1) -> conv -> cmid -> GroupNorm(groups2) -> conv -> cout: 'e2_level' where
    the whole level is one launch (rf_conv3d_e2_level: 4^3 in, both convs on 2^3 volumes), else 'plain' (the max-pool, then ``pair``).  ``skip``: None, or
    (c_skip, tiles, groups) of the decoder stage that reads the output beside a skip tensor with c_skip channels and that many statistics tiles -- the launch
    then writes that GroupNorm's table too, or does not take the level.  Only in place of the very launches whose sums it restates: the pair 'plain', both
    layers 'e2'."""
    if grad or not ops.USE_E2_LEVEL or ops.CONV_ARITH != 'split' or edge != 4:
        return 'plain'
    c_skip, tiles, groups_dec = skip if skip is not None else (0, 0, 0)
    if not _lib.load_level().rf_conv3d_e2_level_supported(n, c, cmid, cout, groups1, groups2, c_skip, tiles, groups_dec):
        return 'plain'
    ok1 = bool(range1())
    ok2 = ok1 and bool(range2())
    if not ok2 or pair(n, c, 0, 2, cmid, cout, groups2, None, False, lambda: ok1, lambda: ok2) != 'plain':
        return 'plain'
    both_e2 = single(n, c, 0, 2, cmid, None, True, False) == 'e2' and single(n, cmid, 0, 2, cout, None, True, False) == 'e2'
    return 'e2_level' if both_e2 else 'plain'


def head(n, c1, edge, cmid, cout, range1, range2):
    """The final decoder's pair + pointwise head: [n, c1, (edge / 2)^3] upsampled -> cmid -> cout @edge^3 -> 1.  'ch8': both convs, channel-interleaved
    hand-over; 'pointwise': the first as a single layer, the head in the second's epilogue; 'plain': two single layers and the 1x1x1 kernel."""
    if ops.CONV_ARITH != 'split':
        return 'plain'
    lib, ok2 = _lib.load(), None
    if ops.USE_CH8 and ops.USE_CONV_UP and lib.rf_conv3d_up_split_ch8_supported(0, c1, n, edge, cmid) \
            and lib.rf_conv3d_split_pointwise_ch8_supported(cmid, n, edge, cout) and range1():
        ok2 = bool(range2())
        if ok2:
            return 'ch8'
    if lib.rf_conv3d_split_pointwise_supported(cmid, n, edge, cout) and (range2() if ok2 is None else ok2):
        return 'pointwise'
    return 'plain'


def _valid_split_takes(lib, n, cin, s, cout, k, stride, range_ok):
    return ops.CONV_ARITH == 'split' and cin % 4 == 0 and range_ok() and bool(lib.rf_conv3d_valid_split_supported(max(n, 1), cin, s, cout, k, stride))


def valid(layer, in_split, nxt=None, fp32_forms=True):
    """valid strided conv + bias + LeakyReLU of the patch encoders -> (form, writes_split).  ``layer`` = (n, cin, s, cout, k, stride, range_ok): [n, cin, s^3]
    (in_split: it arrives as an ops.SplitActs) -> cout; ``nxt``: the same of the layer that reads the output, if any -- writes_split says that this layer
    leaves its output in split form for it (the producer's form and the consumer's both have to be split-form capable).  ``fp32_forms`` False: form None
    where only the LDS-staged / gather forms are left, unasked (forward_grid's question: does a form that tiles a big volume take the layer)."""
    lib, (n, cin, s, cout, k, stride, range_ok) = _lib.load(), layer
    split = in_split or _valid_split_takes(lib, *layer)
    valu = not split and ops.USE_CONVV_VALU and bool(lib.rf_conv3d_valid_valu_supported(max(n, 1), cin, s, cout, k, stride))
    writes = bool(ops.USE_SPLIT_CHAIN and nxt is not None and cout % 4 == 0 and (split or valu) and _valid_split_takes(lib, *nxt))
    if in_split and writes and ops.USE_CONVV_PG and ops.CONV_ARITH == 'split' \
            and lib.rf_conv3d_valid_split_pg_supported(max(n, 1), cin, s, cout, k, stride) and range_ok():
        return 'grid', True
    if split or valu:
        return ('split' if split else 'valu'), writes
    if not fp32_forms:
        return None, False
    return ('lds' if lib.rf_conv3d_valid_lds_supported(n, cin, s, cout, k, stride) else 'gather'), False


def attn_mlp_fused(n_in, n_out):
    """(no conv, but model/'s one other form choice) the attention feature encoder's 4 layers as the fused MFMA kernel (rf_attn_mlp_*)"""
    return ops.USE_FUSED_ATTN_MLP and n_in % 16 == 0 and 16 <= n_in <= 128 and n_out == 32
