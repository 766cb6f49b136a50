"""The fixed-order reductions of csrc/lane_reduce.h, helper by helper: which lane ends up with which value, and in which order the values are added.

The "bit-equal between routes" tests of the conv kernels hold only while every route reduces its GroupNorm statistics in one order; this file pins
that order at its source.  One wave (tests/testkit: rft_lane_reduce_probe) calls each helper on per-lane inputs and stores every lane's result:
  * small integers -- every order gives the same exact result, so plain numpy sums and maxima say which lane must hold what;
  * float64 values whose sum depends on the order (magnitude 2^20, random signs and mantissas: every add of every level rounds) -- compared bit
    for bit with a numpy emulation that adds in the documented partner order.  That the inputs tell that order from its neighbours (a swapped
    pair of masks, at the start or at the end of the tree) is asserted on the emulation itself.
The workgroup reductions (wave totals in wave order, the maximum over waves, the halving tree) get the same treatment on 32 workgroups of 256 threads
(rft_block_reduce_probe), at the end of this file: which thread holds what, the order of the adds against its neighbours, and the sign of a zero sum.
"""
import numpy as np
import pytest
import torch

import testkit

pytestmark = pytest.mark.gpu
LANES = np.arange(64)


def xor_sum(x, masks):
    """x [64, ...] float64 -> every lane's value after `x += x[lane ^ m]` for m in masks, in that order."""
    for m in masks:
        x = x + x[LANES ^ m]
    return x


def transpose_sum16(v):
    """v [64, 16] -> [64]: step k = 0 .. 3 keeps the half picked by bit k of the lane (set: the upper half) and adds what lane ^ (1 << k) hands over,
    then the survivor is added over lanes ^ 16 and ^ 32."""
    v = v.copy()
    for k in range(4):
        c = 8 >> k
        up = ((LANES >> k) & 1).astype(bool)[:, None]
        send = np.where(up, v[:, :c], v[:, c:2 * c])
        keep = np.where(up, v[:, c:2 * c], v[:, :c])
        v[:, :c] = keep + send[LANES ^ (1 << k)]
    return xor_sum(v[:, 0], (16, 32))


def transpose_slot16(lane):
    return (lane & 1) * 8 + ((lane >> 1) & 1) * 4 + ((lane >> 2) & 1) * 2 + ((lane >> 3) & 1)


def pool_cell(u, v):
    """u, v [64, 4] float32 -> (p0, p1) [64]: 2 x 2 in the registers, the third pair in lane ^ 32, ReLU; NaN propagates (np.maximum does)."""
    p0 = np.maximum(np.maximum(u[:, 0], u[:, 1]), np.maximum(v[:, 0], v[:, 1]))
    p1 = np.maximum(np.maximum(u[:, 2], u[:, 3]), np.maximum(v[:, 2], v[:, 3]))
    p0 = np.maximum(p0, p0[LANES ^ 32])
    p1 = np.maximum(p1, p1[LANES ^ 32])
    return np.maximum(p0, np.float32(0)), np.maximum(p1, np.float32(0))


def run_probe(din, fin):
    dout, fout, iout = testkit.lane_reduce_probe(torch.from_numpy(din).cuda(), torch.from_numpy(fin).cuda())
    torch.cuda.synchronize()
    return dout.cpu().numpy(), fout.cpu().numpy(), iout.cpu().numpy()


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint64 if got.dtype == np.float64 else np.uint32),
                          np.ascontiguousarray(want).view(np.uint64 if want.dtype == np.float64 else np.uint32))


def order_sensitive(seed, n):
    """[64, n] float64 of magnitude 2^20 with random signs and full random mantissas, per (lane, column): the partial sums stay at the magnitude of
    the values, so every add of every level rounds at about the same place and a rounding of the first level still shows in the total -- the result
    depends on the association.  (Signs that alternate with the lane cancel exactly against the first partner, lane ^ 1, and leave every later
    add exact; all-positive values grow by a bit per level and round most early differences away.)"""
    return np.random.default_rng(seed).standard_normal((64, n)) * 2.0 ** 20


def differing(x, y):
    return int((x != y).sum())


def transpose_as_butterfly(v, masks):
    """The transpose sum's result lane by lane, were each value a plain butterfly over `masks`: (1, 2, 4, 8, 16, 32) is the documented tree."""
    return xor_sum(v, masks)[LANES, transpose_slot16(LANES)]


def test_small_integers_say_which_lane_holds_what(gpu):
    rng = np.random.default_rng(5)
    din = rng.integers(-9, 10, size=(64, 18)).astype(np.float64)
    fin = rng.integers(-9, 10, size=(64, 8)).astype(np.float32)
    dout, fout, iout = run_probe(din, fin)
    ab = din[:, :2]
    # pair butterflies: plain sums over the lanes that differ in the mask bits
    group = lambda bits: np.stack([ab[(LANES & ~bits) == (l & ~bits)].sum(axis=0) for l in LANES])
    assert np.array_equal(dout[:, 0:2], group(48))
    assert np.array_equal(dout[:, 2:4], group(7))
    assert np.array_equal(dout[:, 4:6], group(7))
    # transpose sum: lane l holds the wave's total of value slot(l); lanes 0 .. 15 cover every value once
    assert np.array_equal(iout, transpose_slot16(LANES))
    assert sorted(iout[:16].tolist()) == list(range(16))
    assert np.array_equal(dout[:, 6], din[:, 2:].sum(axis=0)[iout])
    # pool cell: plain maxima over the cell, clamped at 0, in both lanes of the exchange; its sums; ReLU'd accumulator sums
    u, v = fin[:, :4], fin[:, 4:]
    cell = np.concatenate([u, v], axis=1).reshape(64, 2, 2, 2)          # [lane][block][x pair][x]
    p = np.maximum(cell.max(axis=(1, 3)), 0)                             # [lane][x pair]
    p = np.maximum(p, p[LANES ^ 32])
    assert np.array_equal(fout, p)
    assert np.array_equal(dout[:, 7], p.sum(axis=1, dtype=np.float64))
    assert np.array_equal(dout[:, 8], (p.astype(np.float64) ** 2).sum(axis=1))
    r = np.maximum(u, 0).astype(np.float64)
    assert np.array_equal(dout[:, 9], r.sum(axis=1))
    assert np.array_equal(dout[:, 10], (r * r).sum(axis=1))


def test_order_sensitive_values_pin_the_partner_order(gpu):
    din = order_sensitive(11, 18)
    rng = np.random.default_rng(12)
    fin = (rng.standard_normal((64, 8)) * 3).astype(np.float32)
    fin[5, 0] = np.nan                                                   # lane 5, block u, first x pair
    ab, v16 = din[:, :2], din[:, 2:]
    # the inputs tell the orders apart (numpy against numpy: says nothing about the kernel, everything about the test): the other direction and the
    # neighbouring trees that differ in one pair of masks, at either end; each in at least 16 results, so that no lucky lane hides a change
    for masks, others in (((16, 32), ((32, 16),)), ((1, 2, 4), ((4, 2, 1), (1, 4, 2), (2, 1, 4))), ((4, 2, 1), ((1, 2, 4), (4, 1, 2), (2, 4, 1)))):
        for other in others:
            assert differing(xor_sum(ab, masks), xor_sum(ab, other)) >= 16, (masks, other)
    want16 = transpose_sum16(v16)
    assert same_bits(want16, transpose_as_butterfly(v16, (1, 2, 4, 8, 16, 32)))          # the halving steps ARE that tree, value by value
    for other in ((1, 2, 4, 8, 32, 16), (2, 1, 4, 8, 16, 32), (1, 4, 2, 8, 16, 32), (1, 2, 8, 4, 16, 32), (1, 2, 4, 16, 8, 32), (32, 16, 8, 4, 2, 1)):
        assert differing(want16, transpose_as_butterfly(v16, other)) >= 16, other
    dout, fout, iout = run_probe(din, fin)
    assert same_bits(dout[:, 0:2], xor_sum(ab, (16, 32)))
    assert same_bits(dout[:, 2:4], xor_sum(ab, (1, 2, 4)))
    assert same_bits(dout[:, 4:6], xor_sum(ab, (4, 2, 1)))
    assert same_bits(dout[:, 6], want16)
    # pool cell: NaN propagates to both lanes of the exchange (5 and 37) in p0 and its sums, and nowhere else
    u, v = fin[:, :4], fin[:, 4:]
    p0, p1 = pool_cell(u, v)
    assert np.isnan(p0[[5, 37]]).all() and np.isnan(p0).sum() == 2 and not np.isnan(p1).any()
    nan = np.isnan(p0)
    assert np.array_equal(np.isnan(fout[:, 0]), nan) and same_bits(np.where(nan, np.float32(0), fout[:, 0]), np.where(nan, np.float32(0), p0))
    assert same_bits(fout[:, 1], p1)
    d0, d1 = p0.astype(np.float64), p1.astype(np.float64)
    assert np.array_equal(dout[:, 7], d0 + d1, equal_nan=True) and np.isnan(dout[[5, 37], 7]).all()
    assert np.array_equal(dout[:, 8], d0 * d0 + d1 * d1, equal_nan=True)                 # products of float32 values are exact in float64
    # ReLU'd accumulator sums in register order; a NaN accumulator stays NaN (rf_relu)
    sm, sq = np.zeros(64), np.zeros(64)
    for r in range(4):
        t = np.maximum(u[:, r], np.float32(0)).astype(np.float64)
        sm, sq = sm + t, sq + t * t
    assert np.array_equal(dout[:, 9], sm, equal_nan=True) and np.isnan(dout[5, 9]) and np.isnan(dout[:, 9]).sum() == 1
    assert np.array_equal(dout[:, 10], sq, equal_nan=True)


# ------------------------------------------------------------------------------------------------------- workgroup reductions
# 32 workgroups x 256 threads (tests/testkit: rft_block_reduce_probe); the emulations below work on [32 workgroups][256 threads][columns].
WG, NT = 32, 256


def wave_totals(x):
    """x [32, 256, K] -> [32, 4, K]: wave_sum's total of every wave, as lane 0 holds it (partner masks 32, 16, .. 1, the order of wave_sum's loop)."""
    w = x.reshape(WG, 4, 64, -1).transpose(2, 0, 1, 3)                   # lanes first, for xor_sum
    return xor_sum(w, (32, 16, 8, 4, 2, 1))[0]


def waves_sum(r):
    """r [32, 4, K] -> [32, K]: ((r0 + r1) + r2) + r3, from wave 0's own value."""
    return ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]


def tree_sum(x):
    """x [32, 256, K] -> [32, K]: red[t] += red[t + o] for o = 128 .. 1."""
    x = x.copy()
    o = NT // 2
    while o > 0:
        x[:, :o] = x[:, :o] + x[:, o:2 * o]
        o //= 2
    return x[:, 0]


def serial_sum(x):
    """x [32, 256, K] -> [32, K]: one thread adding in thread order, from thread 0's own value."""
    s = x[:, 0].copy()
    for t in range(1, NT):
        s = s + x[:, t]
    return s


def block_inputs(dseed, fseed):
    rng = np.random.default_rng(dseed)
    din = rng.standard_normal((WG, NT, 5)) * 2.0 ** 20                   # order_sensitive()'s values, per (workgroup, thread, column)
    frng = np.random.default_rng(fseed)
    fin = np.stack([frng.standard_normal((WG, NT)) * 2.0 ** 20, np.abs(frng.standard_normal((WG, NT)))], axis=2).astype(np.float32)
    lin = frng.integers(-2 ** 40, 2 ** 40, size=(WG, NT))
    return din, fin, lin


def run_block_probe(din, fin, lin):
    dout, fout, lout = testkit.block_reduce_probe(torch.from_numpy(din).cuda(), torch.from_numpy(fin).cuda(), torch.from_numpy(lin).cuda())
    torch.cuda.synchronize()
    return dout.cpu().numpy(), fout.cpu().numpy(), lout.cpu().numpy()


def test_block_small_integers_say_which_thread_holds_what(gpu):
    rng = np.random.default_rng(21)
    din = rng.integers(-9, 10, size=(WG, NT, 5)).astype(np.float64)
    fin = rng.integers(0, 1000, size=(WG, NT, 2)).astype(np.float32)
    fin[..., 0] -= 500
    lin = rng.integers(-9, 10, size=(WG, NT))
    dout, fout, lout = run_block_probe(din, fin, lin)
    total = din.sum(axis=1)                                              # every one of the 256 inputs counted once, whatever the order
    assert np.array_equal(dout[:, 0], total)                             # wave-order sum: thread k < K holds value k (K = 1: column 0, K = 4: columns 1 .. 4)
    assert np.array_equal(dout[:, 1], total)                             # ... and any thread may read all of them after the barrier (here the last one)
    assert np.array_equal(dout[:, 2], total)                             # 0.0 + the sum
    assert np.array_equal(dout[:, 3], total)                             # halving tree: thread 0
    assert np.array_equal(fout[:, 0], fin[..., 0].sum(axis=1, dtype=np.float64).astype(np.float32))     # |sum| < 2^24: exact in float32
    assert np.array_equal(fout[:, 1], fin[..., 1].max(axis=1)) and np.array_equal(fout[:, 2], fout[:, 1])
    assert np.array_equal(lout[:, 0], lin.sum(axis=1)) and np.array_equal(lout[:, 1], lout[:, 0])


def test_block_order_sensitive_values_pin_the_order(gpu):
    din, fin, lin = block_inputs(31, 32)
    r = wave_totals(din)
    want_waves, want_tree = waves_sum(r), tree_sum(din)
    # the inputs tell each order from its neighbours (numpy against numpy), on the K = 4 columns: 32 workgroups x 4 values = 128 results
    k4 = slice(1, 5)
    right_to_left = ((r[:, 3] + r[:, 2]) + r[:, 1]) + r[:, 0]
    pairs = (r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])
    up_masks = waves_sum(xor_sum(din.reshape(WG, 4, 64, -1).transpose(2, 0, 1, 3), (1, 2, 4, 8, 16, 32))[0])      # wave_sum with its masks the other way round
    for name, other in (('right to left', right_to_left), ('pairs', pairs), ('masks 1 .. 32', up_masks)):
        assert want_waves[:, k4].size == 128 and differing(want_waves[:, k4], other[:, k4]) >= 16, name
    for name, other in (('serial', serial_sum(din)), ('wave first', want_waves)):
        assert differing(want_tree[:, k4], other[:, k4]) >= 16, name
    f0 = fin[..., :1]
    want_ftree = tree_sum(f0)
    assert want_ftree.dtype == np.float32 and differing(want_ftree, serial_sum(f0)) >= 8         # 32 results here
    dout, fout, lout = run_block_probe(din, fin, lin)
    assert same_bits(dout[:, 0], want_waves)
    assert same_bits(dout[:, 1], want_waves)
    assert same_bits(dout[:, 2], 0.0 + want_waves)
    assert same_bits(dout[:, 3], want_tree)
    assert same_bits(fout[:, 0], want_ftree[:, 0])
    assert np.array_equal(fout[:, 1], fin[..., 1].max(axis=1)) and np.array_equal(fout[:, 2], fout[:, 1])
    assert np.array_equal(lout[:, 0], lin.sum(axis=1)) and np.array_equal(lout[:, 1], lout[:, 0])


def test_block_sign_of_zero(gpu):
    """All-(-0.0) inputs: the wave-order sum starts from wave 0's own value and gives -0.0; `0.0 +` it gives the +0.0 that k_gn_partial's sum from a
    literal 0.0 produced (rf_gn_stats keeps writing it that way).  The tree has no zero in front either."""
    din = np.full((WG, NT, 5), -0.0)
    fin = np.zeros((WG, NT, 2), np.float32)
    fin[..., 0] = -0.0
    dout, fout, lout = run_block_probe(din, fin, np.zeros((WG, NT), np.int64))
    assert (dout == 0).all() and (fout == 0).all() and (lout == 0).all()
    assert np.signbit(dout[:, 0]).all() and np.signbit(dout[:, 1]).all()
    assert not np.signbit(dout[:, 2]).any()
    assert np.signbit(dout[:, 3]).all() and np.signbit(fout[:, 0]).all()
