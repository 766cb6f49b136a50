"""The fixed-order reductions of csrc/lane_reduce.h, helper by helper: which lane ends up with which value, and in which order the values are added.

The "bit-equal between routes" tests of the conv kernels hold only while every route reduces its GroupNorm statistics in one order; this file pins
that order at its source.  One wave (tests/testkit: rft_lane_reduce_probe) calls each helper on per-lane inputs and stores every lane's result:
  * small integers -- every order gives the same exact result, so plain numpy sums and maxima say which lane must hold what;
  * float64 values whose sum depends on the order (magnitude 2^20, random signs and mantissas: every add of every level rounds) -- compared bit
    for bit with a numpy emulation that adds in the documented partner order.  That the inputs tell that order from its neighbours (a swapped
    pair of masks, at the start or at the end of the tree) is asserted on the emulation itself.
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
