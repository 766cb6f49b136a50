"""The retrieval back end -- exact top-k at every k2, every merge tier, same-scene demotion, patch and row gathers, canvas paste, overlap compose --
against tests/search_ref.py (pinned on the CPU by tests/test_search_ref_cpu.py), bit for bit.

No test here has a near-tie allowance.  The grid family (search_ref.grid_family) is exact in float32 in any summation order, so ids and distance bits must
equal the float64 oracle's, ties included (lower row id first); the Gaussian family has no near-tie for its seeds (asserted on the CPU), so its ids must be
exact too, and its distances are held to the bound of test_kernels_gpu.check_topk (rtol 1e-5, atol 1e-6), the only tolerance of this module."""
import functools

import numpy as np
import pytest
import torch

import nonfinite
import search_ref as sr
from oracle import refpath

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ALGOS = [1, 2, 3]                                               # VALU scan, fp32-MFMA-filtered scan, f16-MFMA-filtered scan
NONE_I64 = -1                                                   # search_ref.NONE as the int64 the key tensors hold


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU visible')
    from rfuse import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                # (a copy: the shared problems are read-only)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def row_bases(n):
    return (0, 0xFFFFFFFE - n)                                  # the second: the last row has the largest id the ABI takes; ids above 2^31 come back positive


@functools.lru_cache(maxsize=None)
def problem(family, n, nq):
    """(emb, q, float32 distance matrix of the float64 oracle): computed once per shape, shared by the tests, never written"""
    emb, q = (sr.grid_family(sr.grid_seed(n, nq), n, nq) if family == 'grid' else sr.gauss_family(sr.gauss_seed(n, nq), n, nq))
    d = sr.dist_f32(q, emb)
    for a in (emb, q, d):
        a.setflags(write=False)
    return emb, q, d


def assert_pairs_equal_keys(dist, idx, keys, what):
    """the (dist, idx) outputs hold exactly what the keys say: NONE -> (+inf, -1), ids as positive int64, distance bits"""
    rd, ri = sr.unpack_keys(keys)
    i = idx.cpu().numpy()
    assert np.array_equal(i, ri), f'{what}: {(i != ri).sum()} row ids differ, first at {np.argwhere(i != ri)[:1].tolist()}: {i[i != ri][:4]} vs {ri[i != ri][:4]}'
    nonfinite.assert_bit_equal_nan(dist, torch.from_numpy(rd), what)


# ------------------------------------------------------------------------------------------------ the scans

@pytest.mark.parametrize('n,nq', sr.SHAPES)
@pytest.mark.parametrize('algo', ALGOS)
def test_topk_every_k2_grid(ops, algo, n, nq):
    """k2 = 1..16 (lists are 8 or 16 wide inside: k2 != k2p everywhere but at 8 and 16), both outputs, both row bases; ids and distance bits equal the oracle's"""
    emb, q, d = problem('grid', n, nq)
    packed, qd = ops.db_pack_embeddings(dev(emb)), dev(q)
    for base in row_bases(n):
        ref16 = sr.topk_keys_from_dist(d, base, 16)
        for k2 in range(1, 17):
            what = f'algo {algo} n {n} nq {nq} base {base} k2 {k2}'
            keys = ops.l2_topk_keys(qd, packed, n, base, k2, algo)
            dist, idx = ops.l2_topk(qd, packed, n, base, k2, algo)
            got = u64(keys)
            assert np.array_equal(got, ref16[:, :k2]), f'{what}: {(got != ref16[:, :k2]).sum()} keys differ, first at {np.argwhere(got != ref16[:, :k2])[:1].tolist()}'
            assert_pairs_equal_keys(dist, idx, ref16[:, :k2], what)
            assert (idx >= 0).all()


@pytest.mark.parametrize('n,nq', sr.SHAPES)
@pytest.mark.parametrize('algo', ALGOS)
def test_topk_gauss(ops, algo, n, nq):
    """unit-norm Gaussian rows (they move the filter margins): exact ids with no allowance -- the seeds have no near-tie -- and check_topk's distance bound"""
    emb, q, d = problem('gauss', n, nq)
    packed, qd = ops.db_pack_embeddings(dev(emb)), dev(q)
    for base in row_bases(n):
        ref16 = sr.topk_keys_from_dist(d, base, 16)
        for k2 in (1, 2, 3, 7, 9, 12, 15):
            what = f'algo {algo} n {n} nq {nq} base {base} k2 {k2}'
            rd, ri = sr.unpack_keys(ref16[:, :k2])
            dist, idx = ops.l2_topk(qd, packed, n, base, k2, algo)
            keys = ops.l2_topk_keys(qd, packed, n, base, k2, algo)
            assert np.array_equal(idx.cpu().numpy(), ri), what
            np.testing.assert_allclose(dist.cpu().numpy(), rd, rtol=1e-5, atol=1e-6, err_msg=what)
            assert_pairs_equal_keys(dist, idx, u64(keys), what + ' (keys vs pairs)')
            if n > 10 and k2 >= 2:
                assert idx[1 % nq, :2].tolist() == [base + 4, base + 9], 'the planted duplicate: lower row id first'


@pytest.mark.parametrize('algo', ALGOS)
def test_topk_short_shards(ops, algo):
    """fewer rows than k2: the tail is (+inf, -1) / NONE"""
    for n in (1, 5, 15):
        emb, q = sr.grid_family(900 + n, n, 5)
        packed, qd = ops.db_pack_embeddings(dev(emb)), dev(q)
        for k2 in range(n + 1, 17):
            ref = sr.topk_keys(q, emb, 40, k2)
            assert (ref[:, n:] == sr.NONE).all() and (ref[:, :n] != sr.NONE).all()
            keys = ops.l2_topk_keys(qd, packed, n, 40, k2, algo)
            dist, idx = ops.l2_topk(qd, packed, n, 40, k2, algo)
            assert np.array_equal(u64(keys), ref), (algo, n, k2)
            assert_pairs_equal_keys(dist, idx, ref, f'algo {algo} n {n} k2 {k2}')
            assert (idx[:, n:] == -1).all() and torch.isposinf(dist[:, n:]).all()


@pytest.mark.parametrize('k2', [2, 12])
@pytest.mark.parametrize('algo', ALGOS)
def test_sharded_search_with_short_and_empty_shards(ops, algo, k2):
    """shards of 5 and 11 rows (fewer than k2 = 12) and an empty one, merged as keys and as pairs: the single scan's lists (k2 = 2: K = 1, the reference's
    shipped retrieval configs)"""
    n, nq = 190, 70
    emb, q = sr.grid_family(77, n, nq)
    qd = dev(q)
    whole = sr.topk_keys(q, emb, 0, k2)
    single = ops.l2_topk_keys(qd, ops.db_pack_embeddings(dev(emb)), n, 0, k2, algo)
    assert np.array_equal(u64(single), whole)
    ks, ds, is_ = [], [], []
    for lo, hi in ((0, 5), (5, 5), (5, 16), (16, n)):
        if hi == lo:                                            # an empty shard contributes lists of NONE (rfuse.database does the same)
            ks.append(torch.full((nq, k2), NONE_I64, dtype=torch.int64, device=DEV))
            ds.append(torch.full((nq, k2), float('inf'), device=DEV)), is_.append(torch.full((nq, k2), -1, dtype=torch.int64, device=DEV))
            continue
        packed = ops.db_pack_embeddings(dev(emb[lo:hi]))
        ks.append(ops.l2_topk_keys(qd, packed, hi - lo, lo, k2, algo))
        d, i = ops.l2_topk(qd, packed, hi - lo, lo, k2, algo)
        ds.append(d), is_.append(i)
    assert_pairs_equal_keys(*ops.topk_merge_keys(torch.stack(ks)), whole, 'merge of keys')
    assert_pairs_equal_keys(*ops.topk_merge(torch.stack(ds), torch.stack(is_)), whole, 'merge of pairs')


# ------------------------------------------------------------------------------------------------ the merges, fed directly

MERGE_BOUNDS = (128, 256, 512, 1024, 2048)                      # k_merge_wave<R> holds 64 R candidates: R = 2, 4, 8, 16, 32, 64


def merge_totals(k2, bounds, top=4096):
    """candidates per query on each side of every tier boundary: the boundary itself and the next total above it that k2 lists can make (boundary + 1 for k2 = 1)"""
    out = []
    for b in bounds:
        out += [b // k2 * k2, (b // k2 + 1) * k2]
    return sorted(set(out + [top // k2 * k2]))


def merge_candidates(rng, nq, total, k2):
    """[nq, total] uint64: few distinct distances (repeats), +inf and NaN bits, ids from a small range (the same key several times), NONE scattered;
    query 0 has fewer real keys than k2 (none for k2 = 1)"""
    vals = np.array([0.0, 0.25, 0.25, 0.5, 1.0, 1.5, 3.0, np.inf, np.nan], dtype=np.float32)
    d = vals[rng.integers(0, len(vals), size=(nq, total))]
    rows = rng.integers(0, 40, size=(nq, total)).astype(np.uint64)
    rows[:, ::7] += np.uint64(0xF0000000)                       # ids above 2^31
    keys = sr.pack_keys(d, rows)
    keys[rng.random((nq, total)) < 0.3] = sr.NONE
    few = min(k2 - 1, 3)
    keep = rng.permutation(total)[:few]
    saved = keys[0, keep].copy()
    keys[0] = sr.NONE
    keys[0, keep] = np.where(saved == sr.NONE, sr.pack_keys(np.float32(2.0), keep), saved)
    return keys


def as_parts(keys, k2, rng, empty_parts=True):
    nq, total = keys.shape
    parts = keys.reshape(nq, total // k2, k2).transpose(1, 0, 2).copy()
    if empty_parts and parts.shape[0] > 2:
        parts[rng.permutation(parts.shape[0])[:max(1, parts.shape[0] // 5)]] = sr.NONE      # whole parts empty
        parts[-1] = parts[0]                                    # and one part present twice: every key of it must come out twice
    return parts


@pytest.mark.parametrize('k2', [1, 8, 16, 64])
def test_merge_keys_every_tier(ops, k2):
    rng = np.random.default_rng(k2)
    seen_tiers = set()
    for total in merge_totals(k2, MERGE_BOUNDS):
        for nq in (1, 4, 5, 9):                                 # 4 queries per workgroup: full, ragged and several workgroups
            parts = as_parts(merge_candidates(rng, nq, total, k2), k2, rng)
            ref = sr.merge_keys(parts)
            assert (ref[0] == sr.NONE).sum() >= 1 or total // k2 <= 2
            d, i = ops.topk_merge_keys(dev(parts.view(np.int64)))
            assert_pairs_equal_keys(d, i, ref, f'k2 {k2} total {total} nq {nq}')
        seen_tiers.add(int(np.searchsorted(MERGE_BOUNDS, total)))
    assert seen_tiers == set(range(6)), seen_tiers


@pytest.mark.parametrize('k2', [1, 16])
def test_merge_pairs_every_tier(ops, k2):
    rng = np.random.default_rng(100 + k2)
    for total in merge_totals(k2, (256, 1024)):                 # k_merge_pairs<CAP>: 256, 1024, 4096
        for nq in (1, 4, 5, 9):
            parts = as_parts(merge_candidates(rng, nq, total, k2), k2, rng)
            ref = sr.merge_keys(parts)
            d, i = sr.unpack_keys(parts)
            d = d.copy()
            d[(i < 0) & (rng.random(i.shape) < 0.5)] = 0.0      # idx < 0 is no candidate whatever distance stands beside it
            gd, gi = ops.topk_merge(dev(d), dev(i))
            assert_pairs_equal_keys(gd, gi, ref, f'k2 {k2} total {total} nq {nq}')


def test_refusals(ops):
    """refused on the host, before any launch"""
    emb, q = sr.grid_family(5, 64, 3)
    packed, qd = ops.db_pack_embeddings(dev(emb)), dev(q)
    for k2 in (0, 17):
        with pytest.raises(RuntimeError):
            ops.l2_topk(qd, packed, 64, 0, k2, 1)
        with pytest.raises(RuntimeError):
            ops.l2_topk_keys(qd, packed, 64, 0, k2, 1)
    with pytest.raises(RuntimeError, match='4096'):
        ops.topk_merge_keys(torch.full((4097, 2, 1), NONE_I64, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match='4096'):
        ops.topk_merge(torch.zeros((257, 2, 16), device=DEV), torch.zeros((257, 2, 16), dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match='1..64'):
        ops.topk_merge_keys(torch.full((2, 2, 65), NONE_I64, dtype=torch.int64, device=DEV))
    meta = torch.zeros((4, 7), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match='K=5'):
        ops.demote_same_scene(torch.zeros((2, 4), device=DEV), torch.zeros((2, 4), dtype=torch.int64, device=DEV), meta, None, 5)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ non-finite input

def poisoned(n, nq, seed):
    """grid data with non-finite components.  Queries: 3 one NaN component, 10 +inf, 20 -inf, 66 (or the last) +inf in the dim where row 2 has +inf (inf - inf:
    that one pair is NaN, every other +inf); rows: 2 and 7 hold +inf, 5 and the last row a NaN.  Returns (emb, q, clean q, ids of the poisoned queries)."""
    emb, q0 = sr.grid_family(seed, n, nq)
    q = q0.copy()
    bad = [3, 10, 20, min(66, nq - 1)]
    q[3, 5] = np.nan
    q[10, 0] = np.inf
    q[20, 63] = -np.inf
    q[bad[3], 17] = np.inf
    emb[2, 17] = np.inf
    emb[7, 40] = np.inf
    emb[5, 9] = np.nan
    emb[n - 1, 3] = np.nan
    return emb, q, q0, bad


def check_nonfinite(ops, algo, emb, q, q0, bad, ref_rows, k2s):
    """ref_rows: the queries the oracle is computed for (all of them when None)"""
    n, nq = emb.shape[0], q.shape[0]
    rows = np.arange(nq) if ref_rows is None else np.asarray(ref_rows)
    d = sr.dist_f32(q[rows], emb)
    at = {int(r): j for j, r in enumerate(rows)}
    assert np.isnan(d[at[3]]).all() and np.isposinf(d[at[10], 0]) and np.isposinf(d[at[20], 0]) and np.isnan(d[:, n - 1]).all()
    assert np.isnan(d[at[bad[3]], 2]) == np.isinf(emb[2, 17])
    packed, qd, qd0 = ops.db_pack_embeddings(dev(emb)), dev(q), dev(q0)
    rows_t = torch.from_numpy(rows).to(DEV)
    clean = torch.from_numpy(np.setdiff1d(np.arange(nq), bad)).to(DEV)
    for k2 in k2s:
        what = f'algo {algo} n {n} nq {nq} k2 {k2}'
        ref = sr.topk_keys_from_dist(d, 1000, k2)
        dist, idx = ops.l2_topk(qd, packed, n, 1000, k2, algo)
        keys = ops.l2_topk_keys(qd, packed, n, 1000, k2, algo)
        assert_pairs_equal_keys(dist[rows_t], idx[rows_t], ref, what)
        kd, ki = sr.unpack_keys(u64(keys))                      # the keys: same ids, same NaN mask, same bits elsewhere (a NaN's payload is the kernel's own)
        assert np.array_equal(ki, idx.cpu().numpy()), what + ' (keys: ids)'
        nonfinite.assert_bit_equal_nan(torch.from_numpy(kd), dist, what + ' (keys: distances)')
        # a poisoned query changes no other query's bits
        dist0, idx0 = ops.l2_topk(qd0, packed, n, 1000, k2, algo)
        assert torch.equal(idx0[clean], idx[clean]) and torch.equal(dist0[clean].view(torch.int32), dist[clean].view(torch.int32)), what + ' (clean queries)'
        # and the lists survive both merges
        md, mi = ops.topk_merge_keys(keys[None].contiguous())
        assert torch.equal(mi, idx), what + ' (merge of keys: ids)'
        nonfinite.assert_bit_equal_nan(md, dist, what + ' (merge of keys)')
        md, mi = ops.topk_merge(dist[None].contiguous(), idx[None].contiguous())
        assert torch.equal(mi, idx), what + ' (merge of pairs: ids)'
        nonfinite.assert_bit_equal_nan(md, dist, what + ' (merge of pairs)')


@pytest.mark.parametrize('n', [190, 4097])
@pytest.mark.parametrize('algo', ALGOS)
def test_topk_nonfinite(ops, algo, n):
    """A NaN distance is a key like any other: it sorts behind +inf, by row id.  Every scan returns the lists of the float64 oracle in float32 key order.
    Second round: only the last row is poisoned, so the filtered scans keep a finite bound (the non-finite first rows of round one leave none) and meet
    the NaN row in the re-check."""
    emb, q, q0, bad = poisoned(n, 70, 31 + n)
    check_nonfinite(ops, algo, emb, q, q0, bad, None, (1, 2, 7, 8, 16))
    emb[[2, 5, 7]] = sr.grid_family(1, 3, 1)[0]
    check_nonfinite(ops, algo, emb, q, q0, bad, None, (2, 16))


@pytest.mark.parametrize('nq', [1990, 2010])
def test_topk_nonfinite_auto_on_each_side_of_the_scan_choice(ops, nq):
    """TOPK_AUTO takes the VALU scan below nq * n = 4e7 and the f16-filtered scan from there on: a query's lists do not depend on which.  The oracle is
    computed for the poisoned queries, their neighbours and every 16th query; every clean query is also compared with the clean launch."""
    n = 20000
    assert (nq * n >= 4.0e7) == (nq == 2010)
    emb, q, q0, bad = poisoned(n, nq, 5)
    rows = sorted(set(bad) | {b + 1 for b in bad} | {b - 1 for b in bad} | set(range(0, nq, 16)) | {nq - 1})
    check_nonfinite(ops, ops.TOPK_AUTO, emb, q, q0, bad, rows, (8,))


@pytest.mark.parametrize('algo', ALGOS)
def test_topk_negative_nan_query(ops, algo):
    """the sign of a NaN does not move it: every distance of the query is NaN, so its list is the k2 lowest rows"""
    n, nq, k2 = 190, 5, 7
    emb, q = sr.grid_family(8, n, nq)
    q = q.copy()
    q[2, 11] = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
    ref = sr.topk_keys(q, emb, 0, k2)
    dist, idx = ops.l2_topk(dev(q), ops.db_pack_embeddings(dev(emb)), n, 0, k2, algo)
    assert idx[2].tolist() == list(range(k2)) and torch.isnan(dist[2]).all()
    assert_pairs_equal_keys(dist, idx, ref, f'algo {algo}')


# ------------------------------------------------------------------------------------------------ same-scene demotion

def demotion_lists(rng, nq, k2, K, meta, offset):
    """query i has pattern (i + offset) % 6: 0 all from its own scene, 1 exactly K others, 2 fewer than K others, 3 missing entries in the middle,
    4 missing entries at the end, 5 anything"""
    scenes = meta[:, 0]
    idx = np.empty((nq, k2), dtype=np.int64)
    qscene = (np.arange(nq) % 4).astype(np.int32)
    for i in range(nq):
        own, other = np.where(scenes == qscene[i])[0], np.where(scenes != qscene[i])[0]
        kind = (i + offset) % 6
        if kind <= 2:
            n_other = (0, min(K, k2), min(K, k2) - 1)[kind]
            where = rng.permutation(k2)[:n_other]
            idx[i] = rng.choice(own, size=k2)
            idx[i, where] = rng.choice(other, size=n_other)
        else:
            idx[i] = rng.integers(0, len(scenes), size=k2)
            if kind == 3 and k2 > 2:
                idx[i, rng.integers(1, k2 - 1)] = -1
                idx[i, 0 if k2 < 4 else 2] = -1
            if kind == 4:
                idx[i, k2 - (1 + i % min(3, k2)):] = -1
    dist = np.sort(rng.random((nq, k2)).astype(np.float32), axis=1)
    dist[idx < 0] = np.inf
    return dist, idx, qscene


@pytest.mark.parametrize('nq', [1, 256, 257])
def test_demote_matches_reference(ops, nq):
    """nq = 256 / 257: a full 256-thread block and one thread of the next"""
    rng = np.random.default_rng(nq)
    meta = np.concatenate([np.repeat(np.arange(4), 10)[:, None], rng.integers(0, 49, size=(40, 6))], 1).astype(np.int32)
    meta_d = dev(meta)
    keeps = [None]
    if nq > 1:
        k = np.ones(nq, dtype=bool)
        k[[0, nq // 2, nq - 1]] = False                         # dropped first, interior and last queries
        keeps.append(k)
    else:
        keeps.append(np.zeros(1, dtype=bool))
    for K in (1, 3, 4, 8):
        for k2 in (K, 2 * K):
            for offset in (range(6) if nq == 1 else (0,)):
                dist, idx, qscene = demotion_lists(rng, nq, k2, K, meta, offset)
                for qs in (None, np.full(nq, -1, dtype=np.int32), qscene, np.where(np.arange(nq) % 5 == 4, -1, qscene).astype(np.int32)):
                    for keep in keeps:
                        rm, rd, ri = sr.demote(dist, idx, meta, qs, K, keep)
                        m, d, i = ops.demote_same_scene(dev(dist), dev(idx), meta_d, None if qs is None else dev(qs), K, None if keep is None else dev(keep))
                        what = f'nq {nq} K {K} k2 {k2} offset {offset} scene {"none" if qs is None else qs[:4]} keep {keep is not None}'
                        assert np.array_equal(m.cpu().numpy(), rm), what
                        assert np.array_equal(i.cpu().numpy(), ri), what
                        assert np.array_equal(bits(d.cpu().numpy()), bits(rd)), what


# ------------------------------------------------------------------------------------------------ gathers

def gather_meta(rng, chunks, K, n_scenes, aligned_z):
    m = np.empty((chunks * 64, K, 7), dtype=np.int32)
    m[..., 0] = rng.integers(0, n_scenes, size=m.shape[:2])
    o = rng.integers(0, 49, size=m.shape[:2] + (3,))
    o[::5] = 48                                                 # boxes in the far corner
    if aligned_z:
        o[..., 2] = o[..., 2] // 4 * 4
    else:
        o[1::4, :, 2] = o[1::4, :, 2] // 4 * 4                  # every z0 % 4, a quarter of them on the vector route
    m[..., 1::2] = o
    m[..., 2::2] = o + 16
    flat = m.reshape(-1, 7)
    flat[3::11, 0] = -1                                         # sentinel rows
    flat[5::13, 0] = n_scenes                                   # a scene beyond the store
    flat[0] = [-1, 0, 16, 0, 16, 0, 16]
    return m


@pytest.mark.parametrize('layout', [0, 1])
@pytest.mark.parametrize('half', [False, True])
def test_gather_patches_matches_reference(ops, half, layout):
    """value = ((v * ratio) - mean) / std, three float32 roundings in that order (ratio 1/3: the product is inexact).  The last round runs a store that
    starts one element behind a 16-byte boundary with every z0 a multiple of 4: only the pointer term of the vector route's guard keeps it off that route."""
    rng = np.random.default_rng(17 + layout)
    vols = (rng.random((3, 64, 64, 64)) * 3).astype(np.float32)
    vols_np = vols.astype(np.float16) if half else vols
    store = dev(vols_np)
    base = torch.empty(vols.size + 8, dtype=store.dtype, device=DEV)
    assert base.data_ptr() % 16 == 0
    shifted = base[1:1 + vols.size].view(3, 64, 64, 64)
    shifted.copy_(store)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == store.element_size()
    trunc, mean, std = 3.0, 0.37, 1.7
    for K in (1, 3):
        for chunks in (1, 2):
            for ratio, st, aligned_z in ((1.0, store, False), (0.75, store, False), (1.0 / 3.0, store, False), (1.0 / 3.0, shifted, True)):
                meta = gather_meta(rng, chunks, K, 3, aligned_z)
                ref = sr.gather_patches(vols_np, meta, chunks, K, trunc, ratio, mean, std, layout)
                got = ops.gather_patches(st, dev(meta), chunks, K, trunc, ratio, mean, std, layout).cpu().numpy()
                assert got.shape == ref.shape
                assert np.array_equal(bits(got), bits(ref)), f'half {half} layout {layout} K {K} chunks {chunks} ratio {ratio} shifted {st is shifted}: {(bits(got) != bits(ref)).sum()} values differ'


def test_gather_rows_matches_reference(ops):
    """widths of one float4, two, and more than one pass of 256 float4; idx = -1, n and n + 5 select the last row"""
    rng = np.random.default_rng(3)
    n = 9
    for width in (4, 8, 1028):
        src = rng.standard_normal((n, width)).astype(np.float32)
        for m in (1, 67):
            idx = rng.integers(0, n, size=m)
            idx[::3] = np.array([-1, n, n + 5])[np.arange(len(idx[::3])) % 3]
            got = ops.gather_rows(dev(src), dev(idx.astype(np.int64))).cpu().numpy()
            assert np.array_equal(bits(got), bits(sr.gather_rows(src, idx))), (width, m)
            if m == 1:
                assert np.array_equal(got[0], src[n - 1])


@pytest.mark.parametrize('round_half', [True, False])
def test_paste_chunks_matches_reference(ops, round_half):
    """two canvases of different strides in one float64 buffer full of a guard value; float16 ties, half subnormals, overflow to inf, NaN and -0.0 among the values.
    (Offsets are even: the kernel stores pairs of doubles.)"""
    rng = np.random.default_rng(4)
    df = (rng.standard_normal((4, 1, 64, 64, 64)) * 20).astype(np.float32)
    special = np.array([1.00048828125, 1.00146484375, -1.00048828125, 2.0 ** -24, 3e-8, 2.9e-8, 2.0 ** -25, 6.1e-5, 6.0e-5, 65504.0, 65519.0, 65520.0, 70000.0, -1e9,
                        np.nan, -0.0, 0.0, -1e-9, np.inf, -np.inf], dtype=np.float32)      # ties to even, subnormals, the overflow threshold, ...
    df[:, 0, 5, 7, :len(special)] = special
    df[1, 0, 63, 63, 64 - len(special):] = special
    a_dims, b_dims = (130, 66, 68), (64, 70, 64)
    size_a = int(np.prod(a_dims))
    flat = np.full(size_a + int(np.prod(b_dims)), -7.5)
    want = flat.copy()
    plans = [((66 * 68, 68), [3, 1], [(0 * 66 + 2) * 68 + 4, (66 * 66 + 0) * 68 + 2]),
             ((70 * 64, 64), [0], [size_a + 6 * 64])]
    flat_d = dev(flat)
    for (sx, sy), sel, dst in plans:
        assert all(o % 2 == 0 for o in dst) and sx % 2 == 0 and sy % 2 == 0
        sr.paste_chunks(df, sel, dst, sx, sy, want, round_half)
        ops.paste_chunks(dev(df), dev(np.array(sel, dtype=np.int32)), dev(np.array(dst, dtype=np.int64)), sx, sy, flat_d, round_half)
    got = flat_d.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isnan(want) | (got.view(np.int64) == want.view(np.int64))      # bits: -0.0 stays -0.0
    assert ok.all(), f'{(~ok).sum()} elements differ, first at {np.argwhere(~ok)[:1].tolist()}'
    pasted = np.zeros(flat.size)
    for (sx, sy), sel, dst in plans:
        sr.paste_chunks(np.ones_like(df), sel, dst, sx, sy, pasted, False)
    assert pasted.sum() == 3 * 64 ** 3 and (got[pasted == 0] == -7.5).all(), 'everything outside the three boxes still holds the guard'
    if round_half:
        a = got[:size_a].reshape(a_dims)
        assert a[5, 9, 4] == 1.0 and a[5, 9, 5] == 1.001953125 and a[5, 9, 7] == 2.0 ** -24 and np.isposinf(a[5, 9, 4 + 11]) and a[5, 9, 4 + 10] == 65504.0


# ------------------------------------------------------------------------------------------------ overlap compose

def overlap_problem(rng, size, stride, K, n_scenes):
    """patches of 16^3 at ``stride``, clipped at the scene's border; mapping rows with database boxes of the clipped extent; distances on a coarse grid so that
    a box mean cannot come near a patch's own distance by accident (asserted by the caller)"""
    boxes = np.array([[x, min(x + 16, size[0]), y, min(y + 16, size[1]), z, min(z + 16, size[2])]
                      for x in range(0, size[0], stride) for y in range(0, size[1], stride) for z in range(0, size[2], stride)], dtype=np.int32)
    P = len(boxes)
    ext = boxes[:, 1::2] - boxes[:, 0::2]
    mapping = np.zeros((P, K, 8), dtype=np.float32)
    for k in range(K):
        o = rng.integers(0, 49, size=(P, 3))
        mapping[:, k, 0] = rng.integers(0, n_scenes, size=P)
        mapping[:, k, 1:7:2] = o
        mapping[:, k, 2:7:2] = o + ext
        sent = rng.random(P) < 0.1
        mapping[sent, k, 0] = -1
        mapping[sent, k, 1:7:2] = 0
        mapping[sent, k, 2:7:2] = ext[sent]
        mapping[:, k, 7] = rng.integers(1, 400, size=P) / 4.0 + 0.123      # k/4 + 0.123: means of such values over boxes of <= 4096 voxels
    return mapping, boxes


def overlap_margin(mapping, boxes, K, size):
    """the smallest |box mean - patch distance| the reference's walk meets (float64 means, as refpath.compose_retrieval_overlap forms them)"""
    margin = np.inf
    for k in range(K):
        dist = np.full(size, np.float32(100))
        for p in range(len(boxes)):
            x0, x1, y0, y1, z0, z1 = boxes[p].tolist()
            mean, cur = dist[x0:x1, y0:y1, z0:z1].astype(np.float64).mean(), float(mapping[p, k, 7])
            margin = min(margin, abs(mean - cur))
            if mean > cur:
                dist[x0:x1, y0:y1, z0:z1] = cur
    return margin


@pytest.mark.parametrize('half', [False, True])
def test_compose_overlap_clipped_boxes(ops, half):
    """a scene that is no cube (48 x 64 x 32), patches at stride 9 clipped at the border: extents 16 / 12 / 3, 16 / 10 / 1 and 16 / 14 / 5 -- the three differ and three
    boxes in ten have a volume that is no multiple of the 256 threads that walk them"""
    rng = np.random.default_rng(6)
    size, K, trunc, ratio = (48, 64, 32), 2, 3.0, 0.75
    vols = (rng.random((3, 64, 64, 64)) * 3).astype(np.float32)
    if half:
        vols = vols.astype(np.float16).astype(np.float32)
    mapping, boxes = overlap_problem(rng, size, 9, K, 3)
    ext = boxes[:, 1::2] - boxes[:, 0::2]
    assert len({tuple(e) for e in ext.tolist()}) > 8 and (np.prod(ext, axis=1) % 256 != 0).mean() > 0.25
    assert overlap_margin(mapping, boxes, K, size) >= 1e-6
    ref = refpath.compose_retrieval_overlap(mapping, boxes, vols, K, trunc, ratio, size=size)
    store = dev(vols).half() if half else dev(vols)
    got = ops.compose_overlap(store, dev(mapping), dev(boxes), K, size, trunc, ratio).cpu().numpy()
    assert np.array_equal(bits(got), bits(ref)), f'{(bits(got) != bits(ref)).sum()} voxels differ'
    assert 0 < (got == np.float32(trunc)).mean() < 1
    # P = 0: nothing to paste, all truncation fill
    empty = ops.compose_overlap(store, torch.empty((0, K, 8), device=DEV), torch.empty((0, 6), dtype=torch.int32, device=DEV), K, size, trunc, ratio).cpu().numpy()
    assert empty.shape == (K,) + size and (empty == np.float32(trunc)).all()
