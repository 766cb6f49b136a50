"""The contracts of the retrieval back end in numpy: exact top-k as packed keys, list merge, same-scene demotion, patch and row gathers,
canvas paste.  Test infrastructure: tests/test_search_gpu.py compares the HIP kernels with it, tests/test_distributed_cpu.py runs the
sharded protocol over it, and tests/test_search_ref_cpu.py pins it against oracle/refpath.py and the golden fixtures.

A candidate is ONE unsigned 64-bit key ``dist bits << 32 | global row id``: distances are >= +0, so the unsigned order of the keys is
the order by (distance, row id); +inf sorts after every finite distance and NaN after +inf.  A NaN distance is keyed with the quiet-NaN
pattern 0x7FC00000 whatever its sign or payload, so NaN candidates are ordered by row id alone.  ``NONE`` = 2^64 - 1 is "no candidate":
it unpacks to (+inf, -1).  A merge is a sort of keys; a key present twice stays twice."""
import numpy as np
import torch

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
QNAN_BITS = np.uint32(0x7FC00000)
NO_NEIGHBOUR = np.array([-1, 0, 16, 0, 16, 0, 16], dtype=np.int32)          # the meta row of a missing neighbour (k_demote)


# ------------------------------------------------------------------------------------------------ exact top-k

def dist_f32(q, emb, block=1 << 21):
    """squared L2 distances [nq, n]: float64 differences, squares and sums, rounded to float32 once (inf - inf and NaN propagate as IEEE says)"""
    q, emb = np.asarray(q, dtype=np.float64), np.asarray(emb, dtype=np.float64)
    out = np.empty((q.shape[0], emb.shape[0]), dtype=np.float32)
    step = max(1, block // max(1, emb.shape[0] * emb.shape[1]))
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(0, q.shape[0], step):
            out[s:s + step] = ((q[s:s + step, None, :] - emb[None]) ** 2).sum(-1).astype(np.float32)
    return out


def grid_dist_f32(q, emb):
    """dist_f32 for FINITE dyadic-grid data (grid_family), where |q|^2 + |x|^2 - 2 q.x is exact in float64 in any order: one matrix product"""
    q, emb = np.asarray(q, dtype=np.float64), np.asarray(emb, dtype=np.float64)
    return ((q * q).sum(1)[:, None] + (emb * emb).sum(1)[None] - 2.0 * (q @ emb.T)).astype(np.float32)


def pack_keys(dist, rows):
    """float32 distances and row ids (broadcast against each other) -> uint64 keys; NaN distances take the quiet-NaN pattern"""
    dist = np.asarray(dist, dtype=np.float32)
    bits = np.where(np.isnan(dist), QNAN_BITS, dist.view(np.uint32)).astype(np.uint64)
    return (bits << np.uint64(32)) | np.asarray(rows).astype(np.uint64)


def unpack_keys(keys):
    """uint64 keys -> (dist float32, idx int64); NONE -> (+inf, -1)"""
    keys = np.asarray(keys, dtype=np.uint64)
    none = keys == NONE
    d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    i = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.where(none, np.float32(np.inf), d), np.where(none, np.int64(-1), i)


def topk_keys_from_dist(d, row_base, k2):
    """the k2 smallest keys per query of a float32 distance matrix [nq, n], NONE-padded when n < k2"""
    nq, n = d.shape
    keys = np.full((nq, k2), NONE, dtype=np.uint64)
    if n:
        all_keys = pack_keys(d, (np.arange(n, dtype=np.uint64) + np.uint64(row_base))[None])
        all_keys.sort(axis=1)
        m = min(k2, n)
        keys[:, :m] = all_keys[:, :m]
    return keys


def topk_keys(q, emb, row_base, k2):
    """rf_l2_topk_keys: [nq, k2] uint64"""
    emb = np.asarray(emb)
    if emb.shape[0] == 0:
        return np.full((np.asarray(q).shape[0], k2), NONE, dtype=np.uint64)
    return topk_keys_from_dist(dist_f32(q, emb), row_base, k2)


def topk(q, emb, row_base, k2):
    """rf_l2_topk: (dist [nq, k2] float32, idx [nq, k2] int64)"""
    return unpack_keys(topk_keys(q, emb, row_base, k2))


def merge_keys(parts, k2=None):
    """rf_topk_merge_keys: parts [P, nq, w] uint64 -> the k2 (default w) smallest keys per query, [nq, k2] uint64"""
    parts = np.asarray(parts, dtype=np.uint64)
    p, nq, w = parts.shape
    k2 = w if k2 is None else k2
    flat = np.sort(parts.transpose(1, 0, 2).reshape(nq, p * w), axis=1)
    out = np.full((nq, k2), NONE, dtype=np.uint64)
    out[:, :min(k2, p * w)] = flat[:, :k2]
    return out


def pairs_to_keys(dist, idx):
    """(dist, idx) candidate arrays -> keys; idx < 0 is no candidate whatever its distance"""
    idx = np.asarray(idx, dtype=np.int64)
    return np.where(idx < 0, NONE, pack_keys(dist, np.maximum(idx, 0)))


def merge_pairs(dist_parts, idx_parts):
    """rf_topk_merge: [P, nq, k2] pairs -> (dist [nq, k2], idx [nq, k2])"""
    return unpack_keys(merge_keys(pairs_to_keys(dist_parts, idx_parts)))


# ------------------------------------------------------------------------------------------------ the two data families

SHAPES = ((190, 5), (4097, 70), (131, 300))                     # (rows, queries) of the scans' tests: 1..6 tiles per slice (tests/test_kernels_gpu.py:test_l2_topk)
GAUSS_SEEDS = {(190, 5): 195, (4097, 70): 4167, (131, 300): 436}      # seeds whose data has no near-tie (asserted in tests/test_search_ref_cpu.py)


def grid_seed(n, nq):
    return n + nq


def gauss_seed(n, nq):
    return GAUSS_SEEDS[(n, nq)]


def grid_family(seed, n, nq):
    """embeddings and queries on the dyadic grid {-2..2} / 8: every squared difference (a multiple of 1/64, at most 1/4) and every partial sum of 64 of
    them is exact in float32 in ANY order, so a kernel owes the float64 result bit for bit -- and ties are everywhere (distances take few values)"""
    rng = np.random.default_rng(seed)
    emb = (rng.integers(-2, 3, size=(n, 64)) / 8.0).astype(np.float32)
    q = (rng.integers(-2, 3, size=(nq, 64)) / 8.0).astype(np.float32)
    return emb, q


def gauss_family(seed, n, nq):
    """unit-norm Gaussian rows (they move the filters' margins, which grid data does not), one planted duplicate pair and one exact hit"""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((n, 64)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    q = rng.standard_normal((nq, 64)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if n > 10:
        emb[9] = emb[4]                                            # planted duplicate: lower row id first
        q[1 % nq] = emb[4]
    q[0] = emb[min(7, n - 1)]
    return emb, q


def chain_dist_f32(q, emb):
    """the kernels' float32 summation (four FMA chains over dims 4 m + c, then (c0 + c2) + (c1 + c3)) with every step rounded to float32: on the grid
    family it must equal dist_f32 exactly (tests/test_search_ref_cpu.py); squares of grid differences are exact, so fma = multiply, add"""
    q, emb = np.asarray(q, dtype=np.float32), np.asarray(emb, dtype=np.float32)
    c = np.zeros((4, q.shape[0], emb.shape[0]), dtype=np.float32)
    for m in range(16):
        for g in range(4):
            t = (q[:, None, 4 * m + g] - emb[None, :, 4 * m + g]).astype(np.float32)
            c[g] = (c[g] + (t * t).astype(np.float32)).astype(np.float32)
    return ((c[0] + c[2]).astype(np.float32) + (c[1] + c[3]).astype(np.float32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ same-scene demotion

def demote(dist, idx, meta, query_scene, K, query_keep=None):
    """rf_demote_same_scene.  dist [nq, k2] float32, idx [nq, k2] int64 (-1: missing), meta [n, 7] int32 (column 0: scene), query_scene [nq] (or None;
    < 0: the query's scene is not in the database), query_keep [nq] bool (or None).  Neighbours from the query's own scene go, in order, behind all
    others; a missing neighbour is not of the query's scene and keeps its place, as the entry NO_NEIGHBOUR; a dropped query gives K entries of
    NO_NEIGHBOUR, +inf, -1.  Returns (meta [nq, K, 7] int32, dist [nq, K] float32, idx [nq, K] int64)."""
    dist, idx, meta = np.asarray(dist, dtype=np.float32), np.asarray(idx, dtype=np.int64), np.asarray(meta, dtype=np.int32)
    nq, k2 = idx.shape
    assert 0 < K <= k2
    out_m = np.empty((nq, K, 7), dtype=np.int32)
    out_d = np.empty((nq, K), dtype=np.float32)
    out_i = np.empty((nq, K), dtype=np.int64)
    for i in range(nq):
        if query_keep is not None and not query_keep[i]:
            out_m[i], out_d[i], out_i[i] = NO_NEIGHBOUR, np.inf, -1
            continue
        qs = -1 if query_scene is None else int(query_scene[i])
        same = [qs >= 0 and idx[i, j] >= 0 and meta[idx[i, j], 0] == qs for j in range(k2)]
        order = ([j for j in range(k2) if not same[j]] + [j for j in range(k2) if same[j]])[:K]
        for w, j in enumerate(order):
            out_m[i, w] = meta[idx[i, j]] if idx[i, j] >= 0 else NO_NEIGHBOUR
            out_d[i, w] = dist[i, j]
            out_i[i, w] = idx[i, j]
    return out_m, out_d, out_i


# ------------------------------------------------------------------------------------------------ gathers

def gather_patches(volumes, meta, chunks, K, trunc_fill, trunc_ratio, mean, std, layout):
    """rf_gather_patches(_f16).  volumes [S, 64, 64, 64] float32 or float16, meta [chunks * 64, K, 7] int32 (scene, x0, x1, y0, y1, z0, z1) in (chunk, slot)
    order; the box is 16^3 from (x0, y0, z0).  scene < 0 or >= S: the truncation fill.  value = ((v * ratio) - mean) / std, every step rounded to float32.
    layout 0: [chunks, K, 64, 64, 64], slot = (x / 16) * 16 + (y / 16) * 4 + z / 16; layout 1: [chunks * K * 64, 1, 16, 16, 16], row (chunk * K + k) * 64 + slot."""
    volumes, meta = np.asarray(volumes), np.asarray(meta, dtype=np.int32).reshape(chunks, 64, K, 7)
    f = np.float32
    out0 = np.empty((chunks, K, 64, 64, 64), dtype=np.float32)
    out1 = np.empty((chunks * K * 64, 1, 16, 16, 16), dtype=np.float32)
    for c in range(chunks):
        for slot in range(64):
            for k in range(K):
                scene, x0, _, y0, _, z0, _ = meta[c, slot, k].tolist()
                if 0 <= scene < volumes.shape[0]:
                    v = volumes[scene, x0:x0 + 16, y0:y0 + 16, z0:z0 + 16].astype(np.float32)
                else:
                    v = np.full((16, 16, 16), trunc_fill, dtype=np.float32)
                assert v.shape == (16, 16, 16), 'box outside the scene'
                v = (((v * f(trunc_ratio)).astype(np.float32) - f(mean)).astype(np.float32) / f(std)).astype(np.float32)
                xx, yy, zz = (slot >> 4) * 16, ((slot >> 2) & 3) * 16, (slot & 3) * 16
                out0[c, k, xx:xx + 16, yy:yy + 16, zz:zz + 16] = v
                out1[(c * K + k) * 64 + slot, 0] = v
    return out1 if layout == 1 else out0


def gather_rows(src, idx):
    """rf_gather_rows: out[m] = src[idx[m]]; idx < 0 or idx >= n selects the LAST row (the database's sentinel patch)"""
    src, idx = np.asarray(src), np.asarray(idx, dtype=np.int64)
    n = src.shape[0]
    return src[np.where((idx < 0) | (idx >= n), n - 1, idx)]


# ------------------------------------------------------------------------------------------------ canvas paste

def paste_chunks(df, sel, dst, sx, sy, flat, round_half=True):
    """rf_paste_chunks: chunks df[sel[i]] ([b, 1, 64, 64, 64] float32) -> float16 and back (torch's CPU rounding) when ``round_half`` -> float64 -> ``flat``
    (a float64 numpy vector, written in place) at element offset dst[i], canvas strides sx, sy, z contiguous"""
    t = torch.as_tensor(np.asarray(df, dtype=np.float32))
    if round_half:
        t = t.half().float()
    vals = t.double().numpy().reshape(-1, 64, 64, 64)
    for c, o in zip(np.asarray(sel).tolist(), np.asarray(dst).tolist()):
        for x in range(64):
            for y in range(64):
                at = o + x * sx + y * sy
                flat[at:at + 64] = vals[c, x, y]
    return flat


# ------------------------------------------------------------------------------------------------ the backend seam of rfuse.database

class NumpySearchBackend:
    """rf_l2_topk_keys / rf_topk_merge_keys / rf_demote_same_scene on CPU tensors: what rfuse.database.PatchDatabase(backend=...) takes"""

    @staticmethod
    def pack(emb_shard):
        return emb_shard

    @staticmethod
    def topk_keys(q, packed, n, row_base, k2):
        return torch.from_numpy(topk_keys(q.numpy(), packed.numpy(), row_base, k2).view(np.int64))

    @staticmethod
    def topk(q, packed, n, row_base, k2):
        d, i = topk(q.numpy(), packed.numpy(), row_base, k2)
        return torch.from_numpy(d), torch.from_numpy(i)

    @staticmethod
    def merge_keys(key_parts):
        d, i = unpack_keys(merge_keys(key_parts.numpy().view(np.uint64)))
        return torch.from_numpy(d), torch.from_numpy(i)

    @staticmethod
    def demote(dist_, idx, meta, query_scene, K, query_keep):
        m, d, i = demote(dist_.numpy(), idx.numpy(), meta.numpy(), None if query_scene is None else query_scene.numpy(), K,
                         None if query_keep is None else query_keep.numpy())
        return torch.from_numpy(m), torch.from_numpy(d), torch.from_numpy(i)
