"""tests/search_ref.py -- the numpy statement of the retrieval back end's contracts that tests/test_search_gpu.py holds the HIP kernels to -- pinned, without a
GPU, against what the project already trusts: oracle/refpath.py (knn_exact, demote_same_scene, compose_retrieval) and the retrieval_map_compose fixture made
by the reference itself.  Also asserts the two properties of the test data the GPU tests rely on: the dyadic-grid family is exact in float32 in the kernels'
summation order and full of ties at the cut, and the Gaussian family (for the seeds used) has no near-tie among a query's first k2 + 1 neighbours."""
import numpy as np
import pytest
import torch

import helpers
import search_ref as sr
from oracle import refpath
from rfuse import configs as rf_configs
from rfuse import synthetic


@pytest.mark.parametrize('n,nq', sr.SHAPES)
def test_grid_family_is_exact_and_tied_at_the_cut(n, nq):
    emb, q = sr.grid_family(sr.grid_seed(n, nq), n, nq)
    d = sr.dist_f32(q, emb)
    d64 = ((q[:, None, :].astype(np.float64) - emb[None].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(d.astype(np.float64), d64), 'float32 holds the float64 distance exactly'
    assert np.array_equal(sr.chain_dist_f32(q, emb), d), 'the kernels\' four float32 chains round nowhere'
    assert np.array_equal(sr.grid_dist_f32(q, emb), d)
    idx_ref, dist_ref = refpath.knn_exact(q, emb, 16)
    dk, ik = sr.topk(q, emb, 0, 16)
    assert np.array_equal(ik, idx_ref) and np.array_equal(dk.astype(np.float64), dist_ref)


def test_grid_family_ties_at_the_cut_for_every_k2():
    """what makes the grid family a test of tie-breaking: for every k2 some queries (5 % of them at k2 = 1, 38 % at k2 = 16) have the k2-th and the
    (k2 + 1)-th distance equal, so the cut falls inside a run of equal distances and only the row ids decide"""
    tied, total = np.zeros(17), 0
    for n, nq in sr.SHAPES:
        emb, q = sr.grid_family(sr.grid_seed(n, nq), n, nq)
        srt = np.sort(sr.dist_f32(q, emb), axis=1)
        for k2 in range(1, 17):
            tied[k2] += (srt[:, k2 - 1] == srt[:, k2]).sum()
        total += nq
    assert (tied[1:] > 0).all(), tied[1:] / total


@pytest.mark.parametrize('n,nq', sr.SHAPES)
def test_gauss_family_has_no_near_tie(n, nq):
    """from the float64 oracle alone: among a query's first k2 + 1 = 16 distances no two are closer than 1e-5, the planted duplicate rows (4, 9) apart --
    so the kernels' float32 distances (error ~1e-7 at these magnitudes) cannot reorder them, and the GPU test demands exact indices"""
    emb, q = sr.gauss_family(sr.gauss_seed(n, nq), n, nq)
    idx, dist = refpath.knn_exact(q, emb, 16)
    gap = np.diff(dist, axis=1)
    planted = np.isin(idx[:, :-1], (4, 9)) & np.isin(idx[:, 1:], (4, 9))
    assert (emb[4] == emb[9]).all() and planted.any()
    assert (gap[planted] == 0).all()
    assert gap[~planted].min() >= 1e-5, gap[~planted].min()
    dk, ik = sr.topk(q, emb, 0, 15)
    assert np.array_equal(ik, idx[:, :15]), 'stable float64 argsort and the float32 key sort agree'
    assert np.array_equal(dk, dist[:, :15].astype(np.float32))


def test_keys_order_and_sentinels():
    d = np.array([[0.5, np.inf, np.nan, 0.0, -np.nan, 0.5]], dtype=np.float32)
    d[0, 4] = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]      # a NaN with sign and payload
    keys = sr.topk_keys_from_dist(d, 10, 8)
    dist, idx = sr.unpack_keys(keys)
    assert idx[0].tolist() == [13, 10, 15, 11, 12, 14, -1, -1], 'ties by row id; +inf after finite; NaN after +inf, by row id whatever its sign'
    assert np.isnan(dist[0, 4:6]).all() and np.isinf(dist[0, [3, 6, 7]]).all()
    assert (keys[0, 6:] == sr.NONE).all()
    big = sr.topk_keys_from_dist(np.zeros((1, 3), np.float32), 0xFFFFFFFE - 3, 2)
    assert sr.unpack_keys(big)[1][0].tolist() == [0xFFFFFFFE - 3, 0xFFFFFFFE - 2], 'ids above 2^31 come back positive'


def test_merge_of_shards_equals_single_scan_and_keeps_repeats():
    emb, q = sr.grid_family(3, 50, 7)
    whole = sr.topk_keys(q, emb, 0, 8)
    parts = np.stack([sr.topk_keys(q, emb[lo:hi], lo, 8) for lo, hi in ((0, 3), (3, 3), (3, 30), (30, 50))])      # a short and an empty shard
    assert np.array_equal(sr.merge_keys(parts), whole)
    d, i = sr.unpack_keys(parts)
    md, mi = sr.merge_pairs(d, i)
    assert np.array_equal(mi, sr.unpack_keys(whole)[1]) and np.array_equal(md, sr.unpack_keys(whole)[0])
    twice = sr.merge_keys(np.stack([whole, whole]))
    assert np.array_equal(twice[:, 0::2], whole[:, :4]) and np.array_equal(twice[:, 1::2], whole[:, :4]), 'both copies of a repeated key come out'


def _fixture_problem():
    fix = helpers.load_fixture('retrieval_map_compose')
    cfg = rf_configs.get_config('C1')
    db = synthetic.make_database(int(fix['seed']), cfg, int(fix['n_patches']))
    return fix, cfg, db


def test_search_and_demotion_match_oracle_and_reference_fixture():
    fix, cfg, db = _fixture_problem()
    K, q_scene = cfg['K'], int(fix['q_scene'])
    idx_ref, dist_ref = refpath.knn_exact(fix['queries'], db['emb'], 2 * K)
    dist, idx = sr.topk(fix['queries'], db['emb'], 0, 2 * K)
    assert np.array_equal(idx, idx_ref) and np.array_equal(dist, dist_ref.astype(np.float32))
    rows = refpath.mapping_rows(idx_ref, dist_ref, db['meta'])
    for scene, name in ((np.full(64, q_scene), 'map_train'), (np.full(64, -1), 'map_val'), (None, 'map_val')):
        ref = refpath.demote_same_scene(rows, np.full(64, -1) if scene is None else scene, K)
        m, d, i = sr.demote(dist, idx, db['meta'], scene, K)
        assert np.array_equal(m, ref[..., :7].astype(np.int32)) and np.array_equal(d, ref[..., 7])
        assert np.array_equal(m, fix[name][..., :7].astype(np.int32)), 'the reference\'s own mapping'
        assert np.array_equal(db['meta'][i], m)
        for r in range(64):                                       # the index output names the entries the distances belong to
            assert np.array_equal(d[r], np.array([dist[r, idx[r].tolist().index(v)] for v in i[r]], dtype=np.float32))


def test_demotion_rules_missing_and_dropped():
    meta = np.concatenate([np.repeat(np.arange(4), 5)[:, None], np.tile([0, 16, 16, 32, 32, 48], (20, 1))], 1).astype(np.int32)
    idx = np.array([[0, -1, 5, 1, -1, 6], [0, 1, 2, 3, 4, 0], [5, 6, 7, 8, 9, 5]], dtype=np.int64)
    dist = np.arange(18, dtype=np.float32).reshape(3, 6)
    m, d, i = sr.demote(dist, idx, meta, np.array([0, 0, 0]), 4)
    assert i[0].tolist() == [-1, 5, -1, 6], 'a missing neighbour keeps its place among the others; the own-scene rows 0, 1 go behind'
    assert np.array_equal(m[0, 0], sr.NO_NEIGHBOUR) and d[0].tolist() == [1, 2, 4, 5]
    assert i[1].tolist() == [0, 1, 2, 3] and i[2].tolist() == [5, 6, 7, 8], 'all own scene: the order stays'
    m, d, i = sr.demote(dist, idx, meta, np.array([0, 0, 0]), 2, np.array([True, False, True]))
    assert (i[1] == -1).all() and np.isinf(d[1]).all() and (m[1] == sr.NO_NEIGHBOUR).all() and i[0].tolist() == [-1, 5]
    # rows without missing neighbours: the oracle's demotion
    rng = np.random.default_rng(0)
    idx = np.stack([rng.permutation(20)[:8] for _ in range(40)]).astype(np.int64)
    dist = np.sort(rng.random((40, 8)).astype(np.float32), axis=1)
    qs = rng.integers(-1, 4, size=40)
    for K in (1, 3, 4, 8):
        ref = refpath.demote_same_scene(refpath.mapping_rows(idx, dist, meta), qs, K)
        m, d, i = sr.demote(dist, idx, meta, qs, K)
        assert np.array_equal(m, ref[..., :7].astype(np.int32)) and np.array_equal(d, ref[..., 7])


def test_gather_patches_matches_oracle_compose_and_reference_fixture():
    fix, cfg, db = _fixture_problem()
    _, trunc_t = rf_configs.truncations(cfg)
    K = cfg['K']
    mapping = fix['map_val_sentinel']
    meta = mapping[..., :7].astype(np.int32)
    assert (meta[..., 0] < 0).any()
    raw = sr.gather_patches(db['volumes'], meta, 1, K, trunc_t, 1.0, 0.0, 1.0, layout=0)
    assert helpers.sha(raw[0]) == str(fix['compose_val_sha']), 'the reference\'s own composed volume (mean 0, std 1 change no bit)'
    dd = cfg['dataset_train']
    for ratio in (1.0, 0.75, 1.0 / 3.0):
        ref = refpath.compose_retrieval(mapping, db['volumes'], K, trunc_t, trunc_ratio=ratio)
        ref = ((ref - np.float32(dd['target_mean'])) / np.float32(dd['target_std'])).astype(np.float32)
        got = sr.gather_patches(db['volumes'], meta, 1, K, trunc_t, ratio, dd['target_mean'], dd['target_std'], layout=0)
        assert np.array_equal(got[0], ref), ratio
        rows = sr.gather_patches(db['volumes'], meta, 1, K, trunc_t, ratio, dd['target_mean'], dd['target_std'], layout=1)
        assert torch.equal(torch.from_numpy(rows), refpath.unfold3d(torch.from_numpy(got).reshape(K, 1, 64, 64, 64), 16))
    half = sr.gather_patches(db['volumes'].astype(np.float16), meta, 1, K, trunc_t, 1.0, 0.0, 1.0, layout=0)
    assert np.array_equal(half, sr.gather_patches(db['volumes'].astype(np.float16).astype(np.float32), meta, 1, K, trunc_t, 1.0, 0.0, 1.0, layout=0))
    out_of_range = meta.copy()
    out_of_range[3, 0, 0] = db['volumes'].shape[0]
    g = sr.gather_patches(db['volumes'], out_of_range, 1, K, trunc_t, 1.0, 0.0, 1.0, layout=1)
    assert (g[3] == np.float32(trunc_t)).all()


def test_gather_rows_and_paste():
    src = np.arange(24, dtype=np.float32).reshape(6, 4)
    assert np.array_equal(sr.gather_rows(src, [2, -1, 6, 11, 0]), src[[2, 5, 5, 5, 0]])
    rng = np.random.default_rng(1)
    df = rng.standard_normal((3, 1, 64, 64, 64)).astype(np.float32) * 300
    df[0, 0, 0, 0, :4] = [1.00048828125, 70000.0, np.nan, 3e-8]     # a float16 tie (-> 1.0), overflow, NaN, a value that becomes the smallest half subnormal
    canvas = np.full((70, 66, 68), -7.0)
    sy, sx = 68, 66 * 68
    sr.paste_chunks(df, [2, 0], [2, (4 * 66 + 2) * 68 + 4], sx, sy, canvas.reshape(-1), True)
    want = torch.from_numpy(df).half().double().numpy()
    assert np.array_equal(canvas[4:68, 2:66, 4:68], want[0, 0], equal_nan=True)
    assert canvas[4, 2, 4] == 1.0 and np.isinf(canvas[4, 2, 5]) and np.isnan(canvas[4, 2, 6]) and canvas[4, 2, 7] == 2.0 ** -24
    assert (canvas[:, :, :2] == -7.0).all() and np.array_equal(canvas[:4, :64, 2:66], want[2, 0, :4]) and (canvas[68:] == -7.0).all(), 'outside the later paste the first one / the guard remains'
    plain = np.zeros(64 * 64 * 64)
    sr.paste_chunks(df, [1], [0], 4096, 64, plain, False)
    assert np.array_equal(plain, df[1].astype(np.float64).reshape(-1))
