"""Fixture generator for the patch dataset (CPU; needs the reference checkout, as tools/gen_iou_matrix_golden.py does): writes the toy dataset of
tests/dataset_ref.py to a temporary directory in the reference's on-disk layout, runs the reference's own ``SceneHandler`` (dataset/scene.py) and
``PatchedSceneDataset`` (dataset/patched_scene_dataset.py) on it as written, and saves tests/golden/dataset.npz (arrays only).

    python tools/gen_dataset_golden.py

The toy dataset (tests/dataset_ref.py has the constants), each part aimed at one way to go wrong:
    a   32^3   a spherical shell: voxels exactly on the occupancy threshold (code 33), one NaN voxel
    b   32^3   empty but for a blob that one window sees and two voxels in a corner: windows of count 0 and of count 2 = occupancy_threshold, all dropped
    c   (40, 32, 24)   two planes: starts (0, 24) that the stride does not divide, one axis with a single patch, inputs of (5, 4, 3)
    d   64^3   a tiled 2 x 2 x 2: the whole-grid 128^3 point-cloud item of the refinement configs
    clouds     20000 rows (a, d) and 12000 rows (b: read stacked twice), coordinates below 0 and above the grid, +-inf, duplicates, coordinates on voxel
               boundaries; as float32 and as float64 (2^-40 below: the boundary points fall into the voxel below)
    table      16 rows of 100 indices below 20000, as uint16 and as int64
Every window of the distance-field runs touches the padding on some face (scenes of two patches per axis).

Runs (tests/dataset_ref.py RUNS): df_train / df_val (distance-field inputs, composed retrievals with K = 4, float16 preloaded and float32 from disk: the
same values, asserted), pc32_train / pc64_train (point clouds, ``no_retrievals``), full_train.  For the point-cloud runs ``random.seed(RANDOM_SEED)`` fixes the
``random.randint`` draw of every item, read in order; the draws are recorded.

Layout: ``target_<s>`` / ``input_<s>`` / ``retr_<s>`` uint8 codes, ``cloud_codes`` int16 [20000, 3], ``table`` uint16 [16, 100]; per geometry
``<df|pc|full>_occ_names`` / ``_occ_counts`` = the reference's occupancy JSON in its order; per run ``<run>_names``, ``_extent_in`` / ``_extent_tgt`` int32
[N, 6], ``_rows`` int32 [N] (the table row of each item; empty without clouds), ``_digests`` uint8 [N, 3, 32] = SHA-256 of input, target, retrieval (float32
bytes, NaN canonical: dataset_ref.digest), and ``_w_input`` / ``_w_target`` / ``_w_retrieval`` = the whole windows of item WHOLE_ITEM (the input of a
point-cloud run as packed bits of ``input == (1 - mean) / std``).
"""
import json
import random
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
from oracle.gen_golden import REF, save_fixture, import_reference_util_retrieval      # noqa: E402
import dataset_ref as dr                                                               # noqa: E402

LIMIT = 1 << 20
WHOLE_ITEM = 3
K = 4


def import_reference():
    import_reference_util_retrieval()
    for n in ('tqdm', 'util.visualization'):
        if n not in sys.modules:
            try:
                __import__(n)
            except Exception:
                sys.modules[n] = types.ModuleType(n)
    if not hasattr(sys.modules['tqdm'], 'tqdm') or isinstance(sys.modules['tqdm'].tqdm, types.ModuleType):
        sys.modules['tqdm'].tqdm = lambda x, *a, **kw: x
    for attr in ('visualize_pointcloud', 'visualize_sdf_as_mesh', 'visualize_sdf_as_voxels', 'visualize_grid_as_voxels', 'visualize_float_grid', 'visualize_normals'):
        if not hasattr(sys.modules['util.visualization'], attr):
            setattr(sys.modules['util.visualization'], attr, None)
    from dataset.scene import SceneHandler
    from dataset.patched_scene_dataset import PatchedSceneDataset
    import dataset.scene as scene_mod
    assert str(REF) in scene_mod.__file__, scene_mod.__file__
    return SceneHandler, PatchedSceneDataset


# ------------------------------------------------------------------------------------------------ the toy dataset
def shell_codes(shape, centre, radius):
    ax = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    dist = np.sqrt(sum((a - c) ** 2 for a, c in zip(ax, centre)))
    return np.minimum(np.round(np.abs(dist - radius) * 22), 66).astype(np.uint8)           # 22 codes = one voxel of 11 / 512


def toy_codes(rng):
    out = {}
    a = shell_codes((32, 32, 32), (15.3, 16.1, 14.8), 11.4)
    a[5, 6, 7] = dr.NAN_CODE
    a[0, 0, 0:3] = 33                                                                      # on the threshold, on a face of the scene
    b = np.full((32, 32, 32), 66, np.uint8)
    b[26:31, 26:31, 26:31] = np.minimum(shell_codes((5, 5, 5), (2, 2, 2), 1.2), 66)
    b[2, 2, 2:4] = 10
    xs = np.arange(40)[:, None, None]
    zs = np.arange(24)[None, None, :]
    c = np.minimum(np.minimum(np.round(np.abs(xs - 20.3) * 22), np.round(np.abs(zs - 6.6) * 22)) + np.zeros((40, 32, 24)), 66).astype(np.uint8)
    c[:, 20:, :] = 66
    for s, t in zip(dr.SCENES, (a, b, c)):
        out['target_' + s] = t
        small = tuple(int(v / 8) for v in t.shape)
        blocks = np.where(t == dr.NAN_CODE, 66, t)[:small[0] * 8, :small[1] * 8, :small[2] * 8].reshape(small[0], 8, small[1], 8, small[2], 8)
        out['input_' + s] = np.round(blocks.mean(axis=(1, 3, 5)) * 2.5 + rng.integers(0, 3, small)).astype(np.uint8)
        retr = np.stack([np.roll(t, k + 1, axis=k % 3) for k in range(K)])
        retr[retr == dr.NAN_CODE] = 40
        retr[1] = np.minimum(retr[1] + 5, 66)
        out['retr_' + s] = retr
    out['input_a'][1, 2, 3] = dr.NAN_CODE
    # points near a sphere of radius 10 around (16, 16, 16), in units of 1 / 64; some far outside [0, 32]
    n = 20000
    d = rng.normal(size=(n, 3))
    p = 16 + d / np.linalg.norm(d, axis=1, keepdims=True) * (10 + rng.normal(size=(n, 1)) * 0.3)
    p[:400] = rng.uniform(-4, 36, (400, 3))
    codes = np.round(p * 64).astype(np.int16)
    codes[400:800] = codes[400:800] // 32 * 32                                             # on voxel boundaries at scale 2
    codes[100:200] = codes[0:100]                                                          # duplicates
    codes[12100:12200] = codes[0:100]
    codes[7, 0], codes[8, 1], codes[13000, 2] = dr.CLOUD_POS_INF, dr.CLOUD_NEG_INF, dr.CLOUD_POS_INF
    out['cloud_codes'] = codes
    table = rng.integers(0, n, (16, 100)).astype(np.uint16)
    table[0, :10] = [7, 8, 7, 13000, 19999, 0, 12000, 11999, 100, 0]
    table[3, 50:] = table[3, :50]
    out['table'] = table
    return out


# ------------------------------------------------------------------------------------------------ the reference's files
def write_dataset(root, z, run, preload):
    d, task, no_retr, split, names, cloud_dtype, table_dtype = dr.RUNS[run]
    scenes = dr.toy_scenes(z, cloud_dtype)
    pc = task == 'surface_reconstruction'
    ds = dict(d, data_dir=str(root), scene_dir=str(root), retrieval_dir=str(root), splits_dir='main', input_dir='input', target_dir='target', input_ext='.npz',
              target_ext='.npz', preload_scenes=preload, preload_retrievals=preload, skip_occupancy=False)
    (root / 'splits' / 'Toy' / 'main').mkdir(parents=True)
    (root / 'splits' / 'Toy' / 'main' / (split + '.txt')).write_text('\n'.join(names) + '\n')
    for sub in ('input', 'target'):
        (root / sub / 'Toy').mkdir(parents=True)
    config = {'task': task, 'fast_visualization': True, 'no_retrievals': no_retr, 'retrieval_ckpt': 'runs/toy_experiment/epoch07.ckpt', 'K': K,
              'dataset_train': ds, 'dataset_val': ds}
    compose = root / 'retrieval' / ('%s_%04d' % (task, d['num_points'])) / 'Toy' / 'main' / 'toy_experiment' / 'epoch07' / str(K) / 'compose'
    compose.mkdir(parents=True)
    for s in names:
        np.savez_compressed(root / 'target' / 'Toy' / (s + '.npz'), arr=scenes[s]['target'])
        if pc:
            np.savez_compressed(root / 'input' / 'Toy' / (s + '.npz'), scenes[s]['cloud'])
        else:
            np.savez_compressed(root / 'input' / 'Toy' / (s + '.npz'), arr=scenes[s]['input'])
        if not no_retr:
            np.savez_compressed(compose / (s + '.npz'), scenes[s]['retrieval'])
    (root / 'random_indices').mkdir()
    table = z['table'].astype(table_dtype) if pc else np.zeros((1, 0), np.int64)
    np.savez_compressed(root / 'random_indices' / ('%d.npz' % d['num_points']), arr=table)
    return config, ds, table


def run_reference(SceneHandler, PatchedSceneDataset, z, run, preload):
    d, task, no_retr, split, names, cloud_dtype, table_dtype = dr.RUNS[run]
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        config, ds, table = write_dataset(root, z, run, preload)
        handler = SceneHandler(split, config)
        dataset = PatchedSceneDataset(split, ds, handler)
        assert dataset.scenes == list(names)
        occ = json.loads((root / 'occupancy' / ('Toy_%03d_%02d_%02d.json' % (d['target_chunk_size'], d['patch_size_target'], d['patch_context_target']))).read_text())
        n = len(dataset)
        random.seed(dr.RANDOM_SEED)
        rows = [random.randint(0, table.shape[0] - 1) for _ in range(n)] if task == 'surface_reconstruction' else []
        random.seed(dr.RANDOM_SEED)
        items = [dataset[i] for i in range(n)]
        lookup = {k: list(v) for k, v in dataset.patch_from_scene_lookup.items()}
        extent_in = np.array([np.asarray(it[1]) for it in dataset.data], dtype=np.int32).reshape(n, 6)
    return items, rows, occ, extent_in, lookup


def check_and_record(out, z, run, items, rows, occ, extent_in, lookup):
    d, task, no_retr, split, names, cloud_dtype, table_dtype = dr.RUNS[run]
    g = dr.Geometry(d)
    ctx = d['patch_context_target']
    fill = dr.normalise(g.target_trunc, d['target_mean'], d['target_std'])
    n = len(items)
    digests = np.zeros((n, 3, 32), np.uint8)
    retrievals = []
    for i, it in enumerate(items):
        assert it['input'].dtype == np.float32 and it['target'].dtype == np.float32 and it['retrieval'].dtype == np.float32, run
        assert it['input'].shape == (1, g.wi, g.wi, g.wi) and it['target'].shape == (1, g.wt, g.wt, g.wt), (run, it['input'].shape, it['target'].shape)
        r = it['retrieval']
        if not no_retr:
            # np.pad(arr, context) pads the K axis too (scene.py:74,99): the K real channels are channels context .. context + K
            assert r.shape == (K + 2 * ctx, g.wt, g.wt, g.wt), r.shape
            assert (r[:ctx] == fill).all() and (r[ctx + K:] == fill).all()
            r = r[ctx:ctx + K]
        assert r.shape == (4, g.wt, g.wt, g.wt)
        retrievals.append(r)
        digests[i] = [dr.digest(it['input']), dr.digest(it['target']), dr.digest(r)]
    # the restatement gives the same items, bit for bit, from either store precision
    for store in (np.float16, np.float32):
        ref = dr.run_dataset(z, run, store)
        assert len(ref) == n, (run, len(ref), n)
        assert {k: v for k, v in ref.occupancy.items()} == {k: occ[k] for k in ref.occupancy}, run
        for i, it in enumerate(items):
            mine = ref.item(i, rows[i] if rows else None)
            assert mine['name'] == it['name'] and mine['scene'] == it['scene'] and np.array_equal(mine['extent'], it['extent']), (run, i)
            assert np.array_equal(ref.data[i][1], extent_in[i])
            for k, theirs in (('input', it['input']), ('target', it['target']), ('retrieval', retrievals[i])):
                assert mine[k].dtype == np.float32 and np.array_equal(mine[k], theirs, equal_nan=True), (run, i, k)
    assert lookup == {s: [dr.name_of(s, e) for (q, _, e) in ref.data[:n // (d['train_multiplier'] if split == 'train' else 1)] if q == s] for s in lookup}
    out[run + '_names'] = np.array([it['name'] for it in items])
    out[run + '_extent_in'] = extent_in
    out[run + '_extent_tgt'] = np.array([np.asarray(it['extent']) for it in items], dtype=np.int32).reshape(n, 6)
    out[run + '_rows'] = np.array(rows, dtype=np.int32)
    out[run + '_digests'] = digests
    w = items[min(WHOLE_ITEM, n - 1)]
    if task == 'surface_reconstruction':
        one = dr.normalise(np.float32(1), d['input_mean'], d['input_std'])
        zero = dr.normalise(np.float32(0), d['input_mean'], d['input_std'])
        assert ((w['input'] == one) | (w['input'] == zero)).all() and (w['input'] == one).any()
        out[run + '_w_input'] = np.packbits(w['input'].reshape(-1) == one)
    else:
        out[run + '_w_input'] = w['input']
    if run != 'full_train':
        out[run + '_w_target'] = w['target']
        out[run + '_w_retrieval'] = retrievals[min(WHOLE_ITEM, n - 1)][1]
    return occ


def main():
    SceneHandler, PatchedSceneDataset = import_reference()
    out = toy_codes(np.random.default_rng(2028))
    assert (out['target_a'] == 33).sum() > 20 and (out['target_a'] == dr.NAN_CODE).sum() == 1
    occ_tables = {}
    for run, spec in dr.RUNS.items():
        results = [run_reference(SceneHandler, PatchedSceneDataset, out, run, preload) for preload in (True, False)]
        (items, rows, occ, extent_in, lookup), (items32, rows32, occ32, _, _) = results
        assert rows == rows32 and occ == occ32
        for a, b in zip(items, items32):                                       # float16 preloaded and float32 from disk: the toy values are exact in both
            assert a['name'] == b['name'] and all(np.array_equal(a[k], b[k], equal_nan=True) for k in ('input', 'target', 'retrieval')), run
        check_and_record(out, out, run, items, rows, occ, extent_in, lookup)
        geo = 'pc' if run.startswith('pc') else run.split('_')[0]
        known = occ_tables.setdefault(geo, occ)                                # the first run of a geometry has all of its scenes
        assert all(known[k] == v for k, v in occ.items()), run
        kept = len(items) // (spec[0]['train_multiplier'] if spec[3] == 'train' else 1)
        print('%-11s %3d items (%d kept of %d patches), windows %d^3 / %d^3' % (run, len(items), kept, len(occ), dr.Geometry(spec[0]).wi, dr.Geometry(spec[0]).wt))
    for geo, occ in occ_tables.items():
        out[geo + '_occ_names'] = np.array(list(occ))
        out[geo + '_occ_counts'] = np.array(list(occ.values()), dtype=np.int32)
        print('%-5s occupancy: %d patches, counts %s' % (geo, len(occ), sorted(set(occ.values()))[:8]))
    df = dict(zip(out['df_occ_names'].tolist(), out['df_occ_counts'].tolist()))
    assert 0 in df.values() and dr.DF['occupancy_threshold'] in df.values(), 'the filter needs windows of count 0 and on the threshold'
    save_fixture('dataset', **out)
    size = (REPO / 'tests' / 'golden' / 'dataset.npz').stat().st_size
    print('tests/golden/dataset.npz: %d bytes' % size)
    assert size <= LIMIT


if __name__ == '__main__':
    main()
