"""GPU: the device-resident patch dataset (rfuse/data.py, csrc/dataset.hip) against tests/golden/dataset.npz, the record of the reference's own SceneHandler and
PatchedSceneDataset on the toy dataset (tools/gen_dataset_golden.py), and against the numpy restatement of tests/dataset_ref.py that reproduces that record on
the CPU (tests/test_dataset_cpu.py).

Counts are integers; a batch value is one float32 subtract and one correctly rounded float32 divide of an exactly converted stored value on both sides: every
comparison is for equal bits (SHA-256 of the float32 bytes, NaN canonical, and a few whole windows), without a tolerance."""
import numpy as np
import pytest
import torch

import dataset_ref as dr
import testkit

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
STORES = [torch.float16, torch.float32]


@pytest.fixture(scope='module')
def z(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    return dr.load_fixture(golden_dir)


@pytest.fixture(scope='module')
def made(z):
    """(run, store dtype) -> (store, dataset), built once: the occupancy is counted on the device"""
    from rfuse.data import PatchDataset, SceneStore
    cache = {}

    def get(run, dtype=torch.float16):
        if (run, dtype) not in cache:
            d, task, no_retr, split, names, cloud_dtype, table_dtype = dr.RUNS[run]
            store = SceneStore(*dr.store_fields(z, run), device=DEV, dtype=dtype)
            table = None if table_dtype is None else z['table'].astype(table_dtype)
            cache[(run, dtype)] = (store, PatchDataset(store, d, split, scenes=names, task=task, no_retrievals=no_retr, table=table))
        return cache[(run, dtype)]
    return get


def occupancy_of(z, run):
    geo = 'pc' if run.startswith('pc') else run.split('_')[0]
    return dict(zip(z[geo + '_occ_names'].tolist(), (int(v) for v in z[geo + '_occ_counts'])))


def rows_of(z, run):
    return z[run + '_rows'] if len(z[run + '_rows']) else None


def digests(t):
    return np.stack([dr.digest(x) for x in t.cpu().numpy()])


@pytest.mark.parametrize('dtype', STORES)
@pytest.mark.parametrize('run', list(dr.RUNS))
def test_counts_and_kept_items_equal_the_reference(z, made, run, dtype):
    from rfuse.data import patch_names, patch_occupancy
    d, task, no_retr, split, names = dr.RUNS[run][:5]
    store, ds = made(run, dtype)
    counts = patch_occupancy(store, d, names)
    assert counts.dtype == torch.int32 and counts.device == DEV
    occ = occupancy_of(z, run)
    got = dict(zip(patch_names(store, d, names), counts.cpu().tolist()))
    assert got == {k: occ[k] for k in got} and len(got) == sum(k.split('--')[0] in names for k in occ)
    assert ds.names() == z[run + '_names'].tolist()
    assert np.array_equal(ds.extent_target, z[run + '_extent_tgt']) and np.array_equal(ds.extent_input, z[run + '_extent_in'])
    want = np.array([[occ[k] > d['occupancy_threshold'] for k in occ if k.startswith(s + '--')] for s in names[:1]])
    assert np.array_equal(ds.patch_mask(names[:1]), want)                     # the mask derived from the fixture's counts


@pytest.mark.parametrize('dtype', STORES)
@pytest.mark.parametrize('run', list(dr.RUNS))
def test_every_batch_tensor_equals_the_reference(z, made, run, dtype):
    d, task, no_retr, split, names = dr.RUNS[run][:5]
    g = dr.Geometry(d)
    store, ds = made(run, dtype)
    n = len(ds)
    got = ds.batch(np.arange(n), rows_of(z, run))
    assert set(got) == {'input', 'target', 'retrieval', 'extent', 'scene_index'}
    assert got['input'].shape == (n, 1, g.wi, g.wi, g.wi) and got['target'].shape == (n, 1, g.wt, g.wt, g.wt) and got['retrieval'].shape == (n, 4, g.wt, g.wt, g.wt)
    assert all(got[k].dtype == torch.float32 and got[k].device == DEV for k in ('input', 'target', 'retrieval'))
    assert got['extent'].dtype == torch.int32 and np.array_equal(got['extent'].cpu().numpy(), z[run + '_extent_tgt'])
    assert got['scene_index'].dtype == torch.int64 and [names[i] for i in got['scene_index'].cpu().tolist()] == [s.split('--')[0] for s in z[run + '_names'].tolist()]
    for j, k in enumerate(('input', 'target', 'retrieval')):
        bad = np.nonzero((digests(got[k]) != z[run + '_digests'][:, j]).any(axis=1))[0]
        assert len(bad) == 0, '%s %s: items %s differ from the reference' % (run, k, bad.tolist())
    w = min(3, n - 1)
    if task == 'surface_reconstruction':
        one = dr.normalise(np.float32(1), d['input_mean'], d['input_std'])
        assert np.array_equal(np.packbits(got['input'][w].cpu().numpy().reshape(-1) == one), z[run + '_w_input'])
    else:
        assert np.array_equal(got['input'][w].cpu().numpy(), z[run + '_w_input'], equal_nan=True)
    if run != 'full_train':
        assert np.array_equal(got['target'][w].cpu().numpy(), z[run + '_w_target'], equal_nan=True)
        assert np.array_equal(got['retrieval'][w, 1].cpu().numpy(), z[run + '_w_retrieval'], equal_nan=True)
    if no_retr:
        assert bool((got['retrieval'] == float(g.target_trunc)).all())
    # a permuted subset through device indices: the same items
    pick = torch.tensor([n - 1, 0, n // 2], device=DEV)
    rows = rows_of(z, run)
    sub = ds.batch(pick, None if rows is None else torch.from_numpy(rows[[n - 1, 0, n // 2]]).to(DEV))
    for k in got:
        assert torch.equal(sub[k].view(torch.int32) if sub[k].dtype == torch.float32 else sub[k], (got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k])[pick])


def run_all(z, made):
    out = []
    for run in ('df_train', 'pc64_train'):
        ds = made(run)[1]
        got = ds.batch(made.idx[run], made.rows[run])
        out += [got[k].reshape(-1).view(torch.int32) for k in ('input', 'target', 'retrieval')]
    out.append(made.counts())
    return torch.cat(out)


@pytest.fixture(scope='module')
def on_device(z, made):
    made.idx, made.rows = {}, {}
    for run in ('df_train', 'pc64_train'):
        n = len(made(run)[1])
        made.idx[run] = torch.arange(n, device=DEV)
        made.rows[run] = None if rows_of(z, run) is None else torch.from_numpy(rows_of(z, run)).to(DEV)
    store = made('df_val', torch.float32)[0]
    from rfuse import data
    idx, _, e_tgt = data.patch_table(store, dr.DF)
    items = torch.from_numpy(np.ascontiguousarray(np.concatenate([idx[:, None], e_tgt[:, 0::2]], axis=1), dtype=np.int32)).to(DEV)
    g = data.Geometry(dr.DF)
    made.counts = lambda: data.window_counts(store, items, g.window_target, g.context_target, g.target_trunc, g.threshold)
    return made


def test_two_calls_give_the_same_bits(z, on_device):
    first = run_all(z, on_device)
    assert torch.equal(first, run_all(z, on_device))


def test_side_stream_beside_f16_mfma_keeps_the_solo_bits(z, on_device):
    ref = run_all(z, on_device).clone()
    main, side = torch.cuda.current_stream(), torch.cuda.Stream(DEV)
    scratch = torch.empty(256 * 256, device=DEV)
    torch.cuda.synchronize()
    outs = []
    side.wait_stream(main)
    testkit.f16_mfma_load(main, scratch)
    with torch.cuda.stream(side):
        for _ in range(20):
            outs.append(run_all(z, on_device))
    torch.cuda.synchronize()
    assert sum(0 if torch.equal(o, ref) else 1 for o in outs) == 0


def item_keys(batch):
    return [tuple(r) for r in torch.cat([batch['scene_index'][:, None], batch['extent'].to(torch.int64)], dim=1).cpu().tolist()]


@pytest.mark.parametrize('run', ['df_train', 'pc32_train'])
def test_loader_covers_every_item_once_and_drops_only_the_tail(z, made, run):
    from rfuse.data import BatchLoader
    store, ds = made(run)
    names = dr.RUNS[run][4]
    n = len(ds)
    want = sorted((names.index(nm.split('--')[0]),) + tuple(int(v) for v in e) for nm, e in zip(ds.names(), ds.extent_target))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    loader = BatchLoader(ds, 7, shuffle=True, generator=gen)
    assert len(loader) == (n + 6) // 7
    batches = list(loader)
    assert [b['target'].shape[0] for b in batches] == [7] * (n // 7) + ([n % 7] if n % 7 else [])
    first = [k for b in batches for k in item_keys(b)]
    assert sorted(first) == want                                              # every kept item (times the multiplier) exactly once
    second = [k for b in loader for k in item_keys(b)]
    assert sorted(second) == want and second != first                         # another epoch, another order
    gen.manual_seed(11)
    assert [k for b in loader for k in item_keys(b)] == first                 # the generator decides
    # drop_last: the same order, without its tail
    gen.manual_seed(11)
    dropped = list(BatchLoader(ds, 7, shuffle=True, drop_last=True, generator=gen))
    assert len(dropped) == n // 7 and n % 7 and [k for b in dropped for k in item_keys(b)] == first[:n // 7 * 7]
    # without shuffle: the dataset's order, and the batch is the dataset's
    plain = list(BatchLoader(ds, 5, generator=gen))
    assert [k for b in plain for k in item_keys(b)] == [(names.index(nm.split('--')[0]),) + tuple(int(v) for v in e) for nm, e in zip(ds.names(), ds.extent_target)]
    again = ds.batch(np.arange(5, 10), None if not ds.point_clouds else np.zeros(5, np.int64))['target']
    assert torch.equal(plain[1]['target'].view(torch.int32), again.view(torch.int32))          # bits: a target holds a NaN voxel
    if ds.point_clouds:                                                       # the rows are drawn on the device: inputs differ between epochs, targets do not
        a, b = list(BatchLoader(ds, n, generator=gen))[0], list(BatchLoader(ds, n, generator=gen))[0]
        assert torch.equal(a['target'].view(torch.int32), b['target'].view(torch.int32)) and not torch.equal(a['input'], b['input'])


@pytest.mark.parametrize('run', ['df_train', 'pc32_train'])
def test_an_epoch_never_waits_for_the_host(z, made, run):
    from rfuse.data import BatchLoader
    store, ds = made(run)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    loader = BatchLoader(ds, 8, shuffle=True, generator=gen)
    warm = [b['target'].shape[0] for b in loader]                             # first use: the library is loaded, the allocator warm
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        sizes = [b['target'].shape[0] for b in loader]
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert sizes == warm and sum(sizes) == len(ds)


def test_argument_errors_are_raised_before_any_launch(z, made):
    """the launch log of the bound library stays empty while the host checks refuse"""
    from rfuse import _lib, data
    store, ds = made('df_train')
    lib = _lib.load_data()
    records = []
    lib.start_profile(records)
    try:
        with pytest.raises(ValueError, match='leaves the padded scene'):
            data.windows(store, 'target', np.array([[2, 25, 0, 0]]), 32, 8, 0.06, 0.05, 0.01)
        with pytest.raises(ValueError, match='leaves the padded scene'):
            data.window_counts(store, np.array([[0, 0, 0, 17]]), 32, 8, 0.06, 0.03)
        with pytest.raises(ValueError, match='use_subset: target: the window of item 0'):
            ds.use_subset([dr.name_of('c', (32, 64, 0, 32, 0, 32))])
        with pytest.raises(IndexError, match=r'in \[0, %d\)' % len(ds)):
            ds.batch([len(ds)])
        pc_store, pc = made('pc32_train')
        table = z['table'].astype(np.int64)
        with pytest.raises(ValueError, match='table index out of range'):
            data.PatchDataset(pc_store, dr.PC, 'train', scenes=('a', 'b'), task='surface_reconstruction', no_retrievals=True, table=np.where(table == 19999, 20000, table),
                              occupancy={})
        with pytest.raises(IndexError, match=r'table rows in \[0, 16\)'):
            pc.batch([0, 1], [0, 16])
        mismatch = dict(dr.DF, patch_size_input=3, patch_context_input=0, patch_stride=8)
        odd = data.SceneStore(['x'], [np.zeros((32, 32, 32), np.float32)], [np.zeros((6, 6, 6), np.float32)], device=DEV)
        with pytest.raises(ValueError, match='has 27 target patches but its input'):
            data.PatchDataset(odd, mismatch, 'val')
    finally:
        lib.stop_profile()
    assert records == []
    assert ds.names() == z['df_train_names'].tolist()                         # the refused subset left the dataset as it was


@pytest.mark.parametrize('dtype', STORES)
def test_windows_of_any_size_anywhere(z, made, dtype):
    """the scalar store path (a window that is no multiple of 4), windows that start anywhere, unchecked device items that lie partly or wholly outside their padded
    scene (written as the fill), an item of no scene, and a fill that is itself occupied"""
    from rfuse import data
    store = made('df_train', dtype)[0]
    scenes = dr.toy_scenes(z)
    items = np.array([[0, 3, 5, 7], [2, 30, 20, 11], [1, 22, 23, 24], [2, 38, 30, 22], [0, -3, 0, 31], [1, 100, 100, 100], [-1, 0, 0, 0], [3, 0, 0, 0]], dtype=np.int32)
    dev_items = torch.from_numpy(items).to(DEV)
    fill, mean, std = 0.0625, 0.059954833543534335, 0.010110036361741626
    for w, pad in ((5, 2), (9, 0), (12, 3)):
        for field, key in (('target', 'target'), ('retrieval', 'retrieval')):
            want = []
            for sc, x, y, zz in items:
                if not 0 <= sc < 3:
                    vol = np.full((1 if field == 'target' else 4,) + (w,) * 3, np.float32(fill))
                else:
                    src = scenes['abc'[sc]][key]
                    big = np.pad(src.astype(np.float32), [(0, 0)] * (src.ndim - 3) + [(pad + 128, pad + 128)] * 3, constant_values=np.float32(fill))
                    vol = big[..., x + 128:x + 128 + w, y + 128:y + 128 + w, zz + 128:zz + 128 + w].reshape((-1,) + (w,) * 3)
                want.append(vol)
            want = np.stack(want)
            got = data.windows(store, field, dev_items, w, pad, fill, mean, std).cpu().numpy()
            assert np.array_equal(got, dr.normalise(want, mean, std), equal_nan=True), (w, pad, field)
            raw = data.windows(store, field, dev_items, w, pad, fill).cpu().numpy()
            assert np.array_equal(raw, want, equal_nan=True), (w, pad, field)
    # counts: a fill below the threshold is occupied like any voxel; NaN never is
    for w, pad, fill, thr in ((5, 2, 0.01, 0.03125), (12, 3, 0.0625, 0.03125), (32, 8, 0.03125, 0.03125), (9, 0, float('nan'), 0.05)):
        want = []
        for sc, x, y, zz in items:
            if not 0 <= sc < 3:
                want.append(0)
                continue
            big = np.pad(scenes['abc'[sc]]['target'].astype(np.float32), pad + 128, constant_values=np.float32(fill))
            want.append(int((big[x + 128:x + 128 + w, y + 128:y + 128 + w, zz + 128:zz + 128 + w] <= np.float32(thr)).sum()))
        got = data.window_counts(store, dev_items, w, pad, fill, thr).cpu().tolist()
        assert got == want, (w, pad, fill, thr)


@pytest.mark.parametrize('cloud_dtype,table_dtype', [('float32', np.int32), ('float64', np.uint16)])
def test_points_with_nan_inf_and_a_short_cloud(gpu, cloud_dtype, table_dtype):
    """NaN coordinates are skipped, +-inf clip, a cloud below 20000 rows is read stacked twice, an int32 table; a scale that is no power of two"""
    from rfuse import data
    rng = np.random.default_rng(5)
    clouds = [rng.uniform(-2, 14, (20000, 3)), rng.uniform(-2, 14, (700, 3))]
    for c in clouds:
        c[rng.integers(0, len(c), 60), rng.integers(0, 3, 60)] = np.nan
        c[rng.integers(0, len(c), 40), rng.integers(0, 3, 40)] = np.inf
        c[rng.integers(0, len(c), 40), rng.integers(0, 3, 40)] = -np.inf
    clouds = [c.astype(cloud_dtype) for c in clouds]
    table = rng.integers(0, 1400, (6, 300)).astype(table_dtype)
    store = data.SceneStore(['p', 'q'], [np.zeros((4, 4, 4), np.float32)] * 2, clouds=clouds, device=DEV)
    tab = torch.from_numpy(data.check_table(table, [20000, 700])).to(DEV)
    items = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 5, 9, 2], [0, 17, 17, 17], [1, 17, 0, 8]], dtype=np.int32)
    rows = np.array([0, 5, 2, 3, 1], dtype=np.int32)
    scale, grid, pad, w = 1.75, 24, 3, 13
    got = data.point_windows(store, tab, items, torch.from_numpy(rows).to(DEV), w, grid, pad, scale, 0.25, 0.7).cpu().numpy()
    want = np.stack([dr.normalise(dr.point_window(clouds[sc], table[r], grid, scale, pad, (x, y, zz), w), 0.25, 0.7)[None] for (sc, x, y, zz), r in zip(items, rows)])
    assert np.array_equal(got, want) and (want == want.max()).sum() > 20
    raw = data.point_windows(store, tab, items, torch.from_numpy(rows).to(DEV), w, grid, pad, scale).cpu().numpy()
    assert set(np.unique(raw).tolist()) == {0.0, 1.0} and np.array_equal(raw == 1, want == want.max())
    with pytest.raises(ValueError, match='leaves the padded scene'):
        data.point_windows(store, tab, np.array([[0, 18, 0, 0]], dtype=np.int32), torch.zeros(1, dtype=torch.int32, device=DEV), w, grid, pad, scale)
    if cloud_dtype == 'float64':
        with pytest.raises(ValueError, match='is not a float32 value'):
            data.point_windows(store, tab, items, torch.from_numpy(rows).to(DEV), w, grid, pad, 1 / 3)
