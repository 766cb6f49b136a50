"""CPU: the generated cases of tests/loss_cases.py, before tests/test_loss_sweep_gpu.py runs the kernels on them -- the helper reproduces the inputs of the
reference-generated shape-loss fixture bit for bit, every case reaches the tiling path it is named for (counted from its shape with the kernels' constants
restated in loss_cases.py), and the conditions hold under which a comparison cannot hide a failure: the float32 and float64 restatements agree on every
mask entry (so no voxel has to be left out), enough voxels are valid, the dot-product case has large logits without a saturated loss, and the trainer's
geometry skips a slice for the cap and takes a later one."""
import numpy as np
import pytest

import contrastive_ref as cr
import loss_cases as lc
import shape_loss_ref as slr
from rfuse import configs as rf_configs


def test_helper_reproduces_the_fixture_inputs(golden_dir):
    """make_inputs is the recipe that made tests/golden/shape_loss.npz: target and pred of sn16, odd, mp16 and tiny (and of the two flat cases), bit for bit"""
    cases = slr.load_fixture(golden_dir)
    for name, stats, flat in (('sn16', 'C1', False), ('odd', 'C1', False), ('mp16', 'C4', False), ('tiny', 'C1', False), ('flat4', 'C1', True), ('flat1', 'C1', True)):
        c = cases[name]
        trunc, mean, std = lc.STATS[stats]
        assert (trunc, mean, std) == tuple(float(x) for x in c['params'][:3]), name
        assert (lc.W_OCC, lc.LAM_REC, lc.LAM_N) == tuple(float(x) for x in c['params'][3:]), name
        target, pred = lc.make_inputs(c['target'].shape, trunc, mean, std, lc.SHAPE_SEED, flat)
        assert target.dtype == pred.dtype == np.float32
        assert target.tobytes() == c['target'].tobytes() and pred.tobytes() == c['pred'].tobytes(), name


def test_stats_are_the_configs_rounded():
    """trunc is the config's own; the mean within 5 % of the dataset's and short in bits, the std the power of two below the dataset's"""
    for name, (trunc, mean, std) in lc.STATS.items():
        cfg = rf_configs.get_config(name)
        d = cfg['dataset_train']
        assert trunc == rf_configs.truncations(cfg)[1]
        assert abs(mean - d['target_mean']) < 0.05 * d['target_mean'] and 0.5 < std / d['target_std'] <= 1.0
        assert float(np.log2(std)).is_integer() and mean * 256 == int(mean * 256)
    assert lc.STATS['C1'][0] == 0.0625 and lc.STATS['C4'][0] == 11.25 and not float(np.log2(11.25)).is_integer()


# ------------------------------------------------------------------------------------------------ what the shapes reach
def test_contrastive_cases_reach_the_paths_they_are_named_for():
    assert (lc.NTX_TI, lc.NTX_TJ, lc.NTX_KC, lc.NTX_MAX_CHUNKS) == (16, 64, 64, 4)
    geo = {name: lc.ntx_geometry(n, dim) for name, (n, dim, *_) in lc.SINGLE.items()}
    assert list(geo) == ['w65', 'w96', 'w128', 'w129dot', 'w200iou', 'w256', 'w256n1', 'w100zero', 'g1024']
    g = geo['w65']        # 2 chunks, the second with one feature; 18 rows: the second row tile has 2
    assert (g['chunks'], g['last_chunk'], g['row_tiles'], g['rows_in_last_tile']) == (2, 1, 2, 2) and lc.SINGLE['w65'][0] * 2 == 18
    g = geo['w96']        # a second chunk of 32; 66 columns: a second column step with 2
    assert (g['chunks'], g['last_chunk'], g['col_steps'], g['cols_in_last_step']) == (2, 32, 2, 2)
    g = geo['w128']       # two full chunks, ragged rows and columns
    assert (g['chunks'], g['last_chunk']) == (2, 64) and g['rows_in_last_tile'] < lc.NTX_TI and g['col_steps'] > 1 and g['cols_in_last_step'] < lc.NTX_TJ
    g = geo['w129dot']    # 3 chunks, more than one column step for the running maximum
    assert (g['chunks'], g['last_chunk']) == (3, 1) and g['col_steps'] == 2 and not lc.SINGLE['w129dot'][2]
    g = geo['w200iou']    # 4 chunks, the last of 8; 5 column steps
    assert (g['chunks'], g['last_chunk'], g['col_steps']) == (4, 8, 5) and lc.SINGLE['w200iou'][4]
    g = geo['w256']       # the maximum width, exactly two row tiles
    assert (g['chunks'], g['last_chunk'], g['row_tiles'], g['rows_in_last_tile']) == (lc.NTX_MAX_CHUNKS, 64, 2, 16) and lc.SINGLE['w256'][1] == 256
    assert lc.SINGLE['w256n1'][:2] == (1, 256)
    assert geo['w100zero']['chunks'] == 2 and lc.SINGLE['w100zero'][2]
    g = geo['g1024']      # 128 row tiles, 32 column steps, two chunks
    assert (g['row_tiles'], g['col_steps'], g['chunks'], g['last_chunk']) == (128, 32, 2, 8)
    # every chunk count 2, 3, 4 in cosine or dot mode, and every case wider than the fixture's 64
    assert {g['chunks'] for g in geo.values()} == {2, 3, 4} and min(dim for _, dim, *_ in lc.SINGLE.values()) > 64
    assert all(n <= lc.NTX_MAX_GROUP and dim <= lc.NTX_MAX_CHUNKS * lc.NTX_KC for n, dim, *_ in lc.SINGLE.values())


def test_contrastive_inputs_carry_weight_in_every_feature():
    for name in lc.SINGLE:
        zis, zjs, iou = lc.single_inputs(name)
        n, dim, _, _, with_iou = lc.SINGLE[name]
        assert zis.shape == zjs.shape == (n, dim) and zis.dtype == zjs.dtype == np.float32
        rows = [r for r in range(n) if not (name == 'w100zero' and r == lc.ZERO_ROW)]
        assert (zis[rows] != 0).all() and (zjs != 0).all(), name            # no zero padding: dropping a chunk changes every s_ij
        assert (iou is not None) == with_iou
    for name in lc.SLICED:
        fpred, ftgt, occ = lc.sliced_inputs(name)
        assert fpred.shape == ftgt.shape == (lc.SLICED[name][0], lc.SLICED[name][2]) and occ.shape == (lc.SLICED[name][0],) and occ.dtype == bool
        assert (fpred != 0).all() and (ftgt != 0).all()
    assert not lc.single_inputs('w100zero')[0][lc.ZERO_ROW].any()
    iou = lc.single_inputs('w200iou')[2]
    assert iou.shape == (260, 260) and not np.array_equal(iou, iou.T) and 0.5 <= iou.min() < 0.51 and 0.99 < iou.max() <= 1.0
    # sigmoid(80 iou - 65) crosses 1/2 at iou = 0.8125: temperatures on both sides of it
    assert 0.3 < (iou > 0.8125).mean() < 0.45


def test_w129dot_has_large_logits_and_a_loss_that_is_not_saturated():
    r = lc.single_reference('w129dot')
    n, dim, cosine, tau, _ = lc.SINGLE['w129dot']
    z = np.concatenate([r['zjs'], r['zis']]).astype(np.float64)
    logits = z @ z.T / tau
    logits[np.arange(2 * n), np.arange(2 * n)] = -np.inf
    print('w129dot: largest logit %.2f, smallest %.2f, float64 loss %.4f' % (logits.max(), logits[np.isfinite(logits)].min(), r['loss_f64']))
    assert 20 <= logits.max() <= 40 and r['loss_f64'] > 1e-3


def test_single_references_are_sound():
    for name in lc.SINGLE:
        r = lc.single_reference(name)
        for k in ('zis', 'zjs'):
            g64, g32 = r['grad_%s_f64' % k], r['grad_%s_f32' % k]
            assert g64.dtype == np.float64 and g32.dtype == np.float32 and np.isfinite(g64).all() and np.isfinite(g32).all()
            if name != 'w256n1':
                # the float32 restatement is a usable yardstick: within 1e-4 of the float64 one relative to the largest entry
                assert np.abs(g32 - g64).max() <= 1e-4 * np.abs(g64).max(), name
        if name != 'w256n1':
            assert r['loss_f64'] > 1e-3 and abs(r['loss_f32'] - r['loss_f64']) <= 1e-5 * r['loss_f64'], name
    r = lc.single_reference('w256n1')
    assert r['loss_f64'] == 0 and r['loss_f32'] == 0 and not any(r[k].any() for k in r if k.startswith('grad_'))
    r = lc.single_reference('w100zero')
    assert np.abs(r['grad_zis_f64'][lc.ZERO_ROW]).max() > 1e6 > np.abs(np.delete(r['grad_zis_f64'], lc.ZERO_ROW, 0)).max()       # d (z / 1e-8) / d z


def test_sliced_cases_select_what_they_are_named_for():
    assert lc.NTX_BALLOT == 64 and lc.SLICED_TAU == 0.05
    # bench: the trainer's geometry; at least 8 groups, an occupied slice skipped for the cap, a later one still taken
    rows, slices, dim, max_rows = lc.SLICED['bench']
    assert (rows, slices, dim, max_rows) == (64 * 512, 64, 32, 1280)
    occ = lc.sliced_inputs('bench')[2]
    per_slice = occ.reshape(slices, -1).sum(1)
    assert 0.05 * 512 * 0.5 < per_slice.min() and per_slice.max() < 0.40 * 512 * 1.25 and per_slice.max() > 3 * per_slice.min()
    groups, counts = cr.select(occ, slices, max_rows)
    taken = [int(g[0]) // 512 for g in groups]
    skipped = [s for s in range(slices) if per_slice[s] > 0 and s not in taken]
    print('bench: %d groups of %d-%d rows, slices %s; first skipped %d' % (len(groups), min(map(len, groups)), max(map(len, groups)), taken, skipped[0]))
    assert counts[2] == len(groups) >= 8 and counts[0] == per_slice.sum() > max_rows >= counts[1]
    assert skipped and max(taken) > skipped[0]
    # split100: 7 slices of 100 rows = one full ballot word and 36 rows of a second; 5 trailing rows, occupied, in no slice; two chunks
    rows, slices, dim, max_rows = lc.SLICED['split100']
    p = lc.plan_geometry(rows, slices)
    assert (p['split'], p['ballot_words'], p['rows_in_last_word'], p['trailing_rows']) == (100, 2, 36, 5) and lc.ntx_geometry(1, dim)['chunks'] == 2
    occ = lc.sliced_inputs('split100')[2]
    groups, counts = cr.select(occ, slices, max_rows)
    assert occ[700:].all() and counts[2] == 7 and counts[0] == counts[1] == occ[:700].sum() and max(g.max() for g in groups) < 700
    assert 0.5 < occ[:700].mean() < 0.7
    assert all((g % 100 >= 64).any() and (g % 100 < 64).any() for g in groups)          # rows from both ballot words in every group
    # big: one group of 1200 pairs under the cap
    rows, slices, dim, max_rows = lc.SLICED['big']
    groups, counts = cr.select(lc.sliced_inputs('big')[2], slices, max_rows)
    assert counts == (1200, 1200, 1) and 1200 <= max_rows and lc.plan_geometry(rows, slices)['split'] == 2000
    g = lc.ntx_geometry(1200, dim)
    assert (g['row_tiles'], g['col_steps']) == (150, 38)
    for name in lc.SLICED:
        r = lc.sliced_reference(name)
        rest = np.setdiff1d(np.arange(lc.SLICED[name][0]), r['rows'])
        for k in ('fpred', 'ftgt'):
            g64, g32 = r['grad_%s_f64' % k], r['grad_%s_f32' % k]
            assert not g64[rest].any() and not g32[rest].any() and g64[r['rows']].any(1).all()
            assert np.abs(g32 - g64).max() <= 1e-4 * np.abs(g64).max(), name
        assert abs(r['loss_f32'] - r['loss_f64']) <= 1e-5 * r['loss_f64']


def test_shape_cases_reach_the_paths_they_are_named_for():
    assert (lc.SL_TD, lc.SL_TH, lc.SL_TW, lc.SL_FINISH) == (8, 8, 32, 256)
    assert list(lc.SHAPES.values()) == [(260, 1, 8, 8, 32), (2, 1, 24, 24, 96), (2, 1, 9, 17, 65), (1, 1, 7, 64, 5), (1, 1, 72, 8, 40)]
    geo = {name: lc.sl_geometry(shape) for name, shape in lc.SHAPES.items()}
    g = geo['b260']       # one tile per sample, 260 partials: thread 0 to 3 of the finish kernel add a second partial
    assert g['tiles_per_sample'] == 1 and g['partials'] == 260 > lc.SL_FINISH and g['finish_rounds'] == 2
    g = geo['t333']       # 3 x 3 x 3 tiles: the middle one takes all six halos from neighbouring tiles
    assert g['tiles'] == (3, 3, 3) and g['interior_tiles'] == 1 and g['last_tile'] == (8, 8, 32)
    g = geo['ragged']     # ragged on all three axes, three tiles along w, the last one column wide; a tile count per sample that is no power of two
    assert g['tiles'] == (2, 3, 3) and g['last_tile'] == (1, 1, 1) and g['tiles_per_sample'] & (g['tiles_per_sample'] - 1)
    g = geo['thin']       # d shorter than a tile, eight tiles along h, 5 of 32 columns
    assert g['tiles'] == (1, 8, 1) and g['last_tile'] == (7, 8, 5)
    g = geo['deep']       # nine tiles along d
    assert g['tiles'][0] == 9
    # the fixture's volumes stop at 12 partials (9 x 17 x 33: 2 x 3 x 2 tiles), one finish round and no interior tile
    assert all(lc.sl_geometry(s)['partials'] <= 12 and lc.sl_geometry(s)['tiles'][2] <= 2 and lc.sl_geometry(s)['interior_tiles'] == 0 for s in ((2, 1, 16, 16, 16), (1, 1, 9, 17, 33), (3, 1, 2, 3, 5)))
    assert lc.FORMULA_SHAPES == ('b260', 't333') and len(lc.SHAPE_CASES) == 10


@pytest.mark.parametrize('shape_name,stats_name', lc.SHAPE_CASES)
def test_shape_case_masks_agree_in_both_precisions(shape_name, stats_name):
    """zero differences over ALL mask entries, so the GPU comparison leaves no voxel out; >= 30 % valid; a C1 case has voxels empty on both sides"""
    r = lc.shape_reference(shape_name, stats_name)
    n = r['pred'].size
    m32, m64 = r['masks_f32'], r['masks_f64']
    diff = {k: int((m32[k] != m64[k]).sum()) for k in m64}
    print('%s %s: valid %d / %d (%.2f), empty on both sides %d, mask differences %s' % (shape_name, stats_name, r['counts'][0], n, r['counts'][0] / n, r['counts'][1], diff))
    assert not any(diff.values())
    assert r['counts_f32'] == r['counts_f64'] == (int(m64['valid'].sum()), int(m64['both'].sum()))
    assert np.array_equal(r['empty_f32'], r['empty_f64']) and np.array_equal(r['weights_f32'], r['weights_f64'].astype(np.float32))
    # (the reference holds the NORMALISED target against trunc: with the C4 statistics no voxel is empty and every weight is weight_occupied)
    assert set(np.unique(r['weights_f64'])) == ({1.0, float(lc.W_OCC)} if stats_name == 'C1' else {float(lc.W_OCC)})
    assert r['counts'][0] >= 0.3 * n
    if stats_name == 'C1':
        assert r['counts'][1] >= 1
    assert np.isfinite(r['scalars_f64']).all() and np.isfinite(r['grad_f64']).all() and np.isfinite(r['grad_f32']).all()
    # the autograd gradient of the restatement and its written-out formula are one function
    trunc, mean, std = r['params']
    import torch
    by_formula = slr.grad_by_formula(torch.from_numpy(r['pred']).double(), torch.from_numpy(r['target']).double(), trunc, mean, std, lc.W_OCC, lc.LAM_REC, lc.LAM_N).numpy()
    assert np.abs(by_formula - r['grad_f64']).max() <= 1e-9 * np.abs(r['grad_f64']).max()
    if shape_name in lc.FORMULA_SHAPES:
        assert np.abs(r['grad4_f32'] - r['grad4_f64']).max() <= 1e-3 * np.abs(r['grad4_f64']).max()


def test_every_sample_of_the_260_batch_is_its_own():
    """260 sample bases: no two samples share a prediction and hardly any a target (the radius is drawn per sample, the target rounded through float16), so
    a wrong base shows in the normals, the scalars and the gradient"""
    r = lc.shape_reference('b260', 'C1')
    assert len({row.tobytes() for row in r['pred'].reshape(260, -1)}) == 260
    assert len({row.tobytes() for row in r['target'].reshape(260, -1)}) >= 250
