"""Generated cases for the loss kernels' tiling paths (csrc/ntxent.hip, csrc/shape_loss.hip): seeded inputs in plain numpy / torch on the CPU and their
float64 / float32 references from the restatements of tests/contrastive_ref.py and tests/shape_loss_ref.py, which tests/test_contrastive_cpu.py and
tests/test_shape_loss_cpu.py pin against the reference-generated fixtures.  Used by tests/test_loss_sweep_cpu.py (what every case reaches, and the conditions
that keep a comparison from hiding a failure) and tests/test_loss_sweep_gpu.py (the kernels against these references).

The geometry functions restate the kernels' constants: they say which tiling paths a shape reaches without asking the code under test.
"""
import functools

import numpy as np
import torch

import contrastive_ref as cr
import shape_loss_ref as slr

# ------------------------------------------------------------------------------------------------ contrastive loss: csrc/ntxent.hip
NTX_TI, NTX_TJ, NTX_KC = 16, 64, 64           # rows of a tile, columns per step, features per LDS chunk (kTI, kTJ, kKC)
NTX_MAX_CHUNKS, NTX_MAX_GROUP = 4, 4096       # kMaxChunks, kMaxGroup
NTX_BALLOT = 64                               # rows per ballot word of the plan kernel

#          name        n     dim  cosine tau   iou
SINGLE = {'w65':      (9,    65,  True,  0.07, False),
          'w96':      (33,   96,  True,  0.07, False),
          'w128':     (67,   128, True,  0.07, False),
          'w129dot':  (40,   129, False, 0.5,  False),
          'w200iou':  (130,  200, True,  0.07, True),
          'w256':     (16,   256, True,  0.07, False),
          'w256n1':   (1,    256, True,  0.07, False),
          'w100zero': (5,    100, True,  0.07, False),
          'g1024':    (1024, 72,  True,  0.07, False)}
SIG_SCALE, SIG_SHIFT = 80.0, -65.0
ZERO_ROW = 3                                  # of w100zero's zis

#          name        rows        slices dim  max_rows
SLICED = {'bench':    (64 * 512,   64,    32,  1280),
          'split100': (705,        7,     70,  1280),
          'big':      (2000,       1,     32,  1280)}
SLICED_TAU = 0.05


def ceil_div(a, b):
    return -(-a // b)


def ntx_geometry(n, dim):
    """what one group of n pairs of dim features reaches in k_ntx_lse / k_ntx_bwd"""
    chunks = ceil_div(dim, NTX_KC)
    return {'chunks': chunks, 'last_chunk': dim - (chunks - 1) * NTX_KC, 'row_tiles': ceil_div(2 * n, NTX_TI), 'rows_in_last_tile': 2 * n - (ceil_div(2 * n, NTX_TI) - 1) * NTX_TI,
            'col_steps': ceil_div(2 * n, NTX_TJ), 'cols_in_last_step': 2 * n - (ceil_div(2 * n, NTX_TJ) - 1) * NTX_TJ}


def plan_geometry(rows, slices):
    """what the plan kernel's ballot loop sees of one slice"""
    split = rows // slices
    words = ceil_div(split, NTX_BALLOT)
    return {'split': split, 'ballot_words': words, 'rows_in_last_word': split - (words - 1) * NTX_BALLOT, 'trailing_rows': rows - slices * split}


def _seed(name):
    return 1000 + sum(ord(c) * (i + 1) for i, c in enumerate(name))


def single_inputs(name):
    """-> zis, zjs float32 [n, dim], iou float32 [2n, 2n] or None.  zjs = zis + noise; every feature of every chunk is a full randn: no padding"""
    n, dim, cosine, tau, with_iou = SINGLE[name]
    rng = np.random.default_rng(_seed(name))
    zis = rng.standard_normal((n, dim))
    if name == 'w129dot':
        # dot-product logits s / tau without a normalisation: a component shared by all rows lifts EVERY logit to 20-40 (the running maximum then has to carry
        # large values across the column steps), while their spread stays of the order 5, so that the loss does not saturate to 0
        zis = 0.15 * zis + 0.29 * rng.standard_normal((1, dim))
        zjs = zis + 0.15 * rng.standard_normal((n, dim))
    else:                          # noise of twice the signal: the positive's cosine is about 0.45, the loss of the order 1, and the float32 reference keeps its digits
        zjs = zis + 2.0 * rng.standard_normal((n, dim))
    if name == 'w100zero':
        zis[ZERO_ROW] = 0
    iou = (0.5 + 0.5 * rng.random((2 * n, 2 * n))).astype(np.float32) if with_iou else None
    return zis.astype(np.float32), zjs.astype(np.float32), iou


def sliced_inputs(name):
    """-> fpred, ftgt float32 [rows, dim], occupancy bool [rows]"""
    rows, slices, dim, _ = SLICED[name]
    rng = np.random.default_rng(_seed(name))
    fpred = rng.standard_normal((rows, dim))
    ftgt = fpred + 1.5 * rng.standard_normal((rows, dim))
    split = rows // slices
    occ = np.zeros(rows, bool)
    if name == 'bench':            # per-slice occupancy between 5 % and 40 %: groups of different sizes, so that a slice is skipped for the cap and a later one fits
        for s, share in enumerate(rng.uniform(0.05, 0.40, slices)):
            occ[s * split:(s + 1) * split] = rng.random(split) < share
    elif name == 'split100':       # about 60 %; the 5 rows behind the last slice are occupied too and belong to no slice
        occ[:slices * split] = rng.random(slices * split) < 0.6
        occ[slices * split:] = True
    else:                          # exactly 1200 of the 2000 rows
        occ[rng.permutation(rows)[:1200]] = True
    return fpred.astype(np.float32), ftgt.astype(np.float32), occ


def _grads(loss, *leaves):
    if loss.requires_grad:
        loss.backward()
    return [np.zeros(tuple(t.shape), np.float64 if t.dtype == torch.float64 else np.float32) if t.grad is None else t.grad.numpy() for t in leaves]


@functools.lru_cache(maxsize=None)
def single_reference(name):
    """-> {'zis', 'zjs', 'iou', and per precision p in (f32, f64): 'loss_p', 'grad_zis_p', 'grad_zjs_p'}; computed once, never modified"""
    n, dim, cosine, tau, _ = SINGLE[name]
    zis, zjs, iou = single_inputs(name)
    out = {'zis': zis, 'zjs': zjs, 'iou': iou}
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        a, b = (torch.from_numpy(v).to(dt).requires_grad_(True) for v in (zis, zjs))
        loss = cr.ntxent(a, b, tau, cosine, None if iou is None else torch.from_numpy(iou).to(dt), SIG_SCALE, SIG_SHIFT)
        out['grad_zis_' + tag], out['grad_zjs_' + tag] = _grads(loss, a, b)
        out['loss_' + tag] = loss.item()
    return out


@functools.lru_cache(maxsize=None)
def sliced_reference(name):
    """-> {'fpred', 'ftgt', 'occ', 'rows' (the selected rows in slice order), 'counts', and per precision 'loss_p', 'grad_fpred_p', 'grad_ftgt_p' [rows, dim]}"""
    rows, slices, dim, max_rows = SLICED[name]
    fpred, ftgt, occ = sliced_inputs(name)
    groups, counts = cr.select(occ, slices, max_rows)
    out = {'fpred': fpred, 'ftgt': ftgt, 'occ': occ, 'rows': np.concatenate(groups), 'counts': np.array(counts, np.int64), 'groups': groups}
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        a, b = (torch.from_numpy(v).to(dt).requires_grad_(True) for v in (fpred, ftgt))
        loss, c = cr.sliced(slices, a, b, occ, SLICED_TAU, max_rows)
        assert c == counts
        out['grad_fpred_' + tag], out['grad_ftgt_' + tag] = _grads(loss, a, b)
        out['loss_' + tag] = loss.item()
    return out


# ------------------------------------------------------------------------------------------------ shape loss: csrc/shape_loss.hip
SL_TD, SL_TH, SL_TW = 8, 8, 32                # the tile (kTD, kTH, kTW)
SL_FINISH = 256                               # threads of k_shape_loss_finish = the stride of its loop over the partials
W_OCC, LAM_REC, LAM_N = 8, 1.0, 0.5
# target mean / std per dataset: the mean rounded to a few bits, the std a power of two (tools/gen_shape_loss_golden.py STATS: den(T) of a flat region is then
# trunc itself in float32 and in float64, and both precisions see the same masks); trunc = rfuse.configs.truncations(config)[1]
STATS = {'C1': (0.0625, 15 / 256, 2.0 ** -7), 'C4': (11.25, 10.5, 2.0)}
SHAPES = {'b260': (260, 1, 8, 8, 32), 't333': (2, 1, 24, 24, 96), 'ragged': (2, 1, 9, 17, 65), 'thin': (1, 1, 7, 64, 5), 'deep': (1, 1, 72, 8, 40)}
FORMULA_SHAPES = ('b260', 't333')             # also (total + 3 l1).backward() against grad_by_formula(a = 4, b = 0.5)
SHAPE_SEED = 5
SHAPE_CASES = [(s, c) for s in SHAPES for c in STATS]


def sl_geometry(shape):
    b, _, d, h, w = shape
    td, th, tw = ceil_div(d, SL_TD), ceil_div(h, SL_TH), ceil_div(w, SL_TW)
    return {'tiles': (td, th, tw), 'tiles_per_sample': td * th * tw, 'partials': b * td * th * tw, 'finish_rounds': ceil_div(b * td * th * tw, SL_FINISH),
            'interior_tiles': max(td - 2, 0) * max(th - 2, 0) * max(tw - 2, 0), 'last_tile': (d - (td - 1) * SL_TD, h - (th - 1) * SL_TH, w - (tw - 1) * SL_TW)}


def make_inputs(shape, trunc, mean, std, seed, flat=False):
    """The recipe of tools/gen_shape_loss_golden.py:make_inputs (tests/test_loss_sweep_cpu.py holds it to the fixture's inputs bit for bit): raw target
    | |x| - r | * 4 trunc on a linspace(-1, 1) grid, clamped at trunc and rounded through float16, r per sample in [0.45, 0.75]; target = the raw target
    normalised; pred = clamp(2 raw / trunc - 1 + 0.3 randn, -1, 1) with the noise zeroed on the first third of the last axis."""
    rng = np.random.default_rng(seed)
    b, _, d, h, w = shape
    if flat:
        raw = np.full(shape, trunc, np.float32)
        pred = np.ones(shape, np.float32)
    else:
        ext = 1.0 if min(d, h, w) >= 8 else 0.6      # a volume of a few voxels: keep the corners inside the band, or the target is flat
        ax = [np.linspace(-ext, ext, n) if n > 1 else np.zeros(1) for n in (d, h, w)]
        x = np.stack(np.meshgrid(*ax, indexing='ij'), -1)
        r = rng.uniform(0.45, 0.75, b)
        raw = np.abs(np.linalg.norm(x, axis=-1)[None] - r[:, None, None, None]) * 4 * trunc
        raw = np.minimum(raw, trunc).astype(np.float16).astype(np.float32)[:, None]
        noise = 0.3 * rng.standard_normal(shape)
        noise[..., :w // 3] = 0
        if not float(np.log2(trunc)).is_integer():
            # trunc no power of two: without noise pred would equal the network-space target up to its last bit, and sign(pred - target) would be decided by
            # rounding, differently in float32 and float64 (with trunc = 2^-4 the two are EQUAL there, which is the subgradient-at-0 case and stays)
            noise[..., :w // 3] = np.where(raw < trunc, -0.0625, 0.0)[..., :w // 3]
        pred = np.clip(2 * raw.astype(np.float64) / trunc - 1 + noise, -1, 1).astype(np.float32)
    target = ((raw - np.float32(mean)) / np.float32(std)).astype(np.float32)
    return target, pred


def _masks(pred, target, trunc, mean, std):
    """the three masks of the loss as the restatement forms them, in the dtype of its arguments"""
    _, empty, nt = slr.augment(target, trunc, mean, std, W_OCC)
    df = (pred + 1) * trunc / 2
    valid = (slr.sobel(df, trunc) != 0).any(1) & (nt != 0).any(1)
    return {'valid': valid.numpy(), 'empty': empty.numpy(), 'both': (empty & (df >= trunc)).numpy(), 'normals_zero': (nt == 0).numpy()}


@functools.lru_cache(maxsize=None)
def shape_reference(shape_name, stats_name):
    """-> {'params' = trunc, mean, std; 'target', 'pred', 'counts'; per precision p: 'weights_p', 'empty_p', 'normals_p', 'scalars_p' [3] = total, l1, normal,
    'grad_p' of total, 'masks_p'; for FORMULA_SHAPES also 'grad4_p' = grad_by_formula(a = 4, b = 0.5)}; computed once, never modified"""
    trunc, mean, std = STATS[stats_name]
    target, pred = make_inputs(SHAPES[shape_name], trunc, mean, std, SHAPE_SEED)
    out = {'params': (trunc, mean, std), 'target': target, 'pred': pred}
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        t = torch.from_numpy(target).to(dt)
        p = torch.from_numpy(pred).to(dt).requires_grad_(True)
        weights, empty, nt = slr.augment(t, trunc, mean, std, W_OCC)
        out['weights_' + tag], out['empty_' + tag], out['normals_' + tag] = weights.numpy(), empty.numpy(), nt.numpy()
        total, l1, normal, counts = slr.loss(p, t, trunc, mean, std, W_OCC, LAM_REC, LAM_N)
        total.backward()
        out['scalars_' + tag] = np.array([total.item(), l1.item(), normal.item()], np.float64)
        out['grad_' + tag], out['counts_' + tag] = p.grad.numpy(), counts
        out['masks_' + tag] = _masks(p.detach(), t, trunc, mean, std)
        if shape_name in FORMULA_SHAPES:
            out['grad4_' + tag] = slr.grad_by_formula(p.detach(), t, trunc, mean, std, W_OCC, 4.0, 0.5).numpy()
    out['counts'] = np.array(out['counts_f64'], np.int64)
    return out
