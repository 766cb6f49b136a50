"""Fixture generator for the retrieval trainer's IoU matrix (CPU; needs the reference checkout, as tools/gen_contrastive_golden.py does): runs the reference's
own ``get_iou_matrix`` (util/misc.py:51-59) as written, and for the float case the trainer's expression (trainer/train_retrieval.py:85)
``get_iou_matrix(denormalize_target(batch['target']) <= 0.75 * voxel_size_target).repeat(2, 2)`` with ``PatchedSceneDataset.denormalize_target`` called
unbound, and writes tests/golden/iou_matrix.npz (arrays only).

    python tools/gen_iou_matrix_golden.py

Cases (tests/iou_matrix_ref.py GRID_CASES), each aimed at one way to go wrong:
    n1_empty, n1_full  one window: 0 / 1e-5 = 0 and V / (V + 1e-5)
    n7_5     7 windows of 5^3 = 125 voxels (a ragged last word): one empty, one full, two identical
    n33_12, n67_24     more windows than a pair tile and than a wave; 24^3 is the surface-reconstruction trainer's window
    n5_357   a window that is no cube            n3_64  64^3: 4096 words per window
    other    24 windows of 6^3; the [5, 19] block of the first 5 against the other 19 is the rectangular case (not symmetric)
    shapenet20  20 normalised targets at 32^3 with the ShapeNet constants of rfuse.configs: shells of a distance field with occupancies from a few voxels
                to about a third of the window, values on multiples of 1 / 16 (exact in float16)

Layout: ``<case>_occ`` uint8 [n, ceil(V / 8)] = np.packbits of the flattened windows, ``<case>_iou`` float32 [n, n]; ``shapenet20_target`` float16
[20, 1, 32, 32, 32], ``shapenet20_params`` float64 = (target_mean, target_std, voxel_size_target), ``shapenet20_iou`` float32 [40, 40].
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
from oracle.gen_golden import REF, save_fixture, import_reference_util_retrieval      # noqa: E402
import iou_matrix_ref as ir                                                            # noqa: E402
from rfuse import configs as rf_configs                                                # noqa: E402

LIMIT = 1 << 20


def import_reference():
    """util.misc and the dataset class behind the sys.modules stand-ins of the other generators (trimesh, tqdm, ... are not needed by what is called here)"""
    import_reference_util_retrieval()
    for n in ('tqdm', 'util.visualization'):
        if n not in sys.modules:
            try:
                __import__(n)
            except Exception:
                sys.modules[n] = types.ModuleType(n)
    for attr in ('tqdm',):
        if not hasattr(sys.modules['tqdm'], attr):
            setattr(sys.modules['tqdm'], attr, lambda x, **kw: x)
    for attr in ('visualize_pointcloud', 'visualize_sdf_as_mesh'):
        if not hasattr(sys.modules['util.visualization'], attr):
            setattr(sys.modules['util.visualization'], attr, None)
    import util.misc as misc
    from dataset.patched_scene_dataset import PatchedSceneDataset
    assert str(REF) in misc.__file__, misc.__file__
    return misc.get_iou_matrix, PatchedSceneDataset


def grids(rng, name, n, win):
    if name == 'n1_empty':
        return np.zeros((n, 1) + win, bool)
    if name == 'n1_full':
        return np.ones((n, 1) + win, bool)
    density = rng.uniform(0.02, 0.7, n)                      # a spread of occupancies
    occ = rng.random((n, 1) + win) < density[:, None, None, None, None]
    if name == 'n7_5':
        occ[1], occ[3], occ[5] = False, True, occ[2]
    return occ


def shapenet_targets(rng, d, n=20, edge=32):
    """normalised truncated distances to spherical shells of different radii and offsets; multiples of 1 / 16"""
    trunc = 3 * d['voxel_size_target']
    ax = (np.arange(edge) + 0.5) / edge * 2 - 1
    x = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1)
    out = np.empty((n, 1, edge, edge, edge), np.float32)
    for i in range(n):
        centre, radius = rng.uniform(-0.4, 0.4, 3), rng.uniform(0.05, 0.9)
        width = rng.uniform(0.5, 6.0)                         # voxels of shell per unit of distance: thin to thick shells
        raw = np.minimum(np.abs(np.linalg.norm(x - centre, axis=-1) - radius) * d['voxel_size_target'] * 16 / width, trunc)
        out[i, 0] = np.round((raw - d['target_mean']) / d['target_std'] * 16) / 16
    assert np.array_equal(out.astype(np.float16).astype(np.float32), out)
    return out


def main():
    get_iou_matrix, Dataset = import_reference()
    rng = np.random.default_rng(2027)
    out = {}
    for name, (n, win) in ir.GRID_CASES.items():
        occ = grids(rng, name, n, win)
        iou = get_iou_matrix(torch.from_numpy(occ))
        assert iou.dtype == torch.float32 and iou.shape == (n, n)
        assert torch.equal(iou, ir.count_formula(torch.from_numpy(occ))), name            # the formula the tests restate
        out[name + '_occ'] = np.packbits(occ.reshape(n, -1), axis=1)
        out[name + '_iou'] = iou.numpy()
        print('%-10s n %3d window %-12s occupancy %.3f .. %.3f   iou off the diagonal %.4f .. %.4f' % (
            name, n, win, occ.reshape(n, -1).mean(1).min(), occ.reshape(n, -1).mean(1).max(),
            (iou + 2 * torch.eye(n)).min(), (iou - 2 * torch.eye(n)).max()))
    d = rf_configs.get_config('C2')['dataset_train']
    target = torch.from_numpy(shapenet_targets(rng, d))
    ds = types.SimpleNamespace(target_mean=d['target_mean'], target_std=d['target_std'])
    occ = Dataset.denormalize_target(ds, target) <= 0.75 * d['voxel_size_target']
    iou = get_iou_matrix(occ).repeat(2, 2)
    assert torch.equal(occ, ir.occupied(target, d['target_mean'], d['target_std'], 0.75 * d['voxel_size_target']))
    assert torch.equal(iou, ir.count_formula(occ).repeat(2, 2))
    frac = occ.reshape(20, -1).float().mean(1)
    print('%-10s n  20 window (32, 32, 32) occupancy %.4f .. %.3f   iou off the diagonal up to %.4f' % (ir.FLOAT_CASE, frac.min(), frac.max(), (iou[:20, :20] - 2 * torch.eye(20)).max()))
    assert frac.min() > 0 and frac.max() > 0.2 and frac.max() / frac.min() > 20, 'the targets need a real spread of occupancies'
    out[ir.FLOAT_CASE + '_target'] = target.numpy().astype(np.float16)
    out[ir.FLOAT_CASE + '_params'] = np.array([d['target_mean'], d['target_std'], d['voxel_size_target']], np.float64)
    out[ir.FLOAT_CASE + '_iou'] = iou.numpy()
    save_fixture('iou_matrix', **out)
    size = (REPO / 'tests' / 'golden' / 'iou_matrix.npz').stat().st_size
    print('tests/golden/iou_matrix.npz: %d bytes' % size)
    assert size <= LIMIT


if __name__ == '__main__':
    main()
