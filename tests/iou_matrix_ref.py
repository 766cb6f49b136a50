"""Shared by tests/test_iou_matrix_cpu.py, tests/test_iou_matrix_gpu.py and tools/gen_iou_matrix_golden.py: the count formula of the reference's
``get_iou_matrix`` (util/misc.py:51-59) in torch on the CPU, the trainer's occupancy rule, and the fixture's layout.

The reference sums bools to int64 and evaluates ``intersection / (union + 1e-5)``: the int64 union becomes float32, 1e-5 is added as a float32, the int64
intersection becomes float32 and is divided.  For counts below 2^24 that is ``float32(inter) / (float32(union) + float32(1e-5))``, which ``count_formula``
evaluates from an integer matrix product instead of four [n^2, D, H, W] tensors."""
import numpy as np
import torch

# name -> (n, window); 'other' is 5 against 19 windows: the first 5 and the last 19 of 24
GRID_CASES = {'n1_empty': (1, (4, 4, 4)), 'n1_full': (1, (4, 4, 4)), 'n7_5': (7, (5, 5, 5)), 'n33_12': (33, (12, 12, 12)), 'n67_24': (67, (24, 24, 24)),
              'n5_357': (5, (3, 5, 7)), 'n3_64': (3, (64, 64, 64)), 'other': (24, (6, 6, 6))}
FLOAT_CASE = 'shapenet20'          # 20 normalised float32 targets at 32^3, the ShapeNet constants, the trainer's .repeat(2, 2)
OTHER_SPLIT = 5


def count_formula(a, b=None):
    """a bool [n, ...], b bool [m, ...] or None (= a) -> float32 [n, m], the reference's bits"""
    fa = a.reshape(a.shape[0], -1).to(torch.int64)
    fb = fa if b is None else b.reshape(b.shape[0], -1).to(torch.int64)
    inter = fa @ fb.t()
    union = fa.sum(1)[:, None] + fb.sum(1)[None, :] - inter
    return inter.to(torch.float32) / (union.to(torch.float32) + 1e-5)


def occupied(target, target_mean, target_std, threshold):
    """the trainer's ``denormalize_target(batch['target']) <= 0.75 * voxel_size_target`` on a float32 tensor: Python scalars beside a float32 tensor"""
    return target * target_std + target_mean <= threshold


def load_fixture(golden_dir):
    z = np.load(golden_dir / 'iou_matrix.npz', allow_pickle=False)
    cases = {}
    for name, (n, win) in GRID_CASES.items():
        v = int(np.prod(win))
        occ = np.unpackbits(z[name + '_occ'], axis=1, count=v).astype(bool).reshape((n, 1) + win)
        cases[name] = {'occ': torch.from_numpy(occ), 'iou': torch.from_numpy(z[name + '_iou'])}
    cases[FLOAT_CASE] = {'target': torch.from_numpy(z[FLOAT_CASE + '_target'].astype(np.float32)), 'params': z[FLOAT_CASE + '_params'],
                         'iou': torch.from_numpy(z[FLOAT_CASE + '_iou'])}
    return cases
