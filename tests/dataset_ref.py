"""Shared by tests/test_dataset_cpu.py, tests/test_dataset_gpu.py, tools/gen_dataset_golden.py and tools/data_loader_bench.py: a from-scratch numpy restatement of
what the reference's ``SceneHandler`` (dataset/scene.py) and ``PatchedSceneDataset`` (dataset/patched_scene_dataset.py) compute per item, the toy dataset of
the fixture tests/golden/dataset.npz, and the fixture's layout.  Nothing here imports the product package.

The restatement, operation by operation:
  extents     per axis ``np.linspace(0, size - patch, (size - patch) // stride + 1).astype(int32)``, meshgrid 'ij', end = start + patch + 2 context
              (scene.py:152-167); the input side uses ``int(size / scale_factor)`` and ``int(stride * patch_in / patch_tgt)``
  occupancy   the padded float32 scene's window ``<= float32(1.5) * float32(float16(voxel_size_target))``, summed (scene.py:148-150)
  batch       ``(window - float32(mean)) / float32(std)`` of the padded scene cast to float32 (patched_scene_dataset.py:117-137); without retrievals four
              channels of the truncation, not normalised
  points      ``pc[row] * scale`` in the cloud's type, ``np.clip(., 0, grid - 1).astype(uint32) + pad`` (scene.py:81-90, util/misc.py:73-78); a cloud of fewer
              than 20000 rows is stacked twice.  Only the item's window is built.  A point with a NaN coordinate is skipped (the reference leaves it undefined).

The reference pads the composed retrievals [K, X, Y, Z] with ``np.pad(arr, context)``, which also pads the K axis: its ``retrieval`` has K + 2 context
channels, the first and last ``context`` of them constant.  ``batch_item`` returns the K real channels, which are channels context .. context + K of the
reference's array; the fixture's digests are taken over those, and the generator asserts that the others hold the normalised truncation.

The toy dataset: scenes are uint8 codes, value = code * unit (units are powers of two, so every value is exact in float16), code 255 = NaN.  With
voxel_size_target = 11 / 512 the truncation is code 66 and the occupancy threshold is exactly code 33 of the targets."""
import hashlib

import numpy as np

NAN_CODE = 255
TARGET_UNIT, INPUT_UNIT, CLOUD_UNIT = 1.0 / 1024, 1.0 / 256, 1.0 / 64
CLOUD_POS_INF, CLOUD_NEG_INF = 32767, -32768
DOUBLED_BELOW = 20000
SCENES = ('a', 'b', 'c')
VOXEL_T = 11.0 / 512
_BASE = {'dataset_name': 'Toy', 'target_chunk_size': 64, 'input_mean': 0.3095340441938771, 'input_std': 0.14730652990291243,
         'target_mean': 0.059954833543534335, 'target_std': 0.010110036361741626, 'voxel_size_target': VOXEL_T, 'occupancy_threshold': 2, 'train_multiplier': 2}
# the dataset sections of the three toy configurations (the keys the reference's YAML files use)
DF = dict(_BASE, voxel_size_input=8 * VOXEL_T, input_chunk_size=8, num_points=0, patch_size_target=16, patch_context_target=8, patch_stride=16,
          patch_size_input=2, patch_context_input=1)
PC = dict(_BASE, voxel_size_input=0, input_mean=0.25, input_std=0.7, input_chunk_size=64, num_points=100, patch_size_target=16, patch_context_target=4,
          patch_stride=16, patch_size_input=32, patch_context_input=8)
FULL = dict(_BASE, voxel_size_input=0, input_mean=0.0, input_std=1.0, input_chunk_size=128, num_points=100, patch_size_target=64, patch_context_target=0,
            patch_stride=64, patch_size_input=128, patch_context_input=0, train_multiplier=1)
# run -> (dataset section, task, no_retrievals, split, scenes of the split, cloud dtype, table dtype)
RUNS = {'df_train': (DF, 'superresolution', False, 'train', ('a', 'b', 'c'), None, None),
        'df_val': (DF, 'superresolution', False, 'val', ('c', 'b'), None, None),
        'pc32_train': (PC, 'surface_reconstruction', True, 'train', ('a', 'b'), 'float32', 'uint16'),
        'pc64_train': (PC, 'surface_reconstruction', True, 'train', ('a', 'b'), 'float64', 'int64'),
        'full_train': (FULL, 'surface_reconstruction', True, 'train', ('d',), 'float32', 'int64')}
RANDOM_SEED = 4242          # random.seed before a run's items are read in order: one random.randint(0, R - 1) per point-cloud item


def f16(x):
    return np.float16(x).astype(np.float32)


def decode(codes, unit):
    out = codes.astype(np.float32) * np.float32(unit)
    out[codes == NAN_CODE] = np.nan
    return out


def decode_cloud(codes, dtype, tilt, unit=CLOUD_UNIT):
    """coordinates = code * unit (1 / 64); the float64 clouds (``tilt``) sit 2^-40 below that, so that a coordinate on a voxel boundary falls into the voxel below --
    a float32 evaluation of a float64 cloud would put it into the voxel above"""
    out = codes.astype(np.float64) * unit
    if tilt:
        out -= 2.0 ** -40
    out[codes == CLOUD_POS_INF] = np.inf
    out[codes == CLOUD_NEG_INF] = -np.inf
    return out.astype(dtype)


# ------------------------------------------------------------------------------------------------ the restatement
class Geometry:
    def __init__(self, d):
        self.pt, self.ct, self.st = d['patch_size_target'], d['patch_context_target'], d['patch_stride']
        self.pi, self.ci = d['patch_size_input'], d['patch_context_input']
        self.si = int(d['patch_stride'] * d['patch_size_input'] / d['patch_size_target'])
        self.scale_factor = d['patch_size_target'] / d['patch_size_input']
        self.wt, self.wi = self.pt + 2 * self.ct, self.pi + 2 * self.ci
        self.target_trunc, self.input_trunc = f16(d['voxel_size_target'] * 3), f16(d['voxel_size_input'] * 3)
        self.threshold = np.float32(1.5) * f16(d['voxel_size_target'])


def extents_for_size(size, patch, context, stride):
    axes = [np.linspace(0, s - patch, (s - patch) // stride + 1).astype(np.int32) for s in size]
    x, y, z = (a.flatten() for a in np.meshgrid(*axes, indexing='ij'))
    w = patch + 2 * context
    return np.stack([x, x + w, y, y + w, z, z + w], axis=1)


def scene_patches(size_target, g):
    size_input = [int(s / g.scale_factor) for s in size_target]
    return extents_for_size(size_input, g.pi, g.ci, g.si), extents_for_size(size_target, g.pt, g.ct, g.st)


def name_of(scene, e):
    return '%s--%04d_%04d_%04d_%04d_%04d_%04d' % ((scene,) + tuple(int(v) for v in e))


def padded(volume, context, fill, store_dtype):
    """the scene as the reference holds it: stored in ``store_dtype``, padded with the truncation, read as float32.  [K, X, Y, Z] pads the three last axes."""
    width = [(0, 0)] * (volume.ndim - 3) + [(context, context)] * 3
    return np.pad(volume.astype(store_dtype), width, mode='constant', constant_values=fill).astype(np.float32)


def cut(vol, e):
    return vol[..., e[0]:e[1], e[2]:e[3], e[4]:e[5]]


def occupancy(target, e, g, store_dtype=np.float16):
    return int((cut(padded(target, g.ct, g.target_trunc, store_dtype), e) <= g.threshold).sum())


def normalise(x, mean, std):
    return (x - np.float32(mean)) / np.float32(std)


def point_window(cloud, indices, grid_res, scale, pad, start, w):
    """the window [start, start + w)^3 of point_cloud_to_grid(pc[indices], grid_res, scale, pad), float32 zeros and ones"""
    pc = cloud if cloud.shape[0] >= DOUBLED_BELOW else np.vstack([cloud, cloud])
    p = pc[np.asarray(indices).astype(np.int64), :] * scale
    p = p[~np.isnan(p).any(axis=1)]
    q = np.clip(p, 0, grid_res - 1).astype(np.uint32).astype(np.int64) + pad - np.asarray(start, dtype=np.int64)[None, :]
    q = q[((q >= 0) & (q < w)).all(axis=1)]
    out = np.zeros((w, w, w), dtype=np.float32)
    out[q[:, 0], q[:, 1], q[:, 2]] = 1
    return out


class RefDataset:
    """The items of one split and what ``__getitem__`` returns for them.  ``scenes``: name -> dict with 'target' and optionally 'input', 'cloud', 'retrieval'
    (unpadded float arrays); ``occupancy``: name -> count, or None to compute it."""

    def __init__(self, d, task, no_retrievals, split, names, scenes, table=None, store_dtype=np.float16, occupancy_table=None):
        self.d, self.g, self.task, self.no_retrievals, self.scenes, self.table, self.store_dtype = d, Geometry(d), task, no_retrievals, scenes, table, store_dtype
        self.names = list(names)
        self.occupancy = {} if occupancy_table is None else dict(occupancy_table)
        self.data = []
        for s in self.names:
            e_in, e_tgt = scene_patches(scenes[s]['target'].shape, self.g)
            if len(e_in) != len(e_tgt):
                raise ValueError('scene %s: %d input and %d target patches' % (s, len(e_in), len(e_tgt)))
            for i in range(len(e_tgt)):
                nm = name_of(s, e_tgt[i])
                if nm not in self.occupancy:
                    self.occupancy[nm] = occupancy(scenes[s]['target'], e_tgt[i], self.g, store_dtype)
                if self.occupancy[nm] > d['occupancy_threshold']:
                    self.data.append((s, e_in[i], e_tgt[i]))
        if split == 'train':
            self.data = self.data * d['train_multiplier']

    def __len__(self):
        return len(self.data)

    def item(self, index, table_row=None):
        s, e_in, e_tgt = self.data[index]
        d, g, sc = self.d, self.g, self.scenes[s]
        if self.task == 'surface_reconstruction':
            grid = point_window(sc['cloud'], self.table[table_row], d['input_chunk_size'], 1 / g.scale_factor, g.ci, e_in[0::2], g.wi)
        else:
            grid = cut(padded(sc['input'], g.ci, g.input_trunc, self.store_dtype), e_in)
        target = cut(padded(sc['target'], g.ct, g.target_trunc, self.store_dtype), e_tgt)
        if self.no_retrievals:
            retrieval = np.ones((4, g.wt, g.wt, g.wt), dtype=np.float32) * g.target_trunc
        else:
            retrieval = normalise(cut(padded(sc['retrieval'], g.ct, g.target_trunc, self.store_dtype), e_tgt), d['target_mean'], d['target_std'])
        return {'name': name_of(s, e_tgt), 'scene': s, 'extent': e_tgt, 'input': normalise(grid[None], d['input_mean'], d['input_std']),
                'target': normalise(target[None], d['target_mean'], d['target_std']), 'retrieval': retrieval}

    def batch(self, indices, table_rows=None):
        """what the reference's default collate makes of the items, as numpy arrays"""
        items = [self.item(int(i), None if table_rows is None else int(table_rows[k])) for k, i in enumerate(indices)]
        out = {k: np.stack([it[k] for it in items]) for k in ('input', 'target', 'retrieval')}
        out['extent'] = np.stack([it['extent'] for it in items]).astype(np.int32)
        out['name'] = [it['name'] for it in items]
        return out


# ------------------------------------------------------------------------------------------------ the fixture
def digest(a):
    """SHA-256 of a float32 array's bytes, every NaN as the one quiet NaN 0x7fc00000 (which NaN an operation returns is not part of the contract)"""
    a = np.array(a, dtype=np.float32, order='C', copy=True)
    a[np.isnan(a)] = np.frombuffer(np.uint32(0x7fc00000).tobytes(), dtype=np.float32)[0]
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)


def toy_scenes(z, cloud_dtype=None, store=np.float32):
    """name -> fields of the toy dataset, decoded from the fixture's codes.  Scene 'd' (the whole-grid case) is scene 'a' tiled 2 x 2 x 2."""
    out = {}
    for s in SCENES:
        out[s] = {'target': decode(z['target_' + s], TARGET_UNIT), 'input': decode(z['input_' + s], INPUT_UNIT), 'retrieval': decode(z['retr_' + s], TARGET_UNIT)}
    out['d'] = {'target': np.tile(out['a']['target'], (2, 2, 2))}
    if cloud_dtype is not None:
        tilt = np.dtype(cloud_dtype) == np.float64
        codes = z['cloud_codes']
        out['a']['cloud'] = decode_cloud(codes, cloud_dtype, tilt)
        out['b']['cloud'] = decode_cloud(codes[:12000, ::-1], cloud_dtype, tilt)
        out['d']['cloud'] = decode_cloud(codes, cloud_dtype, tilt, 2 * CLOUD_UNIT)            # a 64-unit scene: the 128^3 grid at scale 2
    return out


def load_fixture(golden_dir):
    with np.load(golden_dir / 'dataset.npz', allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def run_dataset(z, run, store_dtype=np.float16, occupancy_table=None):
    d, task, no_retr, split, names, cloud_dtype, table_dtype = RUNS[run]
    table = None if table_dtype is None else z['table'].astype(table_dtype)
    return RefDataset(d, task, no_retr, split, names, toy_scenes(z, cloud_dtype), table, store_dtype, occupancy_table)


def store_fields(z, run):
    """(scene names, targets, inputs, clouds, retrievals) for a store that serves ``run``: the split's scenes in sorted order, which for df_val is not the
    split's own order"""
    d, task, no_retr, split, names, cloud_dtype, table_dtype = RUNS[run]
    scenes = toy_scenes(z, cloud_dtype)
    order = sorted(names)
    pc = task == 'surface_reconstruction'
    return (order, [scenes[s]['target'] for s in order], None if pc else [scenes[s]['input'] for s in order], [scenes[s]['cloud'] for s in order] if pc else None,
            None if no_retr else [scenes[s]['retrieval'] for s in order])
