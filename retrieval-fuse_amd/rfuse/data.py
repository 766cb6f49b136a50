"""The device-resident patch dataset: what the reference's ``SceneHandler`` (dataset/scene.py) and ``PatchedSceneDataset`` (dataset/patched_scene_dataset.py)
hand a trainer, assembled by HIP kernels (csrc/dataset.hip, include/rfuse_data.h) from scenes that live on the device.

  SceneStore       scene names and their unpadded targets, optionally inputs, point clouds and composed retrievals, as flat device arrays with per-scene
                   offsets and sizes; float16 (the reference's ``preload_scenes`` cast, the default) or float32 (its from-disk path)
  patch_extents    both extent lists of ``SceneHandler.get_scene_patches`` (scene.py:152-167), in its order
  patch_occupancy  ``calculate_occupancy_for_name`` (scene.py:148-150) for every patch, on the device; ``occupancy_json`` / ``read_occupancy`` write and read the
                   reference's ``data/occupancy/<dataset>_<chunk:03d>_<patch:02d>_<ctx:02d>.json``
  PatchDataset     the items with ``count > occupancy_threshold`` in the reference's order (times ``train_multiplier`` for 'train'); ``batch`` returns the
                   reference's ``input`` / ``target`` / ``retrieval`` / ``extent`` for a set of items as device tensors
  BatchLoader      yields those batches for an epoch; permutation and point-cloud rows come from a device generator, nothing waits for the host

The numbers are the reference's, bit for bit: ``(v - float32(mean)) / float32(std)`` of the stored value read as float32, padding = the truncation
rounded through float16, occupancy threshold = ``float32(1.5) * float32(float16(voxel_size_target))``.

One deliberate difference.  The reference pads its composed retrievals with ``np.pad(arr, context)`` (scene.py:74,99), which pads the K axis of the
[K, X, Y, Z] array as well: its ``retrieval`` has K + 2 context channels, the first ``context`` of them constant, and the trainer's ``[:, :K]`` then reads
only padding.  ``batch`` returns the K composed retrievals, the reference's channels context .. context + K.

There is no CPU path for the kernels: a store on the CPU serves the host-side bookkeeping only (extents, names, masks from a given occupancy table)."""
import contextlib
import json
from pathlib import Path

import numpy as np
import torch

from . import _lib
from .formats import parse_patch_name, patch_name, scene_patch_extents
from .ops import _p, _stream

DOUBLED_BELOW = 20000          # scene.py:86-87: a cloud with fewer rows is read stacked twice
_TABLE_KINDS = {np.dtype(np.uint16): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2}


def _f16(x):
    return float(np.float16(x).astype(np.float32))


def _f32(x):
    return float(np.float32(x))


def _scoped(device):
    if device.type != 'cuda' or device.index == torch.cuda.current_device():
        return contextlib.nullcontext()
    return torch.cuda.device(device)


class Geometry:
    """The window geometry of a dataset section (the reference's YAML keys) and the constants derived from it (scene.py:30-40)."""

    def __init__(self, d):
        self.patch_target, self.context_target, self.stride_target = int(d['patch_size_target']), int(d['patch_context_target']), int(d['patch_stride'])
        self.patch_input, self.context_input = int(d['patch_size_input']), int(d['patch_context_input'])
        self.stride_input = int(d['patch_stride'] * d['patch_size_input'] / d['patch_size_target'])
        self.scale_factor = d['patch_size_target'] / d['patch_size_input']
        self.window_target, self.window_input = self.patch_target + 2 * self.context_target, self.patch_input + 2 * self.context_input
        self.target_trunc, self.input_trunc = _f16(d['voxel_size_target'] * 3), _f16(d.get('voxel_size_input', 0) * 3)
        self.threshold = _f32(np.float32(1.5) * np.float16(d['voxel_size_target']).astype(np.float32))      # 0.75 * 2 * target_voxel_size, scene.py:150

    def input_size(self, size):
        return [int(s / self.scale_factor) for s in size]


def _geometry(g):
    return g if isinstance(g, Geometry) else Geometry(g)


def patch_extents(size, geometry):
    """``SceneHandler.get_scene_patches`` (scene.py:152-167) for a scene of unpadded target ``size``: (input extents, target extents), int32 [P, 6] each, padded
    coordinates, the reference's order.  Starts are ``np.linspace(0, size - patch, (size - patch) // stride + 1).astype(int32)`` per axis, so sizes that the
    stride does not divide get the reference's irregular starts.  The reference indexes both lists with one counter; lists of different lengths raise here."""
    g = _geometry(geometry)
    if any(s < g.patch_target for s in size) or any(s < g.patch_input for s in g.input_size(size)):
        raise ValueError('patch_extents: a scene of %s (input %s) is smaller than a patch (%d, input %d)' % (tuple(size), tuple(g.input_size(size)), g.patch_target, g.patch_input))
    e_in = scene_patch_extents(g.input_size(size), g.patch_input, g.context_input, g.stride_input)
    e_tgt = scene_patch_extents(size, g.patch_target, g.context_target, g.stride_target)
    if len(e_in) != len(e_tgt):
        raise ValueError('patch_extents: a scene of %s has %d target patches but its input of %s has %d' % (tuple(size), len(e_tgt), tuple(g.input_size(size)), len(e_in)))
    return e_in, e_tgt


# ------------------------------------------------------------------------------------------------ the store
class _Field:
    """One flat device array of volumes [channels, X, Y, Z] per scene + offsets (int64, elements) and sizes (int32 [n, 3])."""

    def __init__(self, volumes, channels, dtype, device, what):
        np_dtype = np.float16 if dtype == torch.float16 else np.float32
        flat, offsets, sizes, at = [], [], [], 0
        for v in volumes:
            v = np.asarray(v)
            if v.ndim != (3 if channels == 1 else 4) or (channels > 1 and v.shape[0] != channels) or v.size == 0:
                raise ValueError('%s: expected %s volumes, got an array of shape %s' % (what, '[X, Y, Z]' if channels == 1 else '[%d, X, Y, Z]' % channels, v.shape))
            offsets.append(at)
            sizes.append(v.shape[-3:])
            flat.append(np.ascontiguousarray(v).astype(np_dtype).reshape(-1))      # numpy's cast: the reference's .astype(np.float16)
            at += v.size
        self.channels = channels
        self.sizes_host = np.asarray(sizes, dtype=np.int32).reshape(-1, 3)
        self.flat = torch.from_numpy(np.concatenate(flat)).to(device)
        self.offsets = torch.tensor(offsets, dtype=torch.int64).to(device)
        self.sizes = torch.from_numpy(self.sizes_host.copy()).to(device)
        self.is_f32 = int(dtype == torch.float32)


class SceneStore:
    """Scenes on the device.  ``targets`` (required), ``inputs``: one unpadded [X, Y, Z] array per scene; ``retrievals``: [K, X, Y, Z] per scene, the composed
    retrievals of ``formats.save_compose``; ``clouds``: [n, 3] float32 or float64 per scene, one dtype for the whole store, kept in that dtype (the reference
    multiplies a cloud in its own type).  ``dtype``: torch.float16 (the reference's preload cast) or torch.float32 for the volumes."""

    def __init__(self, names, targets, inputs=None, clouds=None, retrievals=None, device='cuda:0', dtype=torch.float16):
        if dtype not in (torch.float16, torch.float32):
            raise TypeError('SceneStore: dtype is torch.float16 or torch.float32, got %s' % dtype)
        self.names = list(names)
        if len(set(self.names)) != len(self.names) or not self.names:
            raise ValueError('SceneStore: scene names must be unique and there must be one')
        self.device, self.dtype = torch.device(device), dtype
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.index = {n: i for i, n in enumerate(self.names)}
        for what, field in (('targets', targets), ('inputs', inputs), ('clouds', clouds), ('retrievals', retrievals)):
            if field is not None and len(field) != len(self.names):
                raise ValueError('SceneStore: %d %s for %d scenes' % (len(field), what, len(self.names)))
        self.target = _Field(targets, 1, dtype, self.device, 'SceneStore: targets')
        self.input = None if inputs is None else _Field(inputs, 1, dtype, self.device, 'SceneStore: inputs')
        self.retrieval = None
        if retrievals is not None:
            self.retrieval = _Field(retrievals, int(np.asarray(retrievals[0]).shape[0]), dtype, self.device, 'SceneStore: retrievals')
            if not np.array_equal(self.retrieval.sizes_host, self.target.sizes_host):
                raise ValueError('SceneStore: a composed retrieval and its target differ in size')
        self.cloud = self.cloud_rows_host = None
        if clouds is not None:
            clouds = [np.asarray(c) for c in clouds]
            kinds = {c.dtype for c in clouds}
            if len(kinds) != 1 or kinds.pop() not in (np.dtype(np.float32), np.dtype(np.float64)):
                raise TypeError('SceneStore: clouds are all float32 or all float64')
            if any(c.ndim != 2 or c.shape[1] != 3 or c.shape[0] == 0 for c in clouds):
                raise ValueError('SceneStore: a cloud is a non-empty [n, 3] array')
            self.cloud_rows_host = np.array([c.shape[0] for c in clouds], dtype=np.int32)
            self.cloud = torch.from_numpy(np.concatenate(clouds)).to(self.device)
            self.cloud_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(self.cloud_rows_host[:-1])]).astype(np.int64)).to(self.device)
            self.cloud_rows = torch.from_numpy(self.cloud_rows_host.copy()).to(self.device)

    @classmethod
    def from_disk(cls, names, target_dir, input_dir=None, retrievals_dir=None, target_ext='.npz', input_ext='.npz', point_clouds=False, device='cuda:0',
                  dtype=torch.float16):
        """The reference's layout: ``<target_dir>/<scene><target_ext>`` and ``<input_dir>/<scene><input_ext>`` with key ``arr`` (``arr_0`` for point clouds,
        scene.py:60-64), ``<retrievals_dir>/compose/<scene>.npz`` with key ``arr_0`` (scene.py:74)."""
        def read(path, key):
            with np.load(path) as z:
                return z[key]
        names = list(names)
        targets = [read(Path(target_dir) / (s + target_ext), 'arr') for s in names]
        inputs = clouds = retrievals = None
        if input_dir is not None and point_clouds:
            clouds = [read(Path(input_dir) / (s + input_ext), 'arr_0') for s in names]
        elif input_dir is not None:
            inputs = [read(Path(input_dir) / (s + input_ext), 'arr') for s in names]
        if retrievals_dir is not None:
            retrievals = [read(Path(retrievals_dir) / 'compose' / (s + '.npz'), 'arr_0') for s in names]
        return cls(names, targets, inputs, clouds, retrievals, device, dtype)

    def size(self, scene):
        """the unpadded target size of a scene (the reference's ``scene_size``)"""
        return [int(v) for v in self.target.sizes_host[self.index[scene]]]


# ------------------------------------------------------------------------------------------------ launches
def _need_gpu(store, what):
    if store.device.type != 'cuda':
        raise RuntimeError('%s: the dataset kernels run on the GPU only (the store is on %s); there is no CPU fallback' % (what, store.device))


def check_items(items, sizes, window, pad, what):
    """Host check of items int [m, 4] = (scene, x0, y0, z0) against the unpadded ``sizes`` [n, 3]: every window lies in its padded scene."""
    items = np.asarray(items)
    if items.ndim != 2 or items.shape[1] != 4 or items.shape[0] == 0 or items.dtype.kind not in 'iu':
        raise ValueError('%s: items are a non-empty integer [m, 4] array of (scene, x0, y0, z0), got %s %s' % (what, items.dtype, items.shape))
    if (items[:, 0] < 0).any() or (items[:, 0] >= len(sizes)).any():
        raise ValueError('%s: a scene index outside [0, %d)' % (what, len(sizes)))
    hi = np.asarray(sizes)[items[:, 0]] + 2 * pad
    bad = np.nonzero(((items[:, 1:] < 0) | (items[:, 1:] + window > hi)).any(axis=1))[0]
    if len(bad):
        i = int(bad[0])
        raise ValueError('%s: the window of item %d (scene %d, start %s, %d^3) leaves the padded scene of %s' %
                         (what, i, int(items[i, 0]), tuple(int(v) for v in items[i, 1:]), window, tuple(int(v) for v in hi[i])))
    return np.ascontiguousarray(items, dtype=np.int32)


def _items(items, field_sizes, window, pad, store, what):
    """host items are checked, then uploaded; a device tensor is taken as it is (the kernels read nothing outside a scene whatever an item says)"""
    if isinstance(items, torch.Tensor) and items.is_cuda:
        if items.dtype != torch.int32 or items.dim() != 2 or items.shape[1] != 4 or items.shape[0] == 0:
            raise ValueError('%s: device items are a non-empty int32 [m, 4] tensor' % what)
        _need_gpu(store, what)
        return items.contiguous()
    checked = check_items(items.numpy() if isinstance(items, torch.Tensor) else items, field_sizes, window, pad, what)
    _need_gpu(store, what)
    return torch.from_numpy(checked).to(store.device)


@torch.no_grad()
def window_counts(store, items, window, pad, fill, threshold):
    """int32 [m] on the device: the voxels of each item's ``window``^3 of the TARGET store whose value is ``<= threshold`` (float32); outside the scene the
    ``fill`` decides.  One launch on the current stream."""
    if window < 1 or pad < 0:
        raise ValueError('window_counts: window %r, pad %r' % (window, pad))
    f = store.target
    it = _items(items, f.sizes_host, window, pad, store, 'window_counts')
    with _scoped(store.device):
        counts = torch.empty(it.shape[0], dtype=torch.int32, device=store.device)
        _lib.load_data().rf_data_occupancy(_p(f.flat), f.is_f32, _p(f.offsets), _p(f.sizes), len(store.names), _p(it), it.shape[0], window, pad, _f32(fill),
                                           _f32(threshold), _p(counts), _stream())
    return counts


@torch.no_grad()
def windows(store, field, items, window, pad, fill, mean=None, std=None):
    """float32 [m, C, w, w, w] on the device: the items' windows of ``field`` ('target', 'input' or 'retrieval'), ``(v - float32(mean)) / float32(std)`` when
    ``mean`` is given and the stored values themselves otherwise.  Host items are checked (a window leaving the padded scene raises before anything is
    launched); device items int32 [m, 4] are used as they are.  One launch on the current stream."""
    f = getattr(store, field, None) if field in ('target', 'input', 'retrieval') else None
    if f is None:
        raise ValueError('windows: the store holds no %r field' % (field,))
    if window < 1 or pad < 0 or (mean is None) != (std is None):
        raise ValueError('windows: window %r, pad %r, mean %r, std %r' % (window, pad, mean, std))
    it = _items(items, f.sizes_host, window, pad, store, 'windows')
    with _scoped(store.device):
        out = torch.empty((it.shape[0], f.channels, window, window, window), dtype=torch.float32, device=store.device)
        _lib.load_data().rf_data_gather(_p(f.flat), f.is_f32, _p(f.offsets), _p(f.sizes), len(store.names), f.channels, _p(it), it.shape[0], window, pad, _f32(fill),
                                        int(mean is not None), _f32(mean or 0.0), _f32(std if std is not None else 1.0), _p(out), _stream())
    return out


def _constant_windows(store, m, channels, window, value):
    """[m, channels, w^3] of one value, by the gather's no-normalise mode: items of scene -1 lie outside every scene and are written as the fill"""
    f = store.target
    it = torch.full((m * channels, 4), -1, dtype=torch.int32, device=store.device)
    out = torch.empty((m, channels, window, window, window), dtype=torch.float32, device=store.device)
    _lib.load_data().rf_data_gather(_p(f.flat), f.is_f32, _p(f.offsets), _p(f.sizes), len(store.names), 1, _p(it), m * channels, window, 0, _f32(value), 0, 0.0, 1.0,
                                    _p(out), _stream())
    return out


def check_table(table, cloud_rows, what='register_table'):
    """The reference's ``random_indices`` [R, P] against the clouds it will index: an index at or above a cloud's length (twice its length below 20000
    rows) would be an IndexError in ``pc[pt_indices, :]`` (scene.py:89).  Host only, from the table's extrema."""
    table = np.asarray(table)
    if table.ndim != 2 or table.size == 0 or table.dtype not in _TABLE_KINDS:
        raise TypeError('%s: the index table is a non-empty [R, P] array of uint16, int32 or int64, got %s %s' % (what, table.dtype, table.shape))
    limit = int(min(2 * n if n < DOUBLED_BELOW else n for n in (int(v) for v in cloud_rows)))
    lo, hi = int(table.min()), int(table.max())
    if lo < 0 or hi >= limit:
        raise ValueError('%s: table index out of range: the table spans [%d, %d] but the shortest cloud has %d readable rows' % (what, lo, hi, limit))
    return np.ascontiguousarray(table)


@torch.no_grad()
def point_windows(store, table, items, rows, window, grid_res, pad, scale, mean=None, std=None):
    """float32 [m, 1, w, w, w] on the device: for item i the window of ``point_cloud_to_grid(pc[table[rows[i]]], grid_res, scale, pad)`` (util/misc.py:73-78,
    scene.py:81-90), zeros and ones, normalised when ``mean`` is given.  ``table``: a device tensor [R, P] registered through ``check_table``; ``rows`` int32
    [m] on the device.  A point with a NaN coordinate sets no voxel (the reference's cast of NaN to uint32 has no defined result); +-inf clips to the grid's
    faces like any other value.  Two launches on the current stream."""
    if store.cloud is None:
        raise ValueError('point_windows: the store holds no point clouds')
    f64 = store.cloud.dtype == torch.float64
    if f64 and float(np.float32(scale)) != float(scale):
        raise ValueError('point_windows: scale %r is not a float32 value, which float64 clouds need (the ABI carries no double scalar)' % (scale,))
    kind = {torch.uint16: 0, torch.int32: 1, torch.int64: 2}[table.dtype]
    grid_sizes = np.full((len(store.names), 3), grid_res, dtype=np.int64)
    it = _items(items, grid_sizes, window, pad, store, 'point_windows')
    with _scoped(store.device):
        if rows.dtype != torch.int32 or rows.shape != (it.shape[0],) or not rows.is_cuda:
            raise ValueError('point_windows: rows are an int32 [m] device tensor')
        out = torch.empty((it.shape[0], 1, window, window, window), dtype=torch.float32, device=store.device)
        _lib.load_data().rf_data_points(_p(store.cloud), int(f64), _p(store.cloud_offsets), _p(store.cloud_rows), len(store.names), _p(table), kind, table.shape[0],
                                        table.shape[1], _p(it), _p(rows.contiguous()), it.shape[0], window, grid_res, pad, _f32(scale), int(mean is not None),
                                        _f32(mean or 0.0), _f32(std if std is not None else 1.0), _p(out), _stream())
    return out


# ------------------------------------------------------------------------------------------------ occupancy
def patch_table(store, geometry, scenes=None):
    """Host: every patch of ``scenes`` (default: all of the store) in the reference's order -> (scene index in the store int32 [P], input extents [P, 6], target
    extents [P, 6])."""
    g = _geometry(geometry)
    scenes = store.names if scenes is None else list(scenes)
    idx, e_in, e_tgt = [], [], []
    for s in scenes:
        if s not in store.index:
            raise KeyError('scene %r is not in the store' % (s,))
        a, b = patch_extents(store.size(s), g)
        idx.append(np.full(len(b), store.index[s], dtype=np.int32))
        e_in.append(a)
        e_tgt.append(b)
    return np.concatenate(idx), np.concatenate(e_in).astype(np.int32), np.concatenate(e_tgt).astype(np.int32)


def patch_names(store, geometry, scenes=None):
    idx, _, e_tgt = patch_table(store, geometry, scenes)
    return [patch_name(store.names[i], e) for i, e in zip(idx, e_tgt)]


def patch_occupancy(store, geometry, scenes=None):
    """``SceneHandler.calculate_occupancy_for_name`` (scene.py:148-150) for every patch of ``patch_table``'s order: int32 [P] on the device, the voxels of the
    padded target window with ``value <= 0.75 * 2 * target_voxel_size``.  The padding is compared like any voxel (the truncation is never occupied, but it is
    the comparison that says so)."""
    g = _geometry(geometry)
    idx, _, e_tgt = patch_table(store, g, scenes)
    items = np.concatenate([idx[:, None], e_tgt[:, 0::2]], axis=1)
    return window_counts(store, items, g.window_target, g.context_target, g.target_trunc, g.threshold)


def occupancy_path(data_dir, dataset_config):
    d = dataset_config
    return Path(data_dir) / 'occupancy' / ('%s_%03d_%02d_%02d.json' % (d['dataset_name'], d['target_chunk_size'], d['patch_size_target'], d['patch_context_target']))


def occupancy_json(path, store, dataset_config, scenes=None, counts=None):
    """Writes the reference's occupancy file (patch name -> int, scene.py:139-146) for the scenes' patches and returns the mapping.  ``counts``: the result of
    ``patch_occupancy`` for the same scenes, or None to compute it."""
    names = patch_names(store, dataset_config, scenes)
    counts = patch_occupancy(store, dataset_config, scenes) if counts is None else counts
    values = [int(v) for v in (counts.cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts))]
    if len(values) != len(names):
        raise ValueError('occupancy_json: %d counts for %d patches' % (len(values), len(names)))
    mapping = dict(zip(names, values))
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(mapping))
    return mapping


def read_occupancy(path):
    return {k: int(v) for k, v in json.loads(Path(path).read_text()).items()}


# ------------------------------------------------------------------------------------------------ the dataset
class PatchDataset:
    """``PatchedSceneDataset(split, dataset_config, scene_handler)`` over a ``SceneStore``.

    ``scenes``: the split's scene list (default: the store's); ``task``: 'surface_reconstruction' reads point clouds through ``table`` (the reference's
    ``random_indices`` [R, num_points], uint16 / int32 / int64), anything else reads the input volumes (default: by what the store holds);
    ``no_retrievals``: the reference's flag (default: the store holds none); ``occupancy``: a mapping patch name -> count to use instead of counting (the
    reference's JSON; a patch it does not name counts 1, as ``get_patch_occupancy`` has it)."""

    def __init__(self, store, dataset_config, split, scenes=None, task=None, no_retrievals=None, table=None, occupancy=None):
        d = self.config = dict(dataset_config)
        g = self.geometry = Geometry(d)
        self.store, self.split = store, split
        self.scenes = list(store.names if scenes is None else scenes)
        self.point_clouds = (store.cloud is not None and store.input is None) if task is None else task == 'surface_reconstruction'
        self.no_retrievals = (store.retrieval is None) if no_retrievals is None else bool(no_retrievals)
        if not self.no_retrievals and store.retrieval is None:
            raise ValueError('PatchDataset: retrievals are asked for but the store holds none')
        if self.point_clouds and (store.cloud is None or table is None):
            raise ValueError('PatchDataset: the point-cloud task needs clouds in the store and the index table')
        if not self.point_clouds and store.input is None:
            raise ValueError('PatchDataset: the store holds no inputs')
        idx, e_in, e_tgt = patch_table(store, g, self.scenes)
        self._patch_scene, self._patch_extent_tgt = idx, e_tgt
        # every window lies in its padded scene: refused here, before any launch
        check_items(np.concatenate([idx[:, None], e_tgt[:, 0::2]], axis=1), store.target.sizes_host, g.window_target, g.context_target, 'PatchDataset: target')
        if self.point_clouds:
            self.grid_res = int(d['input_chunk_size'])
            check_items(np.concatenate([idx[:, None], e_in[:, 0::2]], axis=1), np.full((len(store.names), 3), self.grid_res), g.window_input, g.context_input,
                        'PatchDataset: input grid')
            rows_of = store.cloud_rows_host[[store.index[s] for s in self.scenes]]
            table = check_table(table, rows_of, 'PatchDataset')
            if table.shape[1] != int(d.get('num_points', table.shape[1])):
                raise ValueError('PatchDataset: the table has %d indices per row, num_points is %d' % (table.shape[1], d['num_points']))
            self.table = torch.from_numpy(table).to(store.device)
        else:
            sizes_in = np.array([g.input_size(store.size(s)) for s in store.names])
            if not np.array_equal(sizes_in, store.input.sizes_host):
                raise ValueError('PatchDataset: an input volume is not int(target size / %g) in size' % g.scale_factor)
            check_items(np.concatenate([idx[:, None], e_in[:, 0::2]], axis=1), store.input.sizes_host, g.window_input, g.context_input, 'PatchDataset: input')
        if occupancy is None:
            counts = patch_occupancy(store, g, self.scenes).cpu().numpy()
        else:
            counts = np.array([int(occupancy.get(patch_name(store.names[i], e), 1)) for i, e in zip(idx, e_tgt)], dtype=np.int32)
        self.patch_counts = counts
        keep = np.nonzero(counts > d['occupancy_threshold'])[0]
        self._kept = keep
        if split == 'train':
            keep = np.tile(keep, int(d['train_multiplier']))
        self.item_scene, self.extent_input, self.extent_target = idx[keep], e_in[keep], e_tgt[keep]
        pos = {s: i for i, s in reversed(list(enumerate(self.scenes)))}            # list.index: the first occurrence
        self._scene_pos = pos
        split_index = np.array([pos[store.names[i]] for i in self.item_scene], dtype=np.int64)
        dev = store.device
        self._items_in = torch.from_numpy(np.ascontiguousarray(np.concatenate([self.item_scene[:, None], self.extent_input[:, 0::2]], axis=1), dtype=np.int32)).to(dev)
        self._items_tgt = torch.from_numpy(np.ascontiguousarray(np.concatenate([self.item_scene[:, None], self.extent_target[:, 0::2]], axis=1), dtype=np.int32)).to(dev)
        self._extent = torch.from_numpy(np.ascontiguousarray(self.extent_target, dtype=np.int32)).to(dev)
        self._scene_index = torch.from_numpy(split_index).to(dev)
        self._lookup = None

    def __len__(self):
        return len(self.item_scene)

    def names(self, idx=None):
        """patch names of the items ``idx`` (host indices; default all), built when asked for"""
        idx = range(len(self)) if idx is None else [int(i) for i in idx]
        return [patch_name(self.store.names[self.item_scene[i]], self.extent_target[i]) for i in idx]

    def get_scene_indices(self, scenes):
        return np.array([self.scenes.index(s) for s in scenes])

    @property
    def patch_from_scene_lookup(self):
        """scene -> names of its kept patches, before the train multiplier (patched_scene_dataset.py:30-32)"""
        if self._lookup is None:
            self._lookup = {}
            for p in self._kept:
                s = self.store.names[self._patch_scene[p]]
                self._lookup.setdefault(s, []).append(patch_name(s, self._patch_extent_tgt[p]))
        return self._lookup

    def patch_mask(self, chunk_names):
        """bool [n, P]: which of the P patches of each scene chunk are dataset items, in the enumeration order -- the ``patch_mask`` of ``engine.refine``,
        ``build_database_rows``, ``formats.retrieval_mapping`` and the ``splits`` of ``formats.retrievals_to_disk`` ([n, 64] for 64^3 chunks)."""
        rows = []
        for s in chunk_names:
            if s not in self._scene_pos:
                raise KeyError('patch_mask: scene %r is not in this split' % (s,))
            sel = self._patch_scene == self.store.index[s]
            rows.append(self.patch_counts[sel] > self.config['occupancy_threshold'])
        if len({len(r) for r in rows}) > 1:
            raise ValueError('patch_mask: the scenes do not all have the same number of patches')
        return np.stack(rows)

    def _index(self, idx):
        if isinstance(idx, torch.Tensor) and idx.is_cuda:
            if idx.dim() != 1 or idx.numel() == 0 or idx.dtype not in (torch.int64, torch.int32):
                raise ValueError('PatchDataset.batch: device indices are a non-empty int64 [B] tensor')
            return idx.to(torch.int64)
        host = np.asarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx)
        if host.ndim != 1 or host.size == 0 or host.dtype.kind not in 'iu' or host.min() < 0 or host.max() >= len(self):
            raise IndexError('PatchDataset.batch: indices are a non-empty integer [B] sequence in [0, %d)' % len(self))
        return torch.from_numpy(host.astype(np.int64)).to(self.store.device)

    @torch.no_grad()
    def batch(self, idx, rows=None, generator=None):
        """The reference's collated batch for the items ``idx`` (a device int64 tensor, used as it is, or a host sequence, checked), as device tensors:
        ``input`` float32 [B, 1, wi, wi, wi], ``target`` float32 [B, 1, wt, wt, wt], ``retrieval`` float32 [B, K, wt, wt, wt] (without retrievals: four
        channels of the truncation, not normalised), ``extent`` int32 [B, 6], ``scene_index`` int64 [B] (position in ``scenes``).  ``rows``: for point clouds,
        the row of the index table each item samples with (the reference's ``random.randint``; int [B], host or device); None draws them from ``generator``
        (a device generator) on the device.  Nothing here waits for the host when ``idx`` and ``rows`` are device tensors."""
        store, g, d = self.store, self.geometry, self.config
        _need_gpu(store, 'PatchDataset.batch')
        with _scoped(store.device):
            idx = self._index(idx)
            b = idx.shape[0]
            if self.point_clouds and rows is None:
                rows = torch.randint(0, self.table.shape[0], (b,), device=store.device, generator=generator, dtype=torch.int32)
            elif self.point_clouds and not (isinstance(rows, torch.Tensor) and rows.is_cuda):
                host = np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows)
                if host.shape != (b,) or host.dtype.kind not in 'iu' or host.min() < 0 or host.max() >= self.table.shape[0]:
                    raise IndexError('PatchDataset.batch: rows are %d table rows in [0, %d)' % (b, self.table.shape[0]))
                rows = torch.from_numpy(host.astype(np.int32)).to(store.device)
            items_tgt = self._items_tgt.index_select(0, idx)
            out = {'target': windows(store, 'target', items_tgt, g.window_target, g.context_target, g.target_trunc, d['target_mean'], d['target_std'])}
            if self.point_clouds:
                out['input'] = point_windows(store, self.table, self._items_in.index_select(0, idx), rows.to(torch.int32), g.window_input, self.grid_res,
                                             g.context_input, 1 / g.scale_factor, d['input_mean'], d['input_std'])
            else:
                out['input'] = windows(store, 'input', self._items_in.index_select(0, idx), g.window_input, g.context_input, g.input_trunc, d['input_mean'],
                                       d['input_std'])
            if self.no_retrievals:
                out['retrieval'] = _constant_windows(store, b, 4, g.window_target, g.target_trunc)       # patched_scene_dataset.py:135-136
            else:
                out['retrieval'] = windows(store, 'retrieval', items_tgt, g.window_target, g.context_target, g.target_trunc, d['target_mean'], d['target_std'])
            out['extent'] = self._extent.index_select(0, idx)
            out['scene_index'] = self._scene_index.index_select(0, idx)
        return out

    def use_subset(self, subset):
        """``PatchedSceneDataset.use_subset``: the items become the patches named in ``subset``, in that order; the input extents are the target extents
        divided by the scale factor (patched_scene_dataset.py:36-41).  A name whose window leaves its padded scene is refused."""
        g = self.geometry
        parsed = [parse_patch_name(n) for n in subset]
        scene = np.array([self.store.index[s] for s, _ in parsed], dtype=np.int32)
        e_tgt = np.array([e for _, e in parsed], dtype=np.int32).reshape(-1, 6)
        e_in = np.array([[int(v // g.scale_factor) for v in e] for _, e in parsed], dtype=np.int32).reshape(-1, 6)
        if ((e_tgt[:, 1::2] - e_tgt[:, 0::2]) != g.window_target).any() or ((e_in[:, 1::2] - e_in[:, 0::2]) != g.window_input).any():
            raise ValueError('use_subset: a named patch is not a %d^3 (input %d^3) window' % (g.window_target, g.window_input))
        check_items(np.concatenate([scene[:, None], e_tgt[:, 0::2]], axis=1), self.store.target.sizes_host, g.window_target, g.context_target, 'use_subset: target')
        in_sizes = np.full((len(self.store.names), 3), self.grid_res) if self.point_clouds else self.store.input.sizes_host
        check_items(np.concatenate([scene[:, None], e_in[:, 0::2]], axis=1), in_sizes, g.window_input, g.context_input, 'use_subset: input')
        self.__dict__.update(_subset_state(self, scene, e_in, e_tgt))


def _subset_state(ds, scene, e_in, e_tgt):
    dev = ds.store.device
    up = lambda a, t=np.int32: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(dev)
    return {'item_scene': scene, 'extent_input': e_in, 'extent_target': e_tgt,
            '_items_in': up(np.concatenate([scene[:, None], e_in[:, 0::2]], axis=1)), '_items_tgt': up(np.concatenate([scene[:, None], e_tgt[:, 0::2]], axis=1)),
            '_extent': up(e_tgt), '_scene_index': up(np.array([ds._scene_pos[ds.store.names[i]] for i in scene]), np.int64)}


class BatchLoader:
    """``DataLoader(dataset, batch_size, shuffle, drop_last)`` for a ``PatchDataset``: iterating yields the device batches of one epoch.  The permutation
    (``shuffle``) and the point-cloud rows are drawn on the device from ``generator`` (a ``torch.Generator`` of the store's device; default: a new one seeded from
    ``torch.initial_seed()``); nothing in an epoch waits for the host."""

    def __init__(self, dataset, batch_size, shuffle=False, drop_last=False, generator=None):
        if batch_size < 1:
            raise ValueError('BatchLoader: batch_size %r' % (batch_size,))
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), bool(shuffle), bool(drop_last)
        dev = dataset.store.device
        _need_gpu(dataset.store, 'BatchLoader')
        if generator is None:
            generator = torch.Generator(device=dev)
            generator.manual_seed(torch.initial_seed())
        if generator.device != dev:
            raise ValueError('BatchLoader: the generator lives on %s, the store on %s' % (generator.device, dev))
        self.generator = generator
        self._order = torch.arange(len(dataset), dtype=torch.int64, device=dev)

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def order(self):
        """the epoch's item order, int64 [N] on the device: a uniform permutation as the argsort of N uniform draws"""
        if not self.shuffle:
            return self._order
        return torch.argsort(torch.rand(len(self.dataset), device=self._order.device, generator=self.generator))

    def __iter__(self):
        order, n, b = self.order(), len(self.dataset), self.batch_size
        for lo in range(0, n - b + 1 if self.drop_last else n, b):
            yield self.dataset.batch(order[lo:min(lo + b, n)], generator=self.generator)
