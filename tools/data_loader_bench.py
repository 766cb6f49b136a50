"""Dev tool (GPU box): milliseconds per batch of ``rfuse.data.BatchLoader`` at the trainers' geometries, beside the host path it replaces and the step times it
has to keep up with.

    python tools/data_loader_bench.py [--epochs 9] [--scenes 128] [--out profiles/data_loader_bench.txt]

Rows:
  C2 retrieval    distance-field inputs 4^3, targets 32^3 (patch 2 + 1 / 16 + 8), ``no_retrievals``, B = 512 and B = 128
  C5 retrieval    point-cloud windows 48^3 of a 128^3 grid (patch 32 + 8), 1000 points per item, targets 24^3 (16 + 4), ``no_retrievals``, B = 512 and B = 128
  C2 refinement   whole chunks: input 8^3, target 64^3, K = 4 composed retrievals, B = 8
  C5 refinement   the whole 128^3 grid, 500 points, target 64^3, K = 4 composed retrievals, B = 8
on ``--scenes`` synthetic 64^3 scenes (spherical shells, float16 store, ShapeNetV2 constants).  Every item of an epoch is drawn: the permutation, the index
selects, the point-cloud rows and all launches are in the figure.

Per row: whole shuffled epochs of the loader back to back between two HIP events (as many as fill a quarter of a second), divided by their number of
batches -- the device time a trainer would wait for if it did nothing else; median (p10 .. p90) of ``--epochs`` such runs after a warm-up epoch, and the
host's wall time per batch for enqueueing it (no synchronise inside a run).  Beside it ``tests/dataset_ref.py`` (the numpy restatement of the reference's
``__getitem__``) run single-process on this host for 48 items, scaled to the batch, plus the pinned host-to-device copy of one collated batch (HIP events).
Then the step times recorded in profiles/retrieval_train_C2.txt / _C5.txt (their own batch size) and the ratio loader / step for the same number of items.
A measurement needs the GPU: without one the tool stops."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / 'retrieval-fuse_amd'))
sys.path.insert(0, str(REPO / 'tests'))
import dataset_ref as dr                                                      # noqa: E402
from rfuse import configs                                                      # noqa: E402
from rfuse.data import BatchLoader, PatchDataset, SceneStore, patch_names     # noqa: E402

DEV = torch.device('cuda:0')


def section(cfg_name, **geometry):
    d = dict(configs.get_config(cfg_name)['dataset_train'])
    d.update(occupancy_threshold=0, train_multiplier=1, patch_stride=geometry['patch_size_target'], **geometry)
    return d


CASES = [
    ('C2 retrieval', 'C2', dict(patch_size_input=2, patch_context_input=1, patch_size_target=16, patch_context_target=8), False, (512, 128), 0),
    ('C5 retrieval', 'C5', dict(patch_size_input=32, patch_context_input=8, patch_size_target=16, patch_context_target=4, num_points=1000), True, (512, 128), 0),
    ('C2 refinement', 'C2', dict(patch_size_input=8, patch_context_input=0, patch_size_target=64, patch_context_target=0), False, (8,), 4),
    ('C5 refinement', 'C5', dict(patch_size_input=128, patch_context_input=0, patch_size_target=64, patch_context_target=0), True, (8,), 4),
]


def scenes(n, rng, voxel, with_inputs, with_clouds, k):
    ax = np.arange(64, dtype=np.float32)
    x = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1)
    out = []
    for _ in range(n):
        centre, radius = rng.uniform(20, 44, 3).astype(np.float32), np.float32(rng.uniform(8, 26))
        target = np.minimum(np.abs(np.linalg.norm(x - centre, axis=-1) - radius) * np.float32(voxel), np.float32(3 * voxel)).astype(np.float16)
        s = {'target': target}
        if with_inputs:
            s['input'] = target.astype(np.float32).reshape(8, 8, 8, 8, 8, 8).mean(axis=(1, 3, 5)).astype(np.float16)
        if with_clouds:
            d = rng.normal(size=(20000, 3))
            s['cloud'] = (centre + d / np.linalg.norm(d, axis=1, keepdims=True) * radius).astype(np.float32)
        if k:
            s['retrieval'] = np.stack([np.roll(target, 3 * (j + 1), axis=j % 3) for j in range(k)])
        out.append(s)
    return out


def epoch_ms(loader, runs, min_seconds=0.25):
    """one timed run = as many whole epochs back to back as fill ``min_seconds`` (an epoch of a few batches alone would measure the clock)"""
    def one(inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(inner):
            for batch in loader:
                pass
        e1.record()
        host = time.perf_counter() - t0
        e1.synchronize()
        return e0.elapsed_time(e1) / (inner * len(loader)), host * 1e3 / (inner * len(loader))
    one(1)                                                                     # warm-up: every shape of the epoch, the tail batch included
    inner = max(1, int(np.ceil(min_seconds * 1e3 / (one(1)[0] * len(loader)))))
    timed = sorted(one(inner) for _ in range(runs))
    dev = [r[0] for r in timed]
    return statistics.median(dev), dev[len(dev) // 10], dev[len(dev) * 9 // 10], statistics.median(r[1] for r in timed), inner


def host_path(d, task, no_retr, names, fields, table, occupancy, batch, items=48):
    """tests/dataset_ref.py single-process: ms per batch (from ``items`` items), and the pinned copy of one collated batch"""
    ref = dr.RefDataset(d, task, no_retr, 'val', names, dict(zip(names, fields)), table, np.float16, occupancy)
    rng = np.random.default_rng(1)
    pick = rng.integers(0, len(ref), items)
    rows = rng.integers(0, len(table), items) if table is not None else [None] * items
    t0 = time.perf_counter()
    got = [ref.item(int(i), None if r is None else int(r)) for i, r in zip(pick, rows)]
    per_item = (time.perf_counter() - t0) / items
    pinned = [torch.from_numpy(np.repeat(got[0][k][None], batch, axis=0).astype(np.float32)).pin_memory() for k in ('input', 'target', 'retrieval')]
    copies = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev = [p.to(DEV, non_blocking=True) for p in pinned]
        e1.record()
        e1.synchronize()
        copies.append(e0.elapsed_time(e1))
        del dev
    return per_item * batch * 1e3, statistics.median(copies[2:])


def step_record(name):
    path = REPO / 'profiles' / ('retrieval_train_%s.txt' % name)
    rec = json.loads(path.read_text().strip().splitlines()[-1])
    return rec['ms_per_step'], rec['batch']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=9)
    ap.add_argument('--scenes', type=int, default=128)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'data_loader_bench.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('data_loader_bench: needs the GPU; nothing is measured without one')
    lines = ['device-resident patch dataset (rfuse.data.BatchLoader, csrc/dataset.hip), %s, %d synthetic 64^3 scenes, float16 store' % (torch.cuda.get_device_name(0), args.scenes),
             'device ms per batch = whole shuffled epochs back to back between two HIP events (>= 0.25 s) / their batches, median (p10 .. p90) of %d runs after a warm-up '
             'epoch; host = wall time per batch to enqueue it' % args.epochs,
             'numpy = tests/dataset_ref.py single-process on this host, ms per batch from 48 items; h2d = pinned copy of one collated batch (HIP events)']
    steps = {}
    for name in ('C2', 'C5'):
        steps[name] = step_record(name)
        lines.append('recorded step of profiles/retrieval_train_%s.txt: %.3f ms at batch %d' % (name, steps[name][0], steps[name][1]))
    for label, cfg_name, geometry, clouds, batches, k in CASES:
        d = section(cfg_name, **geometry)
        rng = np.random.default_rng(7)
        made = scenes(args.scenes, rng, d['voxel_size_target'], not clouds, clouds, k)
        names = ['s%04d' % i for i in range(args.scenes)]
        store = SceneStore(names, [s['target'] for s in made], None if clouds else [s['input'] for s in made], [s['cloud'] for s in made] if clouds else None,
                           [s['retrieval'] for s in made] if k else None, device=DEV)
        table = np.stack([rng.choice(20000, d['num_points'], replace=False) for _ in range(2048)]).astype(np.int64) if clouds else None
        task = 'surface_reconstruction' if clouds else 'superresolution'
        ds = PatchDataset(store, d, 'val', task=task, no_retrievals=not k, table=table)
        occupancy = dict(zip(patch_names(store, d), (int(v) for v in ds.patch_counts)))
        g = ds.geometry
        for b in batches:
            gen = torch.Generator(device=DEV)
            gen.manual_seed(5)
            loader = BatchLoader(ds, b, shuffle=True, generator=gen)
            med, lo, hi, host, inner = epoch_ms(loader, args.epochs)
            numpy_ms, h2d = host_path(d, task, not k, names, made, table, occupancy, b)
            out_mb = b * (g.window_input ** 3 + (1 + 4) * g.window_target ** 3) * 4 / 1e6
            line = ('%-14s B = %3d  input %3d^3 target %2d^3 retrieval 4 x %2d^3 (%6.1f MB written)  %5d items, %3d batches x %3d epochs   device %8.3f (%7.3f .. %7.3f) ms   host %7.3f ms   '
                    'numpy %9.1f ms + h2d %7.3f ms   numpy / device = %7.0f' %
                    (label, b, g.window_input, g.window_target, g.window_target, out_mb, len(ds), len(loader), inner, med, lo, hi, host, numpy_ms, h2d, (numpy_ms + h2d) / med))
            if label.endswith('retrieval'):
                step_ms, step_b = steps[cfg_name]
                line += '   step %.3f ms per %d items -> loader / step for the same items = %.4f' % (step_ms, step_b, med * step_b / b / step_ms)
            print(line, flush=True)
            lines.append(line)
        del store, ds
        torch.cuda.empty_cache()
    Path(args.out).write_text('\n'.join(lines) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
