"""Fixture generator for the shape loss (CPU; needs the reference checkout, as tools/gen_mesh_metrics_golden.py does): runs the reference's own
``RefinementTrainingModule.augment_batch_data`` / ``loss_shape`` (trainer/train_refinement.py:175-183, :231-253) and
``PatchedSceneDataset.compute_normals`` (dataset/patched_scene_dataset.py:139-146) as written, in float32 and again in float64, and writes
tests/golden/shape_loss.npz (arrays only).

    python tools/gen_shape_loss_golden.py

``pytorch_lightning`` is stood in for through ``sys.modules`` (``LightningModule = torch.nn.Module``); the methods are called unbound on
``types.SimpleNamespace`` stand-ins that carry the attributes they touch.  For the float64 run the inputs and the Sobel stencils are cast to double.

Inputs per case: raw target ``| |x| - r | * 4 trunc`` on a ``linspace(-1, 1)`` grid, clamped at trunc and rounded through float16, r per sample in
[0.45, 0.75]; ``target`` = the raw target normalised (float32); ``pred = clamp(2 raw / trunc - 1 + 0.3 randn, -1, 1)``
with the noise zeroed on the first third of the last axis (flat regions are then exactly flat: pred = 1, df(pred) = trunc = the padding value).
The mean / std are ``STATS`` below (why: there).

Layout of tests/golden/shape_loss.npz: ``cases`` (names), ``<case>_params`` float64 [6] = trunc, mean, std, weight_occupied, loss_reconstruction,
loss_normal; ``<case>_target`` / ``_pred`` float32 [B,1,D,H,W]; per precision p in (f32, f64): ``_weights_p``, ``_empty`` (bool, the same in both),
``_normals_p`` [B,3,D,H,W], ``_scalars_p`` [3] = total, l1, normal, ``_grad_p`` = pred.grad of total.backward(); ``_counts`` int64 [2] = valid voxels
(both Sobel gradients non-zero), voxels empty in target and prediction.
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
from oracle import gen_golden                          # noqa: E402
from oracle.gen_golden import REF, save_fixture        # noqa: E402
from rfuse import configs as rf_configs                # noqa: E402

SHAPENET, MATTERPORT = 'C1', 'C4'
#        name      shape             config      seed  flat
CASES = [('sn16', (2, 1, 16, 16, 16), SHAPENET, 5, False),
         ('odd', (1, 1, 9, 17, 33), SHAPENET, 5, False),
         ('mp16', (2, 1, 16, 16, 16), MATTERPORT, 5, False),
         ('tiny', (3, 1, 2, 3, 5), SHAPENET, 5, False),
         ('flat4', (1, 1, 4, 4, 4), SHAPENET, 5, True),
         ('flat1', (1, 1, 1, 1, 1), SHAPENET, 5, True)]
# target mean / std: the datasets' (rfuse.configs) rounded to a few bits, the std to a power of two.  With the datasets' own digits den(T) = T * std + mean of
# a flat (truncated) region is a constant with a full mantissa, float32's in one run and float64's in the other; the reference's float64 convolution then returns
# rounding noise of the order 1e-17 where the Sobel gradient is mathematically 0, the voxel counts as valid, and the float64 'truth' averages the cosine of noise.
# With these values den(T) of a flat region is trunc itself in both precisions, and the float32 and float64 runs see the same masks.
STATS = {SHAPENET: (15 / 256, 2.0 ** -7), MATTERPORT: (10.5, 2.0)}
CHECKED = ('sn16', 'odd', 'mp16')           # the non-degenerate cases whose masks and valid share are asserted


def import_reference_trainer():
    pl = types.ModuleType('pytorch_lightning')
    pl.LightningModule = torch.nn.Module
    sys.modules['pytorch_lightning'] = pl
    gen_golden.import_reference_util_retrieval()
    for k in [k for k in sys.modules if k in ('model', 'trainer') or k.startswith('model.') or k.startswith('trainer.')]:
        del sys.modules[k]
    import trainer.train_refinement as tr
    from dataset.patched_scene_dataset import PatchedSceneDataset
    assert str(REF) in tr.__file__, tr.__file__
    return tr.RefinementTrainingModule, PatchedSceneDataset


def make_inputs(shape, trunc, mean, std, seed, flat):
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


def run_reference(Module, Dataset, target, pred, trunc, mean, std, hp, dtype):
    ds = types.SimpleNamespace(scene_handler=types.SimpleNamespace(target_trunc=np.float32(trunc)), target_mean=mean, target_std=std,
                               sobel_3d_x=Dataset.sobel_3d_x.to(dtype), sobel_3d_y=Dataset.sobel_3d_y.to(dtype), sobel_3d_z=Dataset.sobel_3d_z.to(dtype))
    ds.compute_normals = types.MethodType(Dataset.compute_normals, ds)
    ds.denormalize_target = types.MethodType(Dataset.denormalize_target, ds)
    mod = types.SimpleNamespace(train_dataset=ds, scene_handlers={'train': types.SimpleNamespace(target_trunc=np.float32(trunc))}, hparams=hp,
                                adjust_weights=Module.adjust_weights)
    for name in ('network_pred_to_df', 'normalized_target_to_network_pred'):
        setattr(mod, name, types.MethodType(getattr(Module, name), mod))
    batch = {'target': torch.from_numpy(target).to(dtype)}
    Module.augment_batch_data(mod, batch)
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    total, l1, normal = Module.loss_shape(mod, p, batch)
    total.sum().backward()
    with torch.no_grad():
        df = mod.network_pred_to_df(p)
        pred_empty = df >= np.float32(trunc)
        n_p = ds.compute_normals(df).permute(0, 2, 3, 4, 1).reshape(-1, 3)
        n_t = batch['normals'].permute(0, 2, 3, 4, 1).reshape(-1, 3)
        valid = (torch.norm(n_p, dim=1) != 0) & (torch.norm(n_t, dim=1) != 0)
    return {'weights': batch['weights'].numpy(), 'empty': batch['empty'].numpy(), 'normals': batch['normals'].numpy(),
            'scalars': np.array([float(total.sum()), float(l1.sum()), float(normal.sum())], np.float64).astype(batch['weights'].numpy().dtype),
            'grad': p.grad.numpy(), 'valid': valid.numpy(), 'pred_empty': pred_empty.numpy()}


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def main():
    Module, Dataset = import_reference_trainer()
    out = {'cases': np.array([c[0] for c in CASES])}
    for name, shape, cfg_name, seed, flat in CASES:
        cfg = rf_configs.get_config(cfg_name)
        d = cfg['dataset_train']
        trunc = rf_configs.truncations(cfg)[1]
        mean, std = STATS[cfg_name]
        assert abs(mean - d['target_mean']) < 0.05 * d['target_mean'] and 0.7 < std / d['target_std'] < 1.0
        hp = {'weight_occupied': 8, 'loss_reconstruction': 1, 'loss_normal': 0.5}
        target, pred = make_inputs(shape, trunc, mean, std, seed, flat)
        r32 = run_reference(Module, Dataset, target, pred, trunc, mean, std, hp, torch.float32)
        r64 = run_reference(Module, Dataset, target, pred, trunc, mean, std, hp, torch.float64)
        n = int(np.prod(shape))
        both_empty = r32['empty'] & r32['pred_empty']
        diff = int((r32['valid'] != r64['valid']).sum() + (r32['pred_empty'] != r64['pred_empty']).sum() + (r32['empty'] != r64['empty']).sum()
                   + ((r32['normals'] == 0) != (r64['normals'] == 0)).sum())
        print('%-6s %-18s valid %d / %d, empty on both sides %d, mask differences fp32 vs float64 %d' % (name, shape, r32['valid'].sum(), n, both_empty.sum(), diff))
        if name in CHECKED:
            assert diff == 0, 'case %s: the float32 and float64 runs disagree on %d mask entries -- change its seed' % (name, diff)
            assert 0.3 <= r32['valid'].mean() <= 0.8, 'case %s: %.1f %% valid voxels -- change its seed' % (name, 100 * r32['valid'].mean())
        if flat:
            assert r32['valid'].sum() == 0 and np.isnan(r32['scalars'][[0, 2]]).all() and np.isfinite(r32['grad']).all()
        else:
            print('       err_ref: total %.3e  l1 %.3e  normal %.3e (relative);  grad %.3e  normals %.3e (max-abs / max|f64|)' % (
                *(abs(float(r32['scalars'][k]) - r64['scalars'][k]) / abs(r64['scalars'][k]) for k in range(3)), rel(r32['grad'], r64['grad']),
                rel(r32['normals'], r64['normals'])))
        assert np.array_equal(r32['weights'], r64['weights'].astype(np.float32)) and np.array_equal(r32['empty'], r64['empty'])
        out[name + '_params'] = np.array([trunc, mean, std, hp['weight_occupied'], hp['loss_reconstruction'], hp['loss_normal']], np.float64)
        out[name + '_target'], out[name + '_pred'] = target, pred
        out[name + '_empty'] = r32['empty']
        out[name + '_counts'] = np.array([r32['valid'].sum(), both_empty.sum()], np.int64)
        for tag, r in (('f32', r32), ('f64', r64)):
            for k in ('weights', 'normals', 'scalars', 'grad'):
                out['%s_%s_%s' % (name, k, tag)] = r[k]
    save_fixture('shape_loss', **out)
    size = (REPO / 'tests' / 'golden' / 'shape_loss.npz').stat().st_size
    print('tests/golden/shape_loss.npz: %d bytes' % size)
    assert size <= (REPO / 'tests' / 'golden' / 'mesh_metrics.npz').stat().st_size


if __name__ == '__main__':
    main()
