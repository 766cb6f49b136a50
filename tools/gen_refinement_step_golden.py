"""Fixture generator for the refinement trainer's steps (CPU, float32; needs the reference checkout, as tools/gen_shape_loss_golden.py does): runs the
reference's own ``RefinementTrainingModule.training_step_unet`` / ``_retrieval`` / ``_attention`` / ``_full`` and ``validation_step``
(trainer/train_refinement.py:50-132) as written, over the reference's own networks, and writes tests/golden/refinement_step.npz (arrays only, a few KB).

    python tools/gen_refinement_step_golden.py

``pytorch_lightning`` is stood in for through ``sys.modules`` (tools/gen_shape_loss_golden.import_reference_trainer); the module instance is made without
its ``__init__`` (which builds scene handlers and datasets from files) and given the attributes the methods touch: the four networks from the reference's
factories with seeded weights, the fold / unfold modules, ``NTXentLoss``, ``hparams``, a ``log`` that records, and stand-ins that supply ``target_trunc``,
``target_voxel_size``, ``denormalize_target`` and ``compute_normals`` (the reference's own two dataset methods, bound to a namespace).  ``Tensor.cuda`` is
mapped to ``Tensor.to`` for the calls, as tools/gen_contrastive_golden.py does.  Gumbel-hard attention draws its noise inside torch's ``gumbel_softmax``;
for the calls that function is replaced by torch's own formula with the noise given (the tests scale it by 4, which a seed cannot express).

Inputs: configs C3 (softmax attention; phases 0-3 and validation) and C1 (Gumbel-hard; phase 3), B = 1, the seeds of
tests/test_autograd_gpu.py:test_forward_full_trains_like_the_oracle (tests/refinement_step_ref.problem).  The side-task weights are
tests/refinement_step_ref.HPARAMS's.

Layout: ``cases`` (names ``<config>_p<phase>`` and ``<config>_val``); per case ``_scalar_names`` / ``_scalars`` float64 (the loss and what the reference logs or
returns from loss_shape, in call order), ``_occ`` (np.packbits of occupancy_attn; phases 2, 3 and validation), ``_param_names`` / ``_grad_norms`` float32 (every
parameter of the phase's optimiser, in its order; training cases), ``_stats`` int64 = occupied rows, voxels of pred_back with |df - thr| <= 1e-4 trunc, voxels
with |pred| > 0.95 (phases 2, 3), and for validation ``_metric_counts`` int64 [2][3] = (n_pred, n_target, n_inter) as fed to the fuse and the 1-NN metrics.
"""
import sys
import types
from pathlib import Path
from unittest import mock

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tests'))
from oracle.gen_golden import REF, save_fixture                 # noqa: E402
from tools.gen_shape_loss_golden import import_reference_trainer      # noqa: E402
from rfuse import synthetic                                     # noqa: E402
import refinement_step_ref as ref                               # noqa: E402

CASES = [('C3', 0), ('C3', 1), ('C3', 2), ('C3', 3), ('C3', 'val'), ('C1', 3)]


def given_noise_gumbel_softmax(noise):
    """torch.nn.functional.gumbel_softmax with its draw replaced by ``noise``"""
    def gumbel_softmax(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        y_soft = ((logits + noise.to(logits.dtype)) / tau).softmax(dim)
        if not hard:
            return y_soft
        index = y_soft.max(dim, keepdim=True)[1]
        y_hard = torch.zeros_like(logits, memory_format=torch.legacy_contiguous_format).scatter_(dim, index, 1.0)
        return y_hard - y_soft.detach() + y_soft
    return gumbel_softmax


def build_module(Module, Dataset, ref_model, ref_loss, cfg, hp):
    from model.attention import Unfold3D, Fold3D
    c = ref.constants(cfg)
    mod = Module.__new__(Module)
    torch.nn.Module.__init__(mod)
    with mock.patch('builtins.print'):
        nets = {'unet_backbone': ref_model.get_unet_backbone(cfg), 'decoder': ref_model.get_decoder(cfg), 'retrieval_backbone': ref_model.get_retrieval_backbone(cfg),
                'patched_attention_block': ref_model.get_attention_block(cfg)}
    for i, (name, net) in enumerate(nets.items()):
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.seeded_state_dict(shapes, ref.SD_SEED + i).items()})
        setattr(mod, name, net)
    mod.K = cfg['K']
    mod.unfold_shape, mod.unfold_features = Unfold3D(16, 1), Unfold3D(8, mod.retrieval_backbone.nf)
    mod.fold_shape, mod.fold_features = Fold3D(4, 16, 1), Fold3D(4, 8, mod.retrieval_backbone.nf)
    mod.loss_ntxent = ref_loss.NTXentLoss(hp['attn_temprature'], True)
    object.__setattr__(mod, 'hparams', dict(hp, lr=1e-4, scheduler=None))
    handler = types.SimpleNamespace(target_trunc=c['trunc'], target_voxel_size=cfg['dataset_train']['voxel_size_target'])
    ds = types.SimpleNamespace(scene_handler=handler, target_mean=c['mean'], target_std=c['std'], sobel_3d_x=Dataset.sobel_3d_x, sobel_3d_y=Dataset.sobel_3d_y,
                               sobel_3d_z=Dataset.sobel_3d_z)
    ds.compute_normals = types.MethodType(Dataset.compute_normals, ds)
    ds.denormalize_target = types.MethodType(Dataset.denormalize_target, ds)
    object.__setattr__(mod, 'scene_handlers', {'train': handler, 'val': handler})
    object.__setattr__(mod, 'train_dataset', ds)
    object.__setattr__(mod, 'val_dataset', ds)
    return mod, nets


def record(mod, Module):
    """wrap what the steps call on the way, so that what they compute and do not return is seen"""
    seen = {'scalars': [], 'occ': None, 'pred_back': None, 'metrics': []}

    def loss_shape(pred, batch):
        r = Module.loss_shape(mod, pred, batch)
        tag = 'abcdefgh'[len([s for s in seen['scalars'] if s[0].startswith('shape')])]
        seen['scalars'] += [(k + '_' + tag, float(v.detach().sum())) for k, v in zip(('shape', 'l1', 'normal'), r)]
        return r

    def sliced(batch_size, fpred, ftgt, occupancy_attn):
        r = Module.compute_sliced_attn_nt_xent_loss(mod, batch_size, fpred, ftgt, occupancy_attn)
        seen['scalars'].append(('attn_contrastive', float(r.detach().sum())))
        seen['occ'] = occupancy_attn.detach().numpy().astype(bool)
        return r

    def occupancy_from_prediction(df):
        seen['df_back'] = df.detach()
        return Module.occupancy_from_prediction(mod, df)

    def log(name, value, **kw):
        if name.endswith('attn_occupancy'):
            seen['scalars'].append(('attn_occupancy', float(value)))

    def metric(kind):
        def call(pred, target):
            seen['metrics'].append((kind, int(pred.sum()), int(target.sum()), int((pred & target).sum())))
        return call

    for name, fn in (('loss_shape', loss_shape), ('compute_sliced_attn_nt_xent_loss', sliced), ('occupancy_from_prediction', occupancy_from_prediction), ('log', log)):
        object.__setattr__(mod, name, fn)
    for name, kind in (('metrics_train_fuse', 'fuse'), ('metrics_val_fuse', 'fuse'), ('metrics_train_nn1', 'nn1'), ('metrics_val_nn1', 'nn1')):
        object.__setattr__(mod, name, [metric(kind)])
    return seen


def main():
    Module, Dataset = import_reference_trainer()
    import model as ref_model
    import model.loss as ref_loss
    assert str(REF) in ref_model.__file__ and str(REF) in ref_loss.__file__
    torch.set_num_threads(min(32, torch.get_num_threads()))
    out, names = {}, []
    hp = dict(ref.HPARAMS)
    built = {}
    for cfg_name, phase in CASES:
        if cfg_name not in built:
            from rfuse import configs as rf_configs
            cfg = rf_configs.get_config(cfg_name)
            mod, nets = build_module(Module, Dataset, ref_model, ref_loss, cfg, hp)
            shapes = {k: {n: tuple(v.shape) for n, v in net.state_dict().items()} for k, net in nets.items()}
            built[cfg_name] = (cfg, mod, nets, ref.problem(cfg_name, shapes))
        cfg, mod, nets, (_, _, data, noise) = built[cfg_name]
        c = ref.constants(cfg)
        case = '%s_%s' % (cfg_name, 'val' if phase == 'val' else 'p%d' % phase)
        names.append(case)
        seen = record(mod, Module)
        for net in nets.values():
            net.zero_grad(set_to_none=True)
        batch = {k: v.clone() for k, v in data.items()}
        patches = [mock.patch.object(torch.Tensor, 'cuda', lambda self, device=None, **kw: self.to(device))]
        if noise is not None:
            patches.append(mock.patch('torch.nn.functional.gumbel_softmax', given_noise_gumbel_softmax(noise)))
        for p in patches:
            p.start()
        try:
            if phase == 'val':
                with torch.no_grad():
                    mod.validation_step(batch, 0, 0)
                scalars = seen['scalars']
            else:
                step = (mod.training_step_unet, mod.training_step_retrieval, mod.training_step_attention, mod.training_step_full)[phase]
                loss = step(batch, 0)['loss']
                loss.sum().backward()
                scalars = [('loss', float(loss.detach().sum()))] + seen['scalars']
                opt = (mod.optimizer_unet, mod.optimizer_retrieval, mod.optimizer_attention, mod.optimizer_full)[phase]()
                opt = opt[0][0] if isinstance(opt, tuple) else opt[0]
                by_id = {id(p): net_name + '.' + n for net_name, net in nets.items() for n, p in net.named_parameters()}
                params = opt.param_groups[0]['params']
                out[case + '_param_names'] = np.array([by_id[id(p)] for p in params])
                out[case + '_grad_norms'] = np.array([0.0 if p.grad is None else float(p.grad.double().norm()) for p in params], np.float32)
        finally:
            for p in patches:
                p.stop()
        out[case + '_scalar_names'] = np.array([s[0] for s in scalars])
        out[case + '_scalars'] = np.array([s[1] for s in scalars], np.float64)
        line = '%-7s %s' % (case, '  '.join('%s %.7g' % s for s in scalars))
        if seen['occ'] is not None:
            out[case + '_occ'] = np.packbits(seen['occ'])
            df = seen['df_back']
            pred = df * 2 / c['trunc'] - 1
            stats = [int(seen['occ'].sum()), int(((df - c['thr']).abs() <= 1e-4 * c['trunc']).sum()), int((pred.abs() > 0.95).sum())]
            out[case + '_stats'] = np.array(stats, np.int64)
            groups, counts = ref.contrastive_ref.select(seen['occ'], 8 * data['target'].shape[0], hp['max_rows'])
            line += '\n        rows occupied %d of %d, slices taken %d of 8 (%d rows), voxels within the margin %d, |pred| > 0.95: %d' % (
                stats[0], seen['occ'].size, counts[2], counts[1], stats[1], stats[2])
        if phase == 'val':
            m = {kind: (a, b, i) for kind, a, b, i in seen['metrics']}
            out[case + '_metric_counts'] = np.array([m['fuse'], m['nn1']], np.int64)
        print(line)
    out['cases'] = np.array(names)
    save_fixture('refinement_step', **out)
    size = (REPO / 'tests' / 'golden' / 'refinement_step.npz').stat().st_size
    print('tests/golden/refinement_step.npz: %d bytes' % size)
    assert size <= 64 * 1024


if __name__ == '__main__':
    main()
