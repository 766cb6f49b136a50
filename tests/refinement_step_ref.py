"""The refinement trainer's four training steps and its validation quantities (trainer/train_refinement.py:50-132, :175-183, :208-253) restated in plain
torch, any dtype, from pieces that exist already: the networks of oracle/refpath.py, the shape loss of tests/shape_loss_ref.py and the sliced contrastive
loss of tests/contrastive_ref.py.  Independent of the kernels; tests/test_refinement_step_cpu.py holds it (float32) to the reference's own methods
(tests/golden/refinement_step.npz), tests/test_refinement_step_gpu.py uses it in float64 as the other side of ``rfuse.training.RefinementStep``.

``occupancy_rows``: an override of the attention rows' occupancy.  The rows are a discrete choice (a voxel on one side or the other of the
threshold); a comparison of the arithmetic after it gives both sides the same rows.
"""
import contextlib
import io

import numpy as np
import torch
import torch.nn.functional as F

import contrastive_ref
import helpers
import shape_loss_ref
from oracle import refpath
from rfuse import configs as rf_configs

NETWORKS = ('unet_backbone', 'decoder', 'retrieval_backbone', 'patched_attention_block')
PHASE_NETWORKS = (('unet_backbone', 'decoder'), ('retrieval_backbone',), ('patched_attention_block',), NETWORKS)       # trainer :185-203
HPARAMS = {'weight_occupied': 8, 'loss_reconstruction': 1, 'loss_normal': 0.5, 'attn_temprature': 0.05, 'max_rows': 1280, 'loss_attn_contrastive': 0.01,
           'loss_side_task_retr': 0.5, 'loss_side_task_unet': 0.25}      # the side-task weights: the tests' own choice, two different values
SD_SEED, INPUT_SEED, NOISE_SCALE = 7000, 21, 4.0                        # tests/test_autograd_gpu.py:test_forward_full_trains_like_the_oracle


def constants(cfg):
    d = cfg['dataset_train']
    return {'trunc': rf_configs.truncations(cfg)[1], 'thr': d['voxel_size_target'] * 0.75, 'mean': d['target_mean'], 'std': d['target_std']}


def make_modules(cfg):
    """the drop-in modules (CPU, only their parameter names and shapes matter here)"""
    import model
    with contextlib.redirect_stdout(io.StringIO()):
        return {'unet_backbone': model.get_unet_backbone(cfg), 'decoder': model.get_decoder(cfg), 'retrieval_backbone': model.get_retrieval_backbone(cfg),
                'patched_attention_block': model.get_attention_block(cfg)}


def problem(cfg_name, shapes_by_module, batch=1):
    """-> cfg, state dicts (float32), batch dict (float32, CPU), Gumbel noise or None: the seeds of test_forward_full_trains_like_the_oracle"""
    cfg = rf_configs.get_config(cfg_name)
    trunc_t = rf_configs.truncations(cfg)[1]
    sds = {k: helpers.seeded_sd(shapes_by_module[k], SD_SEED + i) for i, k in enumerate(NETWORKS)}
    gen = torch.Generator().manual_seed(INPUT_SEED)
    K, s_in = cfg['K'], cfg['dataset_train']['input_chunk_size']
    data = {'input': torch.randn(batch, 1, s_in, s_in, s_in, generator=gen), 'retrieval': torch.randn(batch, K, 64, 64, 64, generator=gen),
            'target': torch.rand(batch, 1, 64, 64, 64, generator=gen) * trunc_t}
    noise = -torch.empty(batch * 4096, K).exponential_(generator=gen).log() * NOISE_SCALE if cfg['attn_retrieval_mode'] else None
    return cfg, sds, data, noise


def leaves(sds, dtype):
    return {k: {n: v.detach().clone().to(dtype).requires_grad_(True) for n, v in sd.items()} for k, sd in sds.items()}


def network_pred_to_df(pred, trunc):
    return (pred + 1) * trunc / 2


def occupancy_from_prediction(df, thr):
    return F.max_pool3d((df <= thr).to(df.dtype), kernel_size=2, stride=2).bool()


def occupancy_rows(pred, trunc, thr, e):
    """the torch formula of the attention rows' occupancy: threshold, max_pool3d, unfold, any"""
    occ = refpath.unfold3d(occupancy_from_prediction(network_pred_to_df(pred, trunc), thr), e)
    return occ.reshape(occ.shape[0], -1).any(dim=1)


def margin_rows(pred, trunc, thr, e, margin):
    """rows whose (2e)^3 block holds a voxel with |df - thr| <= margin"""
    near = ((network_pred_to_df(pred, trunc) - thr).abs() <= margin).to(pred.dtype)
    rows = refpath.unfold3d(F.max_pool3d(near, kernel_size=2, stride=2).bool(), e)
    return rows.reshape(rows.shape[0], -1).any(dim=1)


def loss_shape(pred, data, cfg, hp):
    c = constants(cfg)
    total, l1, normal, _ = shape_loss_ref.loss(pred, data['target'], c['trunc'], c['mean'], c['std'], hp['weight_occupied'], hp['loss_reconstruction'], hp['loss_normal'])
    return total, l1, normal


def _attn_e(cfg):
    return cfg['attn_patch_extent'] // 2


def _features(sds, cfg, x_back, x_target, pred_back, rows_override):
    c = constants(cfg)
    occupancy = occupancy_from_prediction(network_pred_to_df(pred_back.detach(), c['trunc']), c['thr'])
    fpred, ftgt, rows = refpath.patched_get_features(x_back, x_target, occupancy, sds['patched_attention_block'], cfg)
    return fpred, ftgt, rows if rows_override is None else torch.as_tensor(rows_override).reshape(-1).bool()


def forward_full(sds, cfg, data, noise=None, rows_override=None):
    """trainer :108-120"""
    b, k, nf = data['target'].shape[0], cfg['K'], cfg['nf']
    x_back = refpath.unet_backbone(data['input'], sds['unet_backbone'], cfg)
    retrievals = data['retrieval'][:, :k].reshape(b * k, 1, 64, 64, 64)
    both = refpath.fold3d(refpath.retrieval_backbone(refpath.unfold3d(torch.cat([retrievals, data['target']], 0), 16), sds['retrieval_backbone'], cfg), 4, 8, nf)
    x_retrieval, x_target = both[:b * k], both[b * k:]
    x = refpath.patched_attention_block(x_back, x_retrieval, sds['patched_attention_block'], cfg, noise)
    pred = refpath.final_decoder(x, sds['decoder'], cfg)
    pred_retr = refpath.fold3d(refpath.final_decoder(refpath.unfold3d(x_target, 8), sds['decoder'], cfg), 4, 16, 1)
    pred_back = refpath.final_decoder(x_back, sds['decoder'], cfg)
    return (pred, pred_back, pred_retr) + _features(sds, cfg, x_back, x_target, pred_back, rows_override)


def _contrastive(out, slices, fpred, ftgt, rows, hp):
    loss, counts = contrastive_ref.sliced(slices, fpred, ftgt, rows, hp['attn_temprature'], hp['max_rows'])
    out['attn_contrastive'], out['attn_occupancy'], out['occupancy_attn'] = loss, counts[0], rows
    return loss


def _shape(out, pred, data, cfg, hp, suffix=''):
    out['shape' + suffix], out['l1' + suffix], out['normal' + suffix] = loss_shape(pred, data, cfg, hp)
    return out['shape' + suffix]


def training_step(phase, sds, cfg, data, hp=HPARAMS, noise=None, rows_override=None):
    """-> the dict ``RefinementStep.training_step`` returns, same keys; ``sds``: {network: {name: tensor}} (leaves that require grad where wanted)"""
    out, b, nf = {}, data['target'].shape[0], cfg['nf']
    if phase == 0:
        out['pred_shape'] = refpath.final_decoder(refpath.unet_backbone(data['input'], sds['unet_backbone'], cfg), sds['decoder'], cfg)
        out['loss'] = _shape(out, out['pred_shape'], data, cfg, hp)
    elif phase == 1:
        x = refpath.retrieval_backbone(refpath.unfold3d(data['target'], 16), sds['retrieval_backbone'], cfg)
        out['pred_shape'] = refpath.fold3d(refpath.final_decoder(x, sds['decoder'], cfg), 4, 16, 1)
        out['loss'] = _shape(out, out['pred_shape'], data, cfg, hp)
    elif phase == 2:
        x_ = refpath.unet_backbone(data['input'], sds['unet_backbone'], cfg)
        x_target = refpath.fold3d(refpath.retrieval_backbone(refpath.unfold3d(data['target'], 16), sds['retrieval_backbone'], cfg), 4, 8, nf)
        out['pred_back'] = refpath.final_decoder(x_, sds['decoder'], cfg)
        fpred, ftgt, rows = _features(sds, cfg, x_, x_target, out['pred_back'], rows_override)
        out['loss'] = _contrastive(out, b * 8, fpred, ftgt, rows, hp)
    else:
        out['pred_shape'], out['pred_back'], out['pred_retr'], fpred, ftgt, rows = forward_full(sds, cfg, data, noise, rows_override)
        fuse = _shape(out, out['pred_shape'], data, cfg, hp, '_fuse')
        back = _shape(out, out['pred_back'], data, cfg, hp, '_back')
        retr = _shape(out, out['pred_retr'], data, cfg, hp, '_retr')
        contrastive = _contrastive(out, b * 8, fpred, ftgt, rows, hp)
        out['loss'] = fuse + contrastive * hp['loss_attn_contrastive'] + retr * hp['loss_side_task_retr'] + back * hp['loss_side_task_unet']
    return out


def validation_step(sds, cfg, data, hp=HPARAMS, noise=None, rows_override=None):
    """trainer :122-132, :223-229 (loss_shape on the DISTANCE FIELD, as the reference has it) -> scalars as in RefinementStep.validation_step, plus the
    occupancy grids the metrics are fed: 'occ_full', 'occ_nn1', 'occ_target'"""
    c, out = constants(cfg), {}
    with torch.no_grad():
        out['pred_shape'], out['pred_back'], out['pred_retr'], fpred, ftgt, rows = forward_full(sds, cfg, data, noise, rows_override)
        _contrastive(out, data['target'].shape[0] * 8, fpred, ftgt, rows, hp)
        out['occ_target'] = data['target'] * c['std'] + c['mean'] <= c['thr']
        for suffix, df in (('_full', network_pred_to_df(out['pred_shape'], c['trunc'])), ('_nn1', data['retrieval'][:, :1] * c['std'] + c['mean'])):
            out['occ' + suffix] = df <= c['thr']
            _shape(out, df, data, cfg, hp, suffix)
    return out


def grad_norms(sds, phase):
    """float32 norm of every optimised parameter's gradient, in the optimiser's order; a parameter nothing flows to (sig_scale / sig_shift) counts as 0"""
    return np.array([0.0 if p.grad is None else float(p.grad.detach().double().norm()) for net in PHASE_NETWORKS[phase] for p in sds[net].values()], np.float32)


def parameter_names(sds, phase):
    return [net + '.' + name for net in PHASE_NETWORKS[phase] for name in sds[net]]
