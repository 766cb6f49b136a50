"""The refinement trainer's steps on the device: ``RefinementTrainingModule.training_step_unet`` / ``_retrieval`` / ``_attention`` / ``_full`` and
``validation_step`` (trainer/train_refinement.py:50-86, :91-132, :223-229) as one plain class over the drop-in modules.  No Lightning, no loop, no
logging, no checkpoint writing: a step takes a batch and returns device tensors, the caller owns the optimiser and the epochs.

    step = RefinementStep.from_config(cfg, phase, modules, loss_side_task_retr=.., loss_side_task_unet=..)   # modules: the four networks by name
    opt = rfuse.optim.Adam(step.parameters(), lr=..)             # the reference's optimizer_unet / _retrieval / _attention / _full list, in its order
    out = step.training_step(dataset.batch(idx))                 # {'loss': .., the logged scalars, 'occupancy_attn', the predictions}; no host sync
    out['loss'].backward(); opt.step(); opt.zero_grad()
    step.validation_step(batch, metrics_fuse, metrics_nn1)       # under no_grad; updates the rfuse.metrics lists

Everything on the hot path is HIP: the networks through rfuse.autograd (the decoder's head included: PointwiseTanh), ``ShapeLoss``, ``AttnContrastiveLoss``,
and the attention rows' occupancy straight from the decoder's prediction (``ops.attn_occupancy_rows``, one launch for the reference's threshold, cast,
max_pool3d, unfold and any).  CPU tensors raise; there is no fallback.

Knowing the phase, a step does not compute what the reference computes and throws away: the networks outside ``parameters()`` are frozen for the duration
of the call (``requires_grad`` cleared and restored, ``.grad`` untouched), so their weight-gradient kernels are never launched, and any sub-graph no
optimised parameter depends on runs under ``no_grad`` on the inference routes -- in phase 2 the whole U-Net, retrieval backbone and decoder.
The reference's train() / eval() switches are not mirrored: none of the four networks has a layer that behaves differently in the two modes.
"""
import contextlib

import torch

from . import configs as _configs
from . import ops
from .losses import ShapeLoss, AttnContrastiveLoss

NETWORKS = ('unet_backbone', 'decoder', 'retrieval_backbone', 'patched_attention_block')
# trainer/train_refinement.py:185-203: what optimizer_unet, optimizer_retrieval, optimizer_attention and optimizer_full hand to Adam, in their order
PHASE_NETWORKS = (('unet_backbone', 'decoder'), ('retrieval_backbone',), ('patched_attention_block',), NETWORKS)
# the values the project documents (ShapeLoss, AttnContrastiveLoss); the two side-task weights have none: the reference's YAML files are not available
_DEFAULTS = {'weight_occupied': 8, 'loss_reconstruction': 1, 'loss_normal': 0.5, 'attn_temprature': 0.05, 'max_rows': 1280, 'loss_attn_contrastive': 0.01}
_REQUIRED_IN_PHASE_3 = ('loss_side_task_retr', 'loss_side_task_unet')


def _on_gpu(batch, names):
    for name in names:
        t = batch.get(name) if isinstance(batch, dict) else None
        if not isinstance(t, torch.Tensor):
            raise TypeError("RefinementStep: batch['%s'] must be a torch.Tensor" % name)
        if not t.is_cuda:
            raise RuntimeError("RefinementStep: batch['%s'] is a %s tensor; the step runs on the GPU only, there is no CPU fallback" % (name, t.device))


class RefinementStep:
    """One phase's training step and the validation step of the refinement trainer (see the module docstring).  ``hparams`` in the reference's spellings:
    K, attn_temprature, loss_reconstruction, loss_normal, weight_occupied, loss_attn_contrastive, loss_side_task_retr, loss_side_task_unet (the last two
    are required in phase 3 and have no default), and max_rows (the 1280 of compute_sliced_attn_nt_xent_loss)."""

    def __init__(self, phase, unet_backbone, decoder, retrieval_backbone, patched_attention_block, config, **hparams):
        if phase not in (0, 1, 2, 3):
            raise ValueError('RefinementStep: phase must be 0 (unet), 1 (retrieval), 2 (attention) or 3 (full), got %r' % (phase,))
        unknown = set(hparams) - set(_DEFAULTS) - set(_REQUIRED_IN_PHASE_3) - {'K'}
        if unknown:
            raise TypeError('RefinementStep: unknown hyper-parameters %s' % sorted(unknown))
        missing = [k for k in _REQUIRED_IN_PHASE_3 if phase == 3 and hparams.get(k) is None]
        if missing:
            raise TypeError('RefinementStep: phase 3 needs %s (the reference takes them from its YAML; there is no default)' % ', '.join(missing))
        self.phase, self.config = phase, config
        self.hparams = dict(_DEFAULTS, K=config['K'], **hparams)
        self.K = self.hparams['K']
        self.unet_backbone, self.decoder, self.retrieval_backbone, self.patched_attention_block = unet_backbone, decoder, retrieval_backbone, patched_attention_block
        d = config['dataset_train']
        self.target_trunc = _configs.truncations(config)[1]
        self.target_voxel_size, self.target_mean, self.target_std = d['voxel_size_target'], d['target_mean'], d['target_std']
        self.shape_loss = ShapeLoss.from_config(config, weight_occupied=self.hparams['weight_occupied'], loss_reconstruction=self.hparams['loss_reconstruction'],
                                                loss_normal=self.hparams['loss_normal'])
        self.loss_attn = AttnContrastiveLoss(self.hparams['attn_temprature'], self.hparams['max_rows'])
        from model.attention import Unfold3D, Fold3D            # trainer :34-37
        nf = retrieval_backbone.nf
        self.unfold_shape, self.unfold_features = Unfold3D(16, 1), Unfold3D(8, nf)
        self.fold_shape, self.fold_features = Fold3D(4, 16, 1), Fold3D(4, 8, nf)

    @classmethod
    def from_config(cls, config, phase, modules, **hparams):
        """``modules``: a mapping with the four networks under the reference's attribute names (``NETWORKS``), e.g. ``RefinementEngine.modules()``"""
        return cls(phase, *(modules[name] for name in NETWORKS), config, **hparams)

    # ------------------------------------------------------------------------------------------------ parameters
    def networks(self):
        return {name: getattr(self, name) for name in NETWORKS}

    def named_parameters(self):
        """(name, parameter) in the order of ``parameters()``, names prefixed like the reference's state_dict ('decoder.network.1.weight')"""
        return [(net + '.' + name, p) for net in PHASE_NETWORKS[self.phase] for name, p in getattr(self, net).named_parameters()]

    def parameters(self):
        """the list the reference's optimiser of this phase is built over, in its order (trainer :185-203): a Lightning ``optimizer_states`` entry
        loads into ``rfuse.optim.Adam(step.parameters())`` with the indices lined up"""
        return [p for _, p in self.named_parameters()]

    @contextlib.contextmanager
    def _frozen(self):
        """networks outside parameters(): requires_grad cleared for the duration of the call, the previous flags restored; .grad is not touched"""
        saved = [(p, p.requires_grad) for net in NETWORKS if net not in PHASE_NETWORKS[self.phase] for p in getattr(self, net).parameters()]
        try:
            for p, _ in saved:
                p.requires_grad_(False)
            yield
        finally:
            for p, flag in saved:
                p.requires_grad_(flag)

    # ------------------------------------------------------------------------------------------------ the reference's small helpers
    def network_pred_to_df(self, pred):
        return (pred + 1) * self.target_trunc / 2                   # trainer :242-243

    def denormalize_target(self, target):
        return target * self.target_std + self.target_mean

    def occupancy_rows(self, pred):
        """occupancy_from_prediction(network_pred_to_df(pred)) (trainer :245-247) followed by get_features' unfold and any (model/attention.py:135-138):
        bool [B * rows], one launch; no gradient (the reference detaches it)"""
        return ops.attn_occupancy_rows(pred.detach().contiguous(), self.target_trunc, self.target_voxel_size * 0.75, self.patched_attention_block.patch_extent)

    def get_retrievals(self, retrievals):
        b, s = retrievals.shape[0], retrievals.shape[2]
        return retrievals[:, :self.K, :, :, :].reshape((b * self.K, 1, s, s, s))

    def _contrastive(self, slices, fpred, ftgt, occupancy_attn, out, key='attn_contrastive'):
        out[key] = self.loss_attn(slices, fpred, ftgt, occupancy_attn)
        out['attn_occupancy'] = self.loss_attn.last_counts[0]
        out['occupancy_attn'] = occupancy_attn
        return out[key]

    def _shape(self, pred, batch, out, suffix=''):
        out['shape' + suffix], out['l1' + suffix], out['normal' + suffix] = self.shape_loss.loss_shape(pred, batch)
        return out['shape' + suffix]

    # ------------------------------------------------------------------------------------------------ the forwards
    def forward_backbone(self, batch):
        return self.decoder(self.unet_backbone(batch['input']))                                                     # trainer :91-94

    def forward_retrieval(self, batch):
        return self.fold_shape(self.decoder(self.retrieval_backbone(self.unfold_shape(batch['target']))))         # trainer :96-99

    def forward_attention(self, batch):
        """trainer :101-106 (and the U-Net's prediction the occupancy came from).  Everything before get_features depends on no attention parameter:
        no_grad, the inference routes."""
        with torch.no_grad():
            x_ = self.unet_backbone(batch['input'])
            x_target = self.fold_features(self.retrieval_backbone(self.unfold_shape(batch['target'])))
            pred_back = self.decoder(x_)
            rows = self.occupancy_rows(pred_back)
        return self.patched_attention_block.get_features(x_, x_target, None, occupancy_rows=rows) + (pred_back,)

    def forward_full(self, batch, gumbel_noise=None):
        """trainer :108-120 -> pred_shape, pred_shape_back, pred_shape_retr, x_attn_fpred, x_attn_ftgt, occupancy_attn"""
        x_back = self.unet_backbone(batch['input'])
        retrievals = self.get_retrievals(batch['retrieval'])
        n_retr = retrievals.shape[0]
        both = self.fold_features(self.retrieval_backbone(self.unfold_shape(torch.cat([retrievals, batch['target']], dim=0))))
        x_retrieval, x_target = both[:n_retr], both[n_retr:]
        x = self.patched_attention_block(x_back, x_retrieval, gumbel_noise)
        pred_shape = self.decoder(x)
        pred_retr = self.fold_shape(self.decoder(self.unfold_features(x_target)))
        pred_back = self.decoder(x_back)
        fpred, ftgt, occupancy_attn = self.patched_attention_block.get_features(x_back, x_target, None, occupancy_rows=self.occupancy_rows(pred_back))
        return pred_shape, pred_back, pred_retr, fpred, ftgt, occupancy_attn

    # ------------------------------------------------------------------------------------------------ the steps
    def training_step(self, batch, gumbel_noise=None):
        """``batch``: 'input', 'target' (and 'retrieval' in phase 3) as ``rfuse.data.PatchDataset.batch`` returns them; it gains 'weights', 'empty' and
        'normals' (augment_batch_data).  Returns a dict of device tensors: 'loss', the scalars the reference logs for the phase ('shape' / 'l1' /
        'normal' per decoder output -- suffixed '_fuse', '_back', '_retr' in phase 3 --, 'attn_contrastive', 'attn_occupancy'), 'occupancy_attn' (the bool
        row vector) and the predictions ('pred_shape', 'pred_back', 'pred_retr').  Nothing waits for the host."""
        _on_gpu(batch, ('input', 'target') + (('retrieval',) if self.phase == 3 else ()))
        out = {}
        with self._frozen():
            self.shape_loss.augment_batch_data(batch)
            if self.phase == 0:
                out['pred_shape'] = self.forward_backbone(batch)
                out['loss'] = self._shape(out['pred_shape'], batch, out)
            elif self.phase == 1:
                out['pred_shape'] = self.forward_retrieval(batch)
                out['loss'] = self._shape(out['pred_shape'], batch, out)
            elif self.phase == 2:
                fpred, ftgt, occupancy_attn, out['pred_back'] = self.forward_attention(batch)
                out['loss'] = self._contrastive(batch['target'].shape[0] * 8, fpred, ftgt, occupancy_attn, out)
            else:
                out['pred_shape'], out['pred_back'], out['pred_retr'], fpred, ftgt, occupancy_attn = self.forward_full(batch, gumbel_noise)
                fuse = self._shape(out['pred_shape'], batch, out, '_fuse')
                back = self._shape(out['pred_back'], batch, out, '_back')
                retr = self._shape(out['pred_retr'], batch, out, '_retr')
                contrastive = self._contrastive(out['pred_retr'].shape[0] * 8, fpred, ftgt, occupancy_attn, out)
                out['loss'] = (fuse + contrastive * self.hparams['loss_attn_contrastive'] + retr * self.hparams['loss_side_task_retr']
                               + back * self.hparams['loss_side_task_unet'])              # trainer :84
        return out

    @torch.no_grad()
    def validation_step(self, batch, metrics_fuse=None, metrics_nn1=None, gumbel_noise=None):
        """trainer :122-132 with get_evaluation_for_batch (:223-229), its quirk included: loss_shape is fed the DISTANCE FIELD, not the network output.
        ``metrics_fuse`` / ``metrics_nn1``: iterables of ``rfuse.metrics`` modules, updated with ``df <= 0.75 voxel`` of the fused prediction / the first
        retrieval against the target's occupancy.  Returns 'attn_contrastive', 'attn_occupancy', 'occupancy_attn', the three predictions and
        'shape' / 'l1' / 'normal' suffixed '_full' and '_nn1'."""
        _on_gpu(batch, ('input', 'target', 'retrieval'))
        out = {}
        self.shape_loss.augment_batch_data(batch)
        out['pred_shape'], out['pred_back'], out['pred_retr'], fpred, ftgt, occupancy_attn = self.forward_full(batch, gumbel_noise)
        self._contrastive(out['pred_back'].shape[0] * 8, fpred, ftgt, occupancy_attn, out)
        thr = self.target_voxel_size * 0.75
        target_shape = self.denormalize_target(batch['target']) <= thr
        for suffix, metrics, df in (('_full', metrics_fuse, self.network_pred_to_df(out['pred_shape'])),
                                    ('_nn1', metrics_nn1, self.denormalize_target(batch['retrieval'][:, :1, :, :, :]))):
            predicted_shape = df <= thr
            for metric in (metrics if metrics is not None else ()):
                metric(predicted_shape, target_shape)
            self._shape(df.contiguous(), batch, out, suffix)
        return out
