"""GPU: NT-Xent and the sliced attention contrastive loss (rfuse/losses.py NTXent / AttnContrastiveLoss, csrc/ntxent.hip) against
tests/golden/contrastive_loss.npz, the record of the reference's own NTXentLoss.forward / compute_sliced_attn_nt_xent_loss in float32 and in float64
(tools/gen_contrastive_golden.py), and the gradients of PatchedAttentionBlock.get_features in grad mode.

Tolerance rule (shape_loss_ref.within): with err_hip = |x_hip - x_f64| and err_ref = |x_ref32 - x_f64|, both against the fixture's float64 record,
err_hip <= max(2 * err_ref, floor); floor = 4 float32 ulps of |x_f64| for a scalar, and for a tensor 4 ulps of max |x_f64| with max-abs errors.
err_ref as the generator printed it (loss: relative; gradients: max-abs over max |x_f64|):
    n1        loss 0        grad zis   0        zjs  0             (no negative: everything is exactly 0)
    n2        loss 5.8e-8   grad zis   9.5e-8   zjs  9.6e-8
    n67       loss 1.3e-7   grad zis   3.8e-7   zjs  4.4e-7
    iou96     loss 1.2e-7   grad zis   5.1e-7   zjs  6.4e-7
    iou96sym  loss 1.3e-8   grad zis   4.7e-7   zjs  5.0e-7
    dot30     loss 3.9e-8   grad zis   0        zjs  0             (a one-hot softmax: the gradient is a difference of two rows, exact in float32)
    zero      loss 1.6e-8   grad zis   1.3e-7   zjs  1.2e-7        (max |grad| is the all-zero row's 2.0e7 = dw / 1e-8; the other rows are checked on their own)
    cap20     loss 2.3e-7   grad fpred 1.8e-7   ftgt 3.4e-7
    ragged    loss 6.7e-8   grad fpred 1.7e-7   ftgt 1.7e-7
    empty     loss 0        grad       0
    trainer   loss 7.6e-8   grad fpred 2.8e-7   ftgt 2.7e-7
Counts, the selection and exact-zero patterns are compared exactly.
The fixture stops at 64 features and 512 pairs in two occupied slices: widths above 64 (several feature chunks), the trainer's own geometry and one large
group are in tests/test_loss_sweep_gpu.py, on generated cases against the float64 restatement."""
import contextlib
import io

import numpy as np
import pytest
import torch

import contrastive_ref as cr
import helpers
import shape_loss_ref as slr
import testkit
from oracle import refpath
from rfuse import configs as rf_configs

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SINGLE = ['n1', 'n2', 'n67', 'iou96', 'iou96sym', 'dot30', 'zero']
SLICED = ['cap20', 'ragged', 'empty', 'trainer']


@pytest.fixture(scope='module')
def fixture(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    return cr.load_fixture(golden_dir)


def run_single(c, scale=None):
    from rfuse.losses import NTXent
    tau, cosine, sig_scale, sig_shift = (float(v) for v in c['params'])
    ntx = NTXent(tau, bool(cosine), sig_scale, sig_shift)
    zis, zjs = (torch.from_numpy(c[k]).to(DEV).requires_grad_(True) for k in ('zis', 'zjs'))
    loss = ntx(zis, zjs, torch.from_numpy(c['iou']).to(DEV) if 'iou' in c else None)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device == zis.device
    (loss if scale is None else scale * loss).backward()
    return loss.detach(), zis.grad, zjs.grad


def run_sliced(c, scale=None, values=None):
    from rfuse.losses import AttnContrastiveLoss
    tau, num_slices, max_rows = float(c['params'][0]), int(c['params'][1]), int(c['params'][2])
    acl = AttnContrastiveLoss(tau, max_rows)
    if values is None:
        values = tuple(torch.from_numpy(c[k]).to(DEV) for k in ('fpred', 'ftgt'))
    fpred, ftgt = (v.clone().requires_grad_(True) for v in values)
    loss = acl(num_slices, fpred, ftgt, torch.from_numpy(c['occ']).to(DEV))
    assert loss.shape == (1,) and loss.dtype == torch.float32 and loss.device == fpred.device
    assert acl.last_counts.shape == (3,) and acl.last_counts.dtype == torch.int64 and acl.last_counts.device == fpred.device
    (loss if scale is None else scale * loss).sum().backward()
    return loss.detach(), fpred.grad, ftgt.grad, acl.last_counts


@pytest.mark.parametrize('name', SINGLE)
def test_ntxent_loss_and_gradients_match_the_fixture(fixture, name):
    c = fixture[name]
    loss, gi, gj = run_single(c)
    assert gi.shape == c['zis'].shape and gi.dtype == gj.dtype == torch.float32
    assert slr.within(loss.item(), c['loss_f32'], c['loss_f64'], name + ' loss')
    for g, k in ((gi, 'zis'), (gj, 'zjs')):
        g = g.cpu().numpy()
        assert slr.within(g, c['grad_%s_f32' % k], c['grad_%s_f64' % k], '%s grad %s' % (name, k))
        if name == 'zero' and k == 'zis':         # the clamped row's gradient is 1e8 times the others': those on their own
            rest = [0, 1, 2, 4]
            assert slr.within(g[rest], c['grad_zis_f32'][rest], c['grad_zis_f64'][rest], 'zero grad zis, the other rows')
    if name == 'n1':
        assert loss.item() == 0 and not gi.any() and not gj.any()


@pytest.mark.parametrize('name', SLICED)
def test_sliced_loss_counts_and_gradients_match_the_fixture(fixture, name):
    c = fixture[name]
    loss, gp, gt, counts = run_sliced(c)
    np.testing.assert_array_equal(counts.cpu().numpy(), c['counts'])
    assert slr.within(loss.item(), c['loss_f32'], c['loss_f64'], name + ' loss')
    rows = c['rows']
    rest = np.setdiff1d(np.arange(c['fpred'].shape[0]), rows)
    for g, k in ((gp, 'fpred'), (gt, 'ftgt')):
        assert g.shape == c[k].shape and g.dtype == torch.float32
        g = g.cpu().numpy()
        assert not g[rest].any(), 'a row that was not selected has a gradient'
        if len(rows):
            assert slr.within(g[rows], c['grad_%s_f32' % k], c['grad_%s_f64' % k], '%s grad %s' % (name, k))
    if name == 'empty':
        assert loss.item() == 0 and not gp.any() and not gt.any()


def test_upstream_gradient_scales_the_gradient(fixture):
    """(3 * loss).backward(): the gradient is read from the device and multiplies every row; bound = 3 times the fixture's error, or 4 ulps"""
    for name, run, keys in (('n67', run_single, ('zis', 'zjs')), ('cap20', run_sliced, ('fpred', 'ftgt'))):
        c = fixture[name]
        out = run(c, scale=3.0)
        for g, k in zip(out[1:3], keys):
            g = g.cpu().numpy()
            g = g[c['rows']] if name == 'cap20' else g
            assert slr.within(g, 3.0 * c['grad_%s_f32' % k].astype(np.float64), 3.0 * c['grad_%s_f64' % k], '%s 3 x grad %s' % (name, k))


def flat(out):
    return torch.cat([o.reshape(-1).float() for o in out])


def test_two_calls_identical_bits_and_a_nan_does_not_stick(fixture):
    c = fixture['cap20']
    values = tuple(torch.from_numpy(c[k]).to(DEV) for k in ('fpred', 'ftgt'))
    first = flat(run_sliced(c, values=values))
    assert torch.equal(first, flat(run_sliced(c, values=values)))
    bad = (values[0].clone(), values[1])
    bad[0][int(c['rows'][3]), 5] = float('nan')
    out = run_sliced(c, values=bad)
    assert torch.isnan(out[0]).all()
    assert torch.equal(first, flat(run_sliced(c, values=values)))
    # a NaN in a row that is not selected is not read
    rest = np.setdiff1d(np.arange(128), c['rows'])
    bad = (values[0].clone(), values[1])
    bad[0][int(rest[0])] = float('nan')
    assert torch.equal(first, flat(run_sliced(c, values=bad)))
    c = fixture['iou96']
    first = flat(run_single(c))
    assert torch.equal(first, flat(run_single(c)))


def test_side_stream_beside_f16_mfma_keeps_the_solo_bits(fixture):
    c, d = fixture['trainer'], fixture['iou96']
    values = tuple(torch.from_numpy(c[k]).to(DEV) for k in ('fpred', 'ftgt'))

    def run():
        return torch.cat([flat(run_sliced(c, values=values)), flat(run_single(d))])
    ref = run().clone()
    main, side = torch.cuda.current_stream(), torch.cuda.Stream(DEV)
    scratch = torch.empty(256 * 256, device=DEV)
    torch.cuda.synchronize()
    outs = []
    side.wait_stream(main)
    testkit.f16_mfma_load(main, scratch)
    with torch.cuda.stream(side):
        for _ in range(20):
            outs.append(run())
    torch.cuda.synchronize()
    assert sum(0 if torch.equal(o, ref) else 1 for o in outs) == 0


def test_the_sliced_loss_never_waits_for_the_host(fixture):
    from rfuse.losses import AttnContrastiveLoss
    c = fixture['trainer']
    acl = AttnContrastiveLoss(0.05, 1280)
    fpred, ftgt = (torch.from_numpy(c[k]).to(DEV).requires_grad_(True) for k in ('fpred', 'ftgt'))
    occ = torch.from_numpy(c['occ']).to(DEV)
    acl(8, fpred, ftgt, occ).sum().backward()          # first use: the library is loaded, the allocator warm
    fpred.grad = ftgt.grad = None
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = acl(8, fpred, ftgt, occ)
        (loss * 0.01).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert slr.within(loss.item(), c['loss_f32'], c['loss_f64'], 'trainer loss under sync debug')
    assert acl.last_counts.tolist() == c['counts'].tolist() and fpred.grad is not None


def cosine_of(pairs):
    dot = n1 = n2 = 0.0
    for g, ref in pairs:
        g, ref = g.detach().cpu().double(), ref.detach().double()
        dot, n1, n2 = dot + float((g * ref).sum()), n1 + float((g * g).sum()), n2 + float((ref * ref).sum())
    return dot / np.sqrt(n1 * n2)


def test_get_features_trains_through_the_contrastive_loss():
    """PatchedAttentionBlock.get_features in grad mode (phase 2 of the reference's schedule, trainer/train_refinement.py:66-72, 101-106): C1's attention block
    with seeded weights, 2 x 64 patches in 16 slices, AttnContrastiveLoss on top; against oracle.refpath.patched_get_features plus the float64 restatement.
    Loss within 1e-4 relative, cosine over all gradients (the two inputs and the theta / phi parameters) > 0.9999: the bounds of tests/test_autograd_gpu.py.
    (With the in-place normalisation the encoders' saved outputs were overwritten and the normalisation had no backward.)"""
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    import model
    from rfuse.losses import AttnContrastiveLoss
    cfg = rf_configs.get_config('C1')
    with contextlib.redirect_stdout(io.StringIO()):
        block = model.get_attention_block(cfg)
    sd = helpers.seeded_sd({n: tuple(v.shape) for n, v in block.state_dict().items()}, 8101)
    block.load_state_dict(sd)
    block.to(DEV).train()
    gen = torch.Generator().manual_seed(33)
    nf = cfg['nf']
    x_back, x_target = torch.randn(2, nf, 8, 8, 8, generator=gen), torch.randn(2, nf, 8, 8, 8, generator=gen)
    occ = torch.rand(2, 1, 8, 8, 8, generator=gen) < 0.1
    xb, xt = x_back.to(DEV).requires_grad_(True), x_target.to(DEV).requires_grad_(True)
    acl = AttnContrastiveLoss(0.05)
    fpred, ftgt, occ_flat = block.get_features(xb, xt, occ.to(DEV))
    assert fpred.shape == ftgt.shape == (128, 32) and occ_flat.shape == (128,) and occ_flat.dtype == torch.bool and fpred.requires_grad and ftgt.requires_grad
    loss = acl(16, fpred, ftgt, occ_flat)
    loss.sum().backward()

    dt = torch.float64
    sdo = {n: v.detach().clone().to(dt).requires_grad_(True) for n, v in sd.items()}
    xbo, xto = x_back.to(dt).requires_grad_(True), x_target.to(dt).requires_grad_(True)
    fo, to, oo = refpath.patched_get_features(xbo, xto, occ, sdo, cfg)
    assert torch.equal(oo, occ_flat.cpu())
    lo, counts = cr.sliced(16, fo, to, oo, 0.05)
    lo.backward()
    print('\nget_features: loss %.7f, oracle %.7f; counts %s vs %s' % (loss.item(), lo.item(), acl.last_counts.tolist(), list(counts)))
    assert acl.last_counts.tolist() == list(counts) and counts[2] >= 8
    assert abs(loss.item() - lo.item()) < 1e-4 * abs(lo.item())
    pairs = [(xb.grad, xbo.grad), (xt.grad, xto.grad)]
    for name, p in block.named_parameters():
        if sdo[name].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0
            continue
        assert ('theta' in name or 'phi' in name) and p.grad is not None, name
        pairs.append((p.grad, sdo[name].grad))
    assert len(pairs) == 2 + 16
    cos = cosine_of(pairs)
    print('get_features: cosine over all gradients %.8f; of the inputs alone %.8f' % (cos, cosine_of(pairs[:2])))
    assert cos > 0.9999 and cosine_of(pairs[:2]) > 0.9999


def test_one_full_phase_step_with_the_contrastive_term_like_the_oracle():
    """tests/test_shape_loss_gpu.py::test_forward_full_trains_on_the_shape_loss_like_the_oracle's graph (C1, B = 1) extended to the full phase's objective
    (trainer/train_refinement.py:74-84, 108-120): the target through the retrieval backbone, get_features(x_back, x_target, occupancy) with an explicit seeded
    occupancy on both sides, total = shape loss of the fused prediction + 0.01 * contrastive.  Same two bounds against the float64 oracle."""
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    import model
    from model.attention import Unfold3D, Fold3D
    from rfuse.losses import ShapeLoss, AttnContrastiveLoss
    gpu = DEV
    cfg = rf_configs.get_config('C1')
    _, trunc_t = rf_configs.truncations(cfg)
    d = cfg['dataset_train']
    with contextlib.redirect_stdout(io.StringIO()):
        mods = {'unet_backbone': model.get_unet_backbone(cfg), 'decoder': model.get_decoder(cfg),
                'retrieval_backbone': model.get_retrieval_backbone(cfg), 'patched_attention_block': model.get_attention_block(cfg)}
    sds = {k: helpers.seeded_sd({n: tuple(v.shape) for n, v in m.state_dict().items()}, 7000 + i) for i, (k, m) in enumerate(mods.items())}
    for k, m in mods.items():
        m.load_state_dict(sds[k])
        m.to(gpu).train()
    gen = torch.Generator().manual_seed(21)
    K, B = cfg['K'], 1
    s_in = d['input_chunk_size']
    x_in = torch.randn(B, 1, s_in, s_in, s_in, generator=gen)
    retr = torch.randn(B, K, 64, 64, 64, generator=gen)
    raw = torch.rand(B, 1, 64, 64, 64, generator=gen) * trunc_t
    target = ((raw - np.float32(d['target_mean'])) / np.float32(d['target_std'])).float()
    noise = -torch.empty(B * 4096, K).exponential_(generator=gen).log() * 4.0 if cfg['attn_retrieval_mode'] else None
    occ = torch.rand(B, 1, 32, 32, 32, generator=gen) < 0.035          # about a quarter of the 2^3 patches: 8 slices of ~128 rows

    sl, acl = ShapeLoss.from_config(cfg), AttnContrastiveLoss(0.05)
    batch = {'target': target.to(gpu)}
    sl.augment_batch_data(batch)
    x_back = mods['unet_backbone'](x_in.to(gpu))
    feats = mods['retrieval_backbone'](Unfold3D(16, 1)(retr.reshape(B * K, 1, 64, 64, 64).to(gpu)))
    x_retr = Fold3D(4, 8, cfg['nf'])(feats)
    x_target = Fold3D(4, 8, cfg['nf'])(mods['retrieval_backbone'](Unfold3D(16, 1)(batch['target'])))
    x_attn = mods['patched_attention_block'](x_back, x_retr, noise.to(gpu) if noise is not None else None)
    shape_loss, _, _ = sl.loss_shape(mods['decoder'](x_attn), batch)
    fpred, ftgt, occ_flat = mods['patched_attention_block'].get_features(x_back, x_target, occ.to(gpu))
    contrastive = acl(B * 8, fpred, ftgt, occ_flat)
    loss = shape_loss + 0.01 * contrastive
    assert loss.shape == (1,)
    loss.sum().backward()

    dt = torch.float64
    sdo = {k: {n: v.detach().clone().to(dt).requires_grad_(True) for n, v in sd.items()} for k, sd in sds.items()}
    torch.set_num_threads(32)
    stages = {}
    dfo = refpath.forward_full(sdo, cfg, x_in.to(dt), retr.to(dt), trunc_t, noise.to(dt) if noise is not None else None, stages=stages)
    lo_shape, _, _, _ = slr.loss(dfo * 2 / trunc_t - 1, target.to(dt), trunc_t, d['target_mean'], d['target_std'])
    xto = refpath.fold3d(refpath.retrieval_backbone(refpath.unfold3d(target.to(dt), 16), sdo['retrieval_backbone'], cfg), 4, 8, cfg['nf'])
    fo, to, oo = refpath.patched_get_features(stages['x_back'], xto, occ, sdo['patched_attention_block'], cfg)
    assert torch.equal(oo, occ_flat.cpu())
    lo_c, counts = cr.sliced(B * 8, fo, to, oo, 0.05)
    lo = lo_shape + 0.01 * lo_c
    lo.backward()
    got_counts = acl.last_counts.tolist()
    print('\nC1 full phase: loss %.6f (shape %.6f, contrastive %.6f); oracle %.6f (%.6f, %.6f); counts %s vs %s' % (
        loss.item(), shape_loss.item(), contrastive.item(), lo.item(), lo_shape.item(), lo_c.item(), got_counts, list(counts)))
    assert got_counts == list(counts) and counts[2] >= 1
    assert abs(contrastive.item() - lo_c.item()) < 1e-4 * abs(lo_c.item())
    assert abs(loss.item() - lo.item()) < 1e-4 * abs(lo.item())
    pairs = []
    for k, m in mods.items():
        for name, p in m.named_parameters():
            ref = sdo[k][name].grad
            if ref is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0
                continue
            pairs.append((p.grad, ref))
    cos = cosine_of(pairs)
    print('C1 full phase: cosine over all parameter gradients %.8f' % cos)
    assert cos > 0.9999
