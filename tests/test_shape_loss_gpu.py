"""GPU: the shape loss (rfuse/losses.py, csrc/shape_loss.hip) against tests/golden/shape_loss.npz, the record of the reference's own
augment_batch_data / loss_shape / compute_normals in float32 and in float64 (tools/gen_shape_loss_golden.py).

Tolerance rule (shape_loss_ref.within): with err_hip = |x_hip - x_f64| and err_ref = |x_ref32 - x_f64|, both against the fixture's float64 record,
err_hip <= max(2 * err_ref, floor); floor = 4 float32 ulps of |x_f64| for a scalar, and for a tensor 4 ulps of max |x_f64| with max-abs errors.  The factor 2
allows another float32 evaluation order; the error of the gradient is dominated by the 1 / |g| amplification at voxels with a small Sobel gradient, which
every float32 evaluation shares.  err_ref as the generator printed it (relative; tensors: of max |x_f64|):
    sn16   total 6.0e-8  l1 3.1e-8  normal 2.9e-7   grad 1.7e-5  normals 1.2e-7
    odd    total 3.3e-8  l1 9.5e-8  normal 6.9e-8   grad 1.4e-6  normals 1.3e-7
    mp16   total 4.2e-8  l1 2.3e-8  normal 8.2e-7   grad 6.6e-6  normals 8.2e-8
    tiny   total 5.8e-8  l1 7.7e-8  normal 4.3e-6   grad 6.5e-8  normals 6.9e-8
Masks, counts and exact-zero patterns are compared exactly."""
import contextlib
import io

import numpy as np
import pytest
import torch

import helpers
import shape_loss_ref as slr
import testkit
from oracle import refpath
from rfuse import configs as rf_configs

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CASES = ['sn16', 'odd', 'mp16', 'tiny', 'flat4', 'flat1']


@pytest.fixture(scope='module')
def fixture(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    return slr.load_fixture(golden_dir)


def setup(c, lam_rec=None, lam_n=None, grad=True):
    from rfuse.losses import ShapeLoss
    trunc, mean, std, w_occ, f_rec, f_n = (float(x) for x in c['params'])
    sl = ShapeLoss(trunc, mean, std, weight_occupied=int(w_occ), loss_reconstruction=f_rec if lam_rec is None else lam_rec,
                   loss_normal=f_n if lam_n is None else lam_n)
    batch = {'target': torch.from_numpy(c['target']).to(DEV)}
    sl.augment_batch_data(batch)
    pred = torch.from_numpy(c['pred']).to(DEV).requires_grad_(grad)
    return sl, batch, pred


def formula(c, a, b):
    trunc, mean, std, w_occ = (float(x) for x in c['params'][:4])
    return slr.grad_by_formula(torch.from_numpy(c['pred']).double(), torch.from_numpy(c['target']).double(), trunc, mean, std, w_occ, a, b).numpy()


@pytest.mark.parametrize('name', CASES)
def test_augment_batch_data_matches_the_fixture(fixture, name):
    c = fixture[name]
    sl, batch, _ = setup(c)
    assert batch['weights'].dtype == torch.float32 and batch['empty'].dtype == torch.bool and batch['normals'].dtype == torch.float32
    assert batch['weights'].shape == batch['empty'].shape == batch['target'].shape and batch['normals'].shape == c['normals_f32'].shape
    np.testing.assert_array_equal(batch['weights'].cpu().numpy(), c['weights_f32'])
    np.testing.assert_array_equal(batch['empty'].cpu().numpy(), c['empty'])
    normals = batch['normals'].cpu().numpy()
    np.testing.assert_array_equal(normals == 0, c['normals_f32'] == 0)
    if np.abs(c['normals_f64']).max() > 0:
        assert slr.within(normals, c['normals_f32'], c['normals_f64'], name + ' normals')
    # compute_normals on the denormalised target is the same launch with scale 1, shift 0
    den = batch['target'] * np.float32(c['params'][2]) + np.float32(c['params'][1])
    assert torch.equal(sl.compute_normals(den), batch['normals'])


@pytest.mark.parametrize('name', CASES)
def test_loss_shape_scalars_counts_and_gradient(fixture, name):
    c = fixture[name]
    sl, batch, pred = setup(c)
    total, l1, normal = sl.loss_shape(pred, batch)
    assert total.shape == l1.shape == normal.shape == () and total.dtype == torch.float32 and total.device == pred.device
    total.backward()
    got = np.array([total.item(), l1.item(), normal.item()])
    np.testing.assert_array_equal(sl.last_counts.cpu().numpy(), c['counts'])
    grad = pred.grad.cpu().numpy()
    assert slr.within(got[1], c['scalars_f32'][1], c['scalars_f64'][1], name + ' l1')
    if c['counts'][0] == 0:                       # no valid voxel: NaN like the reference, and the gradient is the L1 part alone
        assert np.isnan(got[[0, 2]]).all() and np.isnan(c['scalars_f32'][[0, 2]]).all()
        assert np.isfinite(grad).all()
        np.testing.assert_array_equal(grad, c['grad_f32'])
    else:
        assert slr.within(got[0], c['scalars_f32'][0], c['scalars_f64'][0], name + ' total')
        assert slr.within(got[2], c['scalars_f32'][2], c['scalars_f64'][2], name + ' normal')
        assert slr.within(grad, c['grad_f32'], c['grad_f64'], name + ' grad')


@pytest.mark.parametrize('name', ['sn16', 'odd'])
def test_upstream_gradient_combinations(fixture, name):
    """(total + 3 l1).backward() and the instances with one term switched off, against the written-out float64 gradient.  Bound: the normal part's error is
    the fixture's (same rule, in absolute terms; it scales with its coefficient b / 0.5), the L1 part a * sign * W' / N is one rounding away from exact."""
    c = fixture[name]
    err_ref = float(np.abs(c['grad_f32'].astype(np.float64) - c['grad_f64']).max())

    def check(grad, a, b, what):
        want = formula(c, a, b)
        err = float(np.abs(grad.cpu().numpy().astype(np.float64) - want).max())
        bound = max(2 * err_ref * b / 0.5, 4 * slr.ulp32(np.abs(want).max()))
        print('%s %s: err_hip %.3e  bound %.3e' % (name, what, err, bound))
        assert err <= bound, what

    sl, batch, pred = setup(c)
    total, l1, normal = sl.loss_shape(pred, batch)
    (total + 3 * l1).backward()
    check(pred.grad, 4.0, 0.5, 'total + 3 l1')
    sl, batch, pred = setup(c)
    total, l1, normal = sl.loss_shape(pred, batch)
    (2 * normal + l1).backward()
    check(pred.grad, 1.0, 2.0, '2 normal + l1')
    sl, batch, pred = setup(c, lam_n=0)
    total, l1, normal = sl.loss_shape(pred, batch)
    assert total.shape == (1,) and l1.shape == () and normal.shape == (1,) and normal.item() == 0 and not normal.requires_grad
    assert total.item() == l1.item() and slr.within(l1.item(), c['scalars_f32'][1], c['scalars_f64'][1], name + ' l1 alone')
    total.sum().backward()
    check(pred.grad, 1.0, 0.0, 'loss_normal = 0')
    sl, batch, pred = setup(c, lam_rec=0)
    total, l1, normal = sl.loss_shape(pred, batch)
    assert total.shape == (1,) and l1.shape == (1,) and normal.shape == () and l1.item() == 0
    assert total.item() == 0.5 * normal.item() and slr.within(normal.item(), c['scalars_f32'][2], c['scalars_f64'][2], name + ' normal alone')
    total.sum().backward()
    check(pred.grad, 0.0, 0.5, 'loss_reconstruction = 0')


def run_once(sl, batch, pred_values):
    pred = pred_values.clone().requires_grad_(True)
    total, l1, normal = sl.loss_shape(pred, batch)
    total.backward()
    return torch.cat([torch.stack([total.detach(), l1.detach(), normal.detach()]), sl.last_counts.float(), pred.grad.reshape(-1)])


def test_two_calls_identical_bits_and_a_nan_does_not_stick(fixture):
    c = fixture['sn16']
    sl, batch, pred = setup(c, grad=False)
    first = run_once(sl, batch, pred)
    assert torch.equal(first, run_once(sl, batch, pred))
    bad = pred.clone()
    bad[1, 0, 7, 9, 11] = float('nan')
    out = run_once(sl, batch, bad)
    assert torch.isnan(out[:3]).all()
    assert torch.equal(first, run_once(sl, batch, pred))


def test_side_stream_beside_f16_mfma_keeps_the_solo_bits(fixture):
    c = fixture['odd']
    sl, batch, pred = setup(c, grad=False)

    def run():
        b = {'target': batch['target']}
        sl.augment_batch_data(b)
        return torch.cat([run_once(sl, b, pred), b['normals'].reshape(-1), b['weights'].reshape(-1), b['empty'].reshape(-1).float()])
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


@pytest.mark.parametrize('cfg_name', ['C1', 'C3'])
def test_forward_full_trains_on_the_shape_loss_like_the_oracle(cfg_name):
    """tests/test_autograd_gpu.py::test_forward_full_trains_like_the_oracle's graph with ShapeLoss in place of the L1 stand-in, against oracle.refpath.forward_full in
    float64 plus the float64 restatement of the loss: loss within 1e-4 relative, cosine over all parameter gradients > 0.9999."""
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    import model
    from model.attention import Unfold3D, Fold3D
    from rfuse.losses import ShapeLoss
    gpu = DEV
    cfg = rf_configs.get_config(cfg_name)
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

    sl = ShapeLoss.from_config(cfg)
    batch = {'target': target.to(gpu)}
    sl.augment_batch_data(batch)
    x_back = mods['unet_backbone'](x_in.to(gpu))
    feats = mods['retrieval_backbone'](Unfold3D(16, 1)(retr.reshape(B * K, 1, 64, 64, 64).to(gpu)))
    x_retr = Fold3D(4, 8, cfg['nf'])(feats)
    x_attn = mods['patched_attention_block'](x_back, x_retr, noise.to(gpu) if noise is not None else None)
    loss, l1, normal = sl.loss_shape(mods['decoder'](x_attn), batch)
    loss.backward()

    dt = torch.float64
    sdo = {k: {n: v.detach().clone().to(dt).requires_grad_(True) for n, v in sd.items()} for k, sd in sds.items()}
    torch.set_num_threads(32)
    dfo = refpath.forward_full(sdo, cfg, x_in.to(dt), retr.to(dt), trunc_t, noise.to(dt) if noise is not None else None)
    # (a random target has no flat neighbourhood: a float64 convolution of a constant with a full mantissa returns rounding noise where the exact tap sum is 0,
    # and the float64 side would count such voxels as valid)
    lo, lo_l1, lo_n, counts = slr.loss(dfo * 2 / trunc_t - 1, target.to(dt), trunc_t, d['target_mean'], d['target_std'])
    lo.backward()
    got_counts = sl.last_counts.cpu().tolist()
    print(f'\n{cfg_name}: loss {loss.item():.6f} (l1 {l1.item():.6f}, normal {normal.item():.6f}); oracle {lo.item():.6f} ({lo_l1.item():.6f}, {lo_n.item():.6f});'
          f' counts {got_counts} vs {list(counts)}')
    assert abs(loss.item() - lo.item()) < 1e-4 * abs(lo.item())
    dot = n1 = n2 = 0.0
    for k, m in mods.items():
        for name, p in m.named_parameters():
            ref = sdo[k][name].grad
            if ref is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0
                continue
            g = p.grad.detach().cpu().double()
            dot, n1, n2 = dot + float((g * ref).sum()), n1 + float((g * g).sum()), n2 + float((ref * ref).sum())
    cos = dot / np.sqrt(n1 * n2)
    print(f'{cfg_name}: cosine over all parameter gradients {cos:.8f}')
    assert cos > 0.9999
