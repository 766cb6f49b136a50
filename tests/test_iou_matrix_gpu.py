"""GPU: the retrieval trainer's IoU matrix and the tail of its step (rfuse/losses.py iou_matrix / target_iou_matrix / RetrievalStepLoss,
csrc/iou_matrix.hip) against tests/golden/iou_matrix.npz, the record of the reference's own get_iou_matrix (tools/gen_iou_matrix_golden.py), and against the
count formula of tests/iou_matrix_ref.py that the fixture is checked with on the CPU.

The counts are integers and the float32 conversions, the add and the divide are correctly rounded on both sides: every matrix comparison is torch.equal,
without a tolerance.  The step loss is compared with the float64 CPU evaluation of the same step under the bounds of tests/test_retrieval_training_gpu.py
(loss relative error < 1e-5, its check_grads)."""
import numpy as np
import pytest
import torch

import iou_matrix_ref as ir
import testkit

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


@pytest.fixture(scope='module')
def fixture(golden_dir):
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    return ir.load_fixture(golden_dir)


def shapenet(c):
    mean, std, voxel = (float(x) for x in c['params'])
    return mean, std, 0.75 * voxel


def words_of(occ):
    """bool [n, ...] -> int64 [n, ceil(V / 64)]: voxel v is bit v % 64 of word v / 64, zeros past V"""
    flat = occ.reshape(occ.shape[0], -1).numpy()
    n, v = flat.shape
    padded = np.zeros((n, (v + 63) // 64 * 64), bool)
    padded[:, :v] = flat
    return torch.from_numpy(np.packbits(padded, axis=1, bitorder='little').view('<u8').astype(np.int64))


def packed(x, kind=0, scale=0.0, shift=0.0, thr=0.0):
    from rfuse import losses
    bits, counts, _ = losses._pack(x.contiguous(), kind, scale, shift, thr, x.shape[0])
    return bits.cpu(), counts.cpu()


@pytest.mark.parametrize('name', ['n1_empty', 'n1_full', 'n7_5', 'n33_12', 'n67_24', 'n5_357', 'n3_64'])
def test_matrix_equals_the_reference(fixture, name):
    from rfuse.losses import iou_matrix
    c = fixture[name]
    n = c['occ'].shape[0]
    got = iou_matrix(c['occ'].to(DEV))
    assert got.shape == (n, n) and got.dtype == torch.float32 and got.device == DEV
    assert torch.equal(got.cpu(), c['iou']), name
    bits, counts = packed(c['occ'].to(DEV))
    assert torch.equal(bits, words_of(c['occ'])), 'a bit past the last voxel, or a voxel in the wrong place'
    assert torch.equal(counts, c['occ'].reshape(n, -1).sum(1).to(torch.int32))
    if name == 'n1_empty':
        assert got.item() == 0.0
    if name == 'n1_full':
        assert got.item() == np.float32(64) / (np.float32(64) + np.float32(1e-5))


def test_other_gives_the_rectangular_block(fixture):
    from rfuse.losses import iou_matrix
    occ, full = fixture['other']['occ'], fixture['other']['iou']
    a, b = occ[:ir.OTHER_SPLIT].to(DEV), occ[ir.OTHER_SPLIT:].to(DEV)
    got = iou_matrix(a, b)
    assert got.shape == (5, 19) and torch.equal(got.cpu(), full[:5, 5:])
    assert torch.equal(iou_matrix(b, a).cpu(), full[5:, :5]) and not torch.equal(full[:5, 5:10], full[:5, 5:10].t())
    assert torch.equal(iou_matrix(a, b, repeat=2).cpu(), full[:5, 5:].repeat(2, 2))


def test_repeat_2_from_float_targets(fixture):
    from rfuse.losses import iou_matrix, target_iou_matrix
    c = fixture[ir.FLOAT_CASE]
    mean, std, thr = shapenet(c)
    target = c['target'].to(DEV)
    got = target_iou_matrix(target, mean, std, thr)
    assert got.shape == (40, 40) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), c['iou'])
    occ = ir.occupied(c['target'], mean, std, thr)
    once = iou_matrix(occ.to(DEV))
    assert torch.equal(got, once.repeat(2, 2)) and torch.equal(target_iou_matrix(target, mean, std, thr, repeat=1), once)
    assert torch.equal(iou_matrix(occ.to(DEV), repeat=2), got)
    with pytest.raises(ValueError, match='repeat is 1 or 2'):
        iou_matrix(occ.to(DEV), repeat=3)


def test_uint8_grid_non_zero_is_occupied():
    from rfuse.losses import iou_matrix
    g = torch.Generator().manual_seed(5)
    grid = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, (9, 1, 7, 6, 5), generator=g)]
    assert set(grid.unique().tolist()) == {0, 1, 2, 255}
    assert torch.equal(iou_matrix(grid.to(DEV)).cpu(), ir.count_formula(grid.bool()))
    assert torch.equal(iou_matrix(grid.to(DEV)), iou_matrix(grid.bool().to(DEV)))


def test_non_finite_targets():
    """NaN is unoccupied, -inf occupied, +inf unoccupied: torch's own float32 expression on the CPU decides"""
    from rfuse.losses import target_iou_matrix
    g = torch.Generator().manual_seed(6)
    target = torch.randn(6, 1, 8, 8, 8, generator=g) * 3 - 3
    special = torch.tensor([float('nan'), float('inf'), float('-inf')])[torch.randint(0, 3, target.shape, generator=g)]
    target = torch.where(torch.rand(target.shape, generator=g) < 0.3, special, target)
    mean, std, thr = 0.059954833543534335, 0.010110036361741626, 0.75 * 0.020834
    occ = ir.occupied(target, mean, std, thr)
    assert occ[target == float('-inf')].all() and not occ[torch.isnan(target)].any() and not occ[target == float('inf')].any()
    bits, counts = packed(target.to(DEV), 1, np.float32(std).item(), np.float32(mean).item(), np.float32(thr).item())
    assert torch.equal(bits, words_of(occ))
    assert torch.equal(target_iou_matrix(target.to(DEV), mean, std, thr, repeat=1).cpu(), ir.count_formula(occ))


@pytest.mark.parametrize('mean,std,thr', [(0.3, 0.7, 1.25), (0.3, 0.7, 1.0), (0.059954833543534335, 0.010110036361741626, 0.75 * 0.020834)])
def test_targets_on_the_threshold(mean, std, thr):
    """32768 consecutive float32 values around (thr - mean) / std, shuffled over 64 windows of 8^3.  With the first constants x * std + mean lands exactly on
    thr, one ulp below and one ulp above it, and a double-precision evaluation puts a voxel on the other side; with the second a fused multiply-add does;
    the third are the ShapeNet constants."""
    from rfuse.losses import target_iou_matrix
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    x0 = ((f32(thr) - f32(mean)) / f32(std)).reshape(1)
    start = x0.view(torch.int32).item() - 16384 * (1 if x0.item() > 0 else -1)
    step = 1 if x0.item() > 0 else -1                                   # increasing value
    x = torch.arange(start, start + 32768 * step, step, dtype=torch.int32).view(torch.float32)
    assert bool((x[1:] > x[:-1]).all())
    y = x * std + mean                                                  # torch's float32 expression, Python scalars
    t = f32(thr)
    if thr == 1.25:
        below, above = torch.nextafter(t, f32(-1e30)), torch.nextafter(t, f32(1e30))
        assert (y == t).any() and (y == below).any() and (y == above).any()
        assert ((x.double() * std + mean <= thr) != (y <= t)).any()
    if thr == 1.0:
        fused = (x.double() * f32(std).double() + f32(mean).double()).float()          # one rounding instead of two
        assert ((fused <= t) != (y <= t)).any()
    target = x[torch.randperm(32768, generator=torch.Generator().manual_seed(7))].reshape(64, 1, 8, 8, 8)
    occ = ir.occupied(target, mean, std, thr)
    assert 0.3 < occ.float().mean() < 0.7
    bits, counts = packed(target.to(DEV), 1, f32(std).item(), f32(mean).item(), f32(thr).item())
    assert torch.equal(bits, words_of(occ))
    assert torch.equal(target_iou_matrix(target.to(DEV), mean, std, thr, repeat=1).cpu(), ir.count_formula(occ))


def run_all(c):
    from rfuse.losses import iou_matrix, target_iou_matrix
    mean, std, thr = shapenet(c[ir.FLOAT_CASE])
    return torch.cat([target_iou_matrix(c[ir.FLOAT_CASE]['dev'], mean, std, thr).reshape(-1), iou_matrix(c['n67_24']['dev']).reshape(-1),
                      iou_matrix(c['other']['dev'][:5], c['other']['dev'][5:]).reshape(-1)])


@pytest.fixture(scope='module')
def on_device(fixture):
    c = {k: dict(v) for k, v in fixture.items()}
    for k in ('n67_24', 'other'):
        c[k]['dev'] = c[k]['occ'].to(DEV)
    c[ir.FLOAT_CASE]['dev'] = c[ir.FLOAT_CASE]['target'].to(DEV)
    return c


def test_two_calls_give_the_same_bits(on_device):
    first = run_all(on_device)
    assert torch.equal(first, run_all(on_device))
    want = torch.cat([on_device[ir.FLOAT_CASE]['iou'].reshape(-1), on_device['n67_24']['iou'].reshape(-1), on_device['other']['iou'][:5, 5:].reshape(-1)])
    assert torch.equal(first.cpu(), want)


def test_side_stream_beside_f16_mfma_keeps_the_solo_bits(on_device):
    ref = run_all(on_device).clone()
    main, side = torch.cuda.current_stream(), torch.cuda.Stream(DEV)
    scratch = torch.empty(256 * 256, device=DEV)
    torch.cuda.synchronize()
    outs = []
    side.wait_stream(main)
    testkit.f16_mfma_load(main, scratch)
    with torch.cuda.stream(side):
        for _ in range(20):
            outs.append(run_all(on_device))
    torch.cuda.synchronize()
    assert sum(0 if torch.equal(o, ref) else 1 for o in outs) == 0


def test_the_matrix_never_waits_for_the_host(on_device):
    ref = run_all(on_device)                         # first use: the library is loaded, the allocator warm
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        got = run_all(on_device)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert torch.equal(got, ref)


def test_ntxent_takes_the_device_matrix_bit_for_bit(fixture):
    from rfuse.losses import NTXent, target_iou_matrix
    c = fixture[ir.FLOAT_CASE]
    mean, std, thr = shapenet(c)
    g = torch.Generator().manual_seed(8)
    zjs0 = torch.randn(20, 64, generator=g)
    zis0 = zjs0 + 0.5 * torch.randn(20, 64, generator=g)

    def run(iou):
        zis, zjs = zis0.to(DEV).requires_grad_(True), zjs0.to(DEV).requires_grad_(True)
        loss = NTXent(0.2)(zis, zjs, iou)
        loss.backward()
        return loss.detach(), zis.grad, zjs.grad
    got, want, plain = run(target_iou_matrix(c['target'].to(DEV), mean, std, thr)), run(c['iou'].to(DEV)), run(None)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(got[0], plain[0])         # the matrix does act on the loss


def shell_targets(b, win, seed):
    """normalised ShapeNet targets: truncated distances to spherical shells, occupancies from a few voxels to about a third of the window.  Windows 2k and
    2k + 1 are the same shell but for a sixth of a voxel of radius: pairs with an IoU near 1, where sigmoid(80 iou - 65) raises the temperature"""
    mean, std, voxel = 0.059954833543534335, 0.010110036361741626, 0.020834
    g = torch.Generator().manual_seed(seed)
    ax = (torch.arange(win, dtype=torch.float64) + 0.5) / win * 2 - 1
    x = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1)
    out = torch.empty(b, 1, win, win, win, dtype=torch.float32)
    for i in range(b):
        if i % 2 == 0:
            centre = torch.rand(3, generator=g, dtype=torch.float64) * 0.8 - 0.4
            radius, width = 0.05 + 0.85 * i / (b - 2), 0.5 + 5.5 * float(torch.rand((), generator=g))
        else:
            radius = radius + 1.0 / (3 * win)
        raw = ((x - centre).norm(dim=-1) - radius).abs() * voxel * (win / 2) / width
        out[i, 0] = ((raw.clamp(max=3 * voxel) - mean) / std).float()
    return out, mean, std, voxel


@pytest.mark.parametrize('pair', ['C2', 'C5'])
def test_step_loss_matches_float64(pair):
    """RetrievalStepLoss on the encoder pairs of tests/test_retrieval_training_gpu.py at b = 16 against the float64 CPU evaluation of the same step:
    model.loss.NTXentLoss on the normalised features with the IoU matrix of the count formula, repeated (2, 2)."""
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    import model
    import test_retrieval_training_gpu as rt
    from model.loss import NTXentLoss
    from rfuse.losses import NTXent, RetrievalStepLoss
    b = 16
    loss_mod = NTXentLoss(0.2, True)
    nets = rt.make_pair(model, pair, seed=100 + b)
    target, mean, std, voxel = shell_targets(b, nets[1][3], seed=9)
    xs = [rt.inputs(b, nets[0][3], seed=7), target]
    occ = ir.occupied(target, mean, std, 0.75 * voxel)
    frac = occ.reshape(b, -1).float().mean(1)
    assert frac.min() > 0 and frac.max() > 0.2 and frac.max() / frac.min() > 20, frac          # a real spread of occupancies
    iou = ir.count_formula(occ).repeat(2, 2)
    near = iou[:b, :b].clone().fill_diagonal_(0)
    assert (near > 0.85).sum() >= 8 and near.max() < 1.0 and (near < 0.5).sum() > b * b // 2          # pairs that overlap, and pairs that do not

    step = RetrievalStepLoss(0.2, mean, std, voxel)
    for _, net, _, _ in nets:
        net.zero_grad(set_to_none=True)
    fi, ft = (net(x.to(DEV)) for (_, net, _, _), x in zip(nets, xs))
    total, contrastive = step(fi, ft, xs[1].to(DEV))
    assert total.shape == contrastive.shape == () and total.dtype == torch.float32 and torch.equal(total, contrastive)
    total.backward()
    grads = [{k: p.grad.detach().cpu() for k, p in net.named_parameters()} for _, net, _, _ in nets]
    rloss, rgrads = rt.float64_step(nets, xs, iou, loss_mod)
    _, fgrads = rt.float64_step(nets, xs, iou, loss_mod, dtype=torch.float32)
    print('\n%s: step loss %.8f, float64 %.8f (relative %.2e)' % (pair, float(total.detach()), float(rloss), abs(float(total.detach()) - float(rloss)) / abs(float(rloss))))
    assert abs(float(total.detach()) - float(rloss)) / abs(float(rloss)) < 1e-5, (float(total.detach()), float(rloss))
    rt.check_grads(grads, rgrads, fgrads, pair)

    # without iou_scaling: the plain NTXent call, bit for bit; weight 0: zeros(1) for both, as the reference returns them
    with torch.no_grad():
        off = RetrievalStepLoss(0.2, mean, std, voxel, iou_scaling=False)(fi, ft, xs[1].to(DEV))
        plain = NTXent(0.2)(RetrievalStepLoss.reshape_features(fi), RetrievalStepLoss.reshape_features(ft))
        assert torch.equal(off[0], plain) and torch.equal(off[1], plain)
        assert abs(float(plain) - float(contrastive)) > 1e-4 * abs(float(plain))               # the matrix does act on this step
        half = RetrievalStepLoss(0.2, mean, std, voxel, contrastive_weight=0.5)(fi, ft, xs[1].to(DEV))
        assert torch.equal(half[1], contrastive.detach()) and torch.equal(half[0], contrastive.detach() * 0.5)
        zero = RetrievalStepLoss(0.2, mean, std, voxel, contrastive_weight=0)(fi, ft, xs[1].to(DEV))
        for z in zero:
            assert z.shape == (1,) and z.dtype == torch.float32 and z.device == fi.device and not z.any()
        # code noise acts on a training step only
        noisy = RetrievalStepLoss(0.2, mean, std, voxel, code_noise=0.05)
        assert torch.equal(noisy(fi, ft, xs[1].to(DEV))[1], contrastive.detach())
        assert not torch.equal(noisy(fi, ft, xs[1].to(DEV), train=True)[1], contrastive.detach())
