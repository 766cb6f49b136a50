"""Module level: the reference's retrieval training step (trainer/train_retrieval.py:73-87 -- both patch encoders forward, normalise, NT-Xent(0.2,
cosine), backward; Adam with weight decay 5e-5, :37) on the drop-in ``model`` package, against float64 CPU autograd of the same nets.  Encoder pairs
of C2, C4 and C5 and the base surface-reconstruction pair (PCPatch48 nf 10 / Patch24 nf 12) at their real window sizes."""
import pytest
import torch
import torch.nn.functional as F

import helpers
from oracle import refpath

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# name -> (query class, nf, window), (target class, nf, window)
PAIRS = {
    'C2': (('Patch04', 32, 4), ('Patch32', 8, 32)),
    'C4': (('Patch08', 16, 8), ('Patch32', 8, 32)),
    'C5': (('PCPatch48', 12, 48), ('Patch24V2', 12, 24)),
    'base_sr': (('PCPatch48', 10, 48), ('Patch24', 12, 24)),
}
Z = 64


@pytest.fixture(scope='module')
def model():
    if not torch.cuda.is_available():
        pytest.skip('needs the GPU')
    import model as m
    return m


def spec_embed(cls, x, sd):
    """float64 oracle of a conv patch encoder built from its SPEC (Patch24 shares PCPatch48's kernel-size sequence, so refpath cannot tell them apart)"""
    for j, (_, _, k, stride) in enumerate(cls.SPEC):
        x = F.leaky_relu(F.conv3d(x, sd['layers.%d.weight' % (2 * j)], sd['layers.%d.bias' % (2 * j)], stride=stride), 0.2)
    return F.linear(x.reshape(x.shape[0], -1), sd['final_layer.weight'], sd['final_layer.bias'])


def oracle_embed(name, x, sd):
    if name == 'Patch04':
        return refpath.patch04_embed(x, sd)
    if name == 'Patch24':
        from model import retrieval
        return spec_embed(retrieval.Patch24, x, sd)
    return refpath.conv_patch_embed(x, sd)


def make_pair(model, pair, seed):
    from model import retrieval
    nets = []
    for i, (name, nf, win) in enumerate(PAIRS[pair]):
        net = getattr(retrieval, name)(nf, Z)
        sd = helpers.seeded_sd({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed + i)
        net.load_state_dict(sd)
        nets.append((name, net.to(DEV), sd, win))
    return nets


def inputs(b, win, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(b, 1, win, win, win, generator=g) * 2.0 - 1.0).clamp_(-0.8, 1.0)    # a truncated distance field's range


def iou_matrix(b, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(b, b, generator=g)
    m = 0.5 * (m + m.t())
    m.fill_diagonal_(1.0)
    return m.repeat(2, 2)


def step_loss(zq, zt, iou, loss_mod):
    zq, zt = F.normalize(zq.reshape(zq.shape[0], -1), dim=1), F.normalize(zt.reshape(zt.shape[0], -1), dim=1)
    return loss_mod(zq, zt, iou)


def float64_step(nets, xs, iou, loss_mod, dtype=torch.float64):
    params, outs = [], []
    for (name, _, sd, _), x in zip(nets, xs):
        p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        params.append(p)
        outs.append(oracle_embed(name, x.to(dtype), p))
    loss = step_loss(outs[0], outs[1], None if iou is None else iou.to(dtype), loss_mod)
    loss.backward()
    return loss.detach(), [{k: v.grad for k, v in p.items()} for p in params]


def gpu_step(nets, xs, iou, loss_mod):
    for _, net, _, _ in nets:
        net.zero_grad(set_to_none=True)
    zq, zt = (net(x.to(DEV)) for (_, net, _, _), x in zip(nets, xs))
    loss = step_loss(zq, zt, None if iou is None else iou.to(DEV), loss_mod)
    loss.backward()
    return loss.detach().cpu(), [{k: p.grad.detach().cpu() for k, p in net.named_parameters()} for _, net, _, _ in nets]


def check_grads(gpu, ref64, ref32, what):
    num = den = dot = 0.0
    for g_net, r_net, f_net in zip(gpu, ref64, ref32):
        for key in r_net:
            g, r, f = g_net[key].double(), r_net[key], f_net[key].double()
            scale = float(r.abs().max().clamp_min(1e-30))
            err, err32 = float((g - r).abs().max()) / scale, float((f - r).abs().max()) / scale
            assert err <= max(1e-3, 10 * err32), (what, key, err, err32)
            dot += float((g * r).sum())
            num += float((g * g).sum())
            den += float((r * r).sum())
    cos = dot / (num * den) ** 0.5
    assert cos > 0.99999, (what, cos)


@pytest.mark.parametrize('with_iou', [False, True])
@pytest.mark.parametrize('pair,b', [('C2', 24), ('C4', 16), ('C5', 16), ('base_sr', 16)])
def test_step_matches_float64(model, pair, b, with_iou):
    from model.loss import NTXentLoss
    loss_mod = NTXentLoss(0.2, True)
    nets = make_pair(model, pair, seed=100 + b)
    xs = [inputs(b, win, seed=7 + i) for i, (_, _, _, win) in enumerate(nets)]
    iou = iou_matrix(b, 3) if with_iou else None
    loss, grads = gpu_step(nets, xs, iou, loss_mod)
    rloss, rgrads = float64_step(nets, xs, iou, loss_mod)
    _, fgrads = float64_step(nets, xs, iou, loss_mod, dtype=torch.float32)
    assert abs(float(loss) - float(rloss)) / abs(float(rloss)) < 1e-5, (float(loss), float(rloss))
    check_grads(grads, rgrads, fgrads, pair)


def test_c5_step_at_train_batch(model):
    from model.loss import NTXentLoss
    loss_mod = NTXentLoss(0.2, True)
    nets = make_pair(model, 'C5', seed=500)
    xs = [inputs(128, win, seed=17 + i) for i, (_, _, _, win) in enumerate(nets)]
    loss, grads = gpu_step(nets, xs, None, loss_mod)
    rloss, rgrads = float64_step(nets, xs, None, loss_mod)
    _, fgrads = float64_step(nets, xs, None, loss_mod, dtype=torch.float32)
    assert abs(float(loss) - float(rloss)) / abs(float(rloss)) < 1e-5
    check_grads(grads, rgrads, fgrads, 'C5 B=128')


@pytest.mark.parametrize('pair', list(PAIRS))
def test_grad_mode_forward_matches_no_grad(model, pair):
    nets = make_pair(model, pair, seed=40)
    for i, (name, net, _, win) in enumerate(nets):
        x = inputs(8, win, seed=60 + i).to(DEV)
        with torch.no_grad():
            ref = net(x)
        got = net(x)
        assert got.requires_grad
        err = float((got.detach() - ref).abs().max() / ref.abs().max())
        assert err < 2e-6, (pair, name, err)


def cpu_adam(nets, xs, loss_mod, dtype, steps):
    ref = [{k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()} for _, _, sd, _ in nets]
    opt = torch.optim.Adam([p for sd in ref for p in sd.values()], lr=1e-4, weight_decay=5e-5)
    for _ in range(steps):
        opt.zero_grad()
        outs = [oracle_embed(name, x.to(dtype), p) for (name, _, _, _), x, p in zip(nets, xs, ref)]
        step_loss(outs[0], outs[1], None, loss_mod).backward()
        opt.step()
    return ref


@pytest.mark.parametrize('pair', ['C4', 'C5'])
def test_adam_steps_track_float64(model, pair):
    """three Adam steps track the float64 run: every parameter within max(1e-5, 10x the distance of torch's fp32 CPU run) -- Adam divides by sqrt(v),
    so an element whose gradient is near zero moves by up to lr whatever its size and an fp32-sized gradient error there becomes an update error of
    a few 1e-6 (1e-5 = 3 % of the 3 lr the steps travel) -- and the update of all parameters together within 1 % (L2) of float64's"""
    from model.loss import NTXentLoss
    loss_mod = NTXentLoss(0.2, True)
    nets = make_pair(model, pair, seed=900)
    b = 16
    xs = [inputs(b, win, seed=31 + i) for i, (_, _, _, win) in enumerate(nets)]
    opt = torch.optim.Adam([p for _, net, _, _ in nets for p in net.parameters()], lr=1e-4, weight_decay=5e-5)
    for _ in range(3):
        opt.zero_grad()
        zq, zt = (net(x.to(DEV)) for (_, net, _, _), x in zip(nets, xs))
        step_loss(zq, zt, None, loss_mod).backward()
        opt.step()
    ref64, ref32 = cpu_adam(nets, xs, loss_mod, torch.float64, 3), cpu_adam(nets, xs, loss_mod, torch.float32, 3)
    du2 = u2 = 0.0
    for (name, net, sd, _), p64, p32 in zip(nets, ref64, ref32):
        for key, v in net.named_parameters():
            r = p64[key].detach()
            moved = float((r - sd[key].double()).abs().max())
            assert moved > 1e-5, (pair, name, key, moved)                             # the steps did move it
            d = v.detach().cpu().double() - r
            diff = float(d.abs().max())
            diff32 = float((p32[key].detach().double() - r).abs().max())
            assert diff <= max(1e-5, 10 * diff32), (pair, name, key, diff, diff32, moved)
            du2 += float((d * d).sum())
            u2 += float(((r - sd[key].double()) ** 2).sum())
    assert (du2 / u2) ** 0.5 < 1e-2, (pair, (du2 / u2) ** 0.5)


def test_inference_only_routes_still_raise(model):
    from model import retrieval
    for cls in (retrieval.PatchNorm08, retrieval.PatchNorm32):
        net = cls(8, Z).to(DEV)
        win = 8 if cls is retrieval.PatchNorm08 else 32
        with pytest.raises(NotImplementedError):
            net(torch.zeros(2, 1, win, win, win, device=DEV, requires_grad=True))
    net = retrieval.Patch08(16, Z).to(DEV)
    with pytest.raises(NotImplementedError):
        net.forward_grid(torch.zeros(1, 1, 16, 16, 16, device=DEV), 8, 8)
