"""Everything a layer DERIVES from its parameters follows them: the eleven ops.PackedWeight operand images and ops.PackedAttnMLP, the cached max |t| behind
ops.split_range_ok (split-operand forms or fp32 kernels), the ordering of a pack before readers on other streams, and PatchDatabase.feature_cache.

The matrix (test_packed_image_follows_its_parameters) runs, for every image kind, ONE layer at the smallest shape whose route takes that form -- the route
name is asserted first, so a change to a support query fails the case instead of turning it into a copy of the generic one -- and changes one parameter
in each of the ways a caller can: in-place arithmetic, an SGD / Adam step, load_state_dict, a new Parameter object, a round trip over the CPU, and a new
Parameter object on the SAME storage that reaches the same version count (the deterministic stand-in for a block the caching allocator hands back).
After the change the layer must give the bits of a freshly built module with the new parameters, agree with float64 within the form's own parity bound
(tests/test_kernels_gpu.py), and the float64 results before and after must differ by at least 100 x that bound (a change nobody could miss)."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import helpers
from test_kernels_gpu import close, ref_gcr, rnd
from test_network_gpu import maxerr

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU visible')
    from rfuse import ops as _ops
    return _ops


@contextlib.contextmanager
def arith(mode):
    from rfuse import ops as _ops
    saved, _ops.CONV_ARITH = _ops.CONV_ARITH, mode
    try:
        yield
    finally:
        _ops.CONV_ARITH = saved


def quiet(make):
    with contextlib.redirect_stdout(io.StringIO()):
        return make()


def cpu_state(mod):
    return {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}


def owner_of(mod, pname):
    path, _, attr = pname.rpartition('.')
    return (mod.get_submodule(path) if path else mod), attr


# ------------------------------------------------------------------------------------------------------------ the layers

class GcrLayer:
    """model.unet.SingleConv (GroupNorm -> conv3 -> ReLU) on [n, c0 (+ c1 upsampled), edge^3] -> cout; bound and measure of the form's test in test_kernels_gpu"""
    params = ('conv.weight', 'groupnorm.weight', 'groupnorm.bias')
    IMAGES = {'conv3': '_packed', 'conv3up': '_packed_up', 'conv3ups': '_packed_up_split', 'conv3s': '_packed_split', 'conv3e2': '_packed_e2'}

    def __init__(self, kind, route, mode, shape, tol, groups=8):
        self.kind, self.route, self.mode, self.shape, self.tol, self.groups = kind, route, mode, shape, tol, groups

    def make(self):
        from model.unet import SingleConv
        n, c0, c1, edge, cout = self.shape
        return SingleConv(c0 + c1, cout, num_groups=self.groups)

    def draw(self, name, shape, gen):
        if name == 'conv.weight':
            return rnd(gen, *shape, scale=1.0 / math.sqrt(27 * shape[1]))
        return 1 + 0.2 * rnd(gen, *shape) if name == 'groupnorm.weight' else 0.2 * rnd(gen, *shape)

    def inputs(self, gen):
        n, c0, c1, edge, cout = self.shape
        return (rnd(gen, n, c0, edge, edge, edge).relu_() if c0 else None, rnd(gen, n, c1, edge // 2, edge // 2, edge // 2).relu_() if c1 else None)

    def to_device(self, ops, xs):
        return tuple(t.to(DEV) if t is not None else None for t in xs)

    def asked_route(self, mod, xd):
        from rfuse import routes
        n, c0, c1, edge, cout = self.shape
        return routes.single(n, c0, c1, edge, cout, None, routes.split_arith(mod.range_ok(edge)), materialised=False)

    def run(self, mod, xd):
        return mod(*xd)

    def values(self, out):
        return out

    def images_held(self, mod):
        return {k for k, attr in self.IMAGES.items() if getattr(mod.conv, attr)._key is not None}

    def samples(self):
        n = self.shape[0]
        return sorted(set(range(min(n, 3))) | {n - 1})

    def ref(self, sd, xs, idx):
        pick = lambda t: t[idx].double() if t is not None else None
        return ref_gcr(pick(xs[0]), pick(xs[1]), sd['groupnorm.weight'].double(), sd['groupnorm.bias'].double(), self.groups, sd['conv.weight'].double())

    def check_close(self, got, ref, what):
        close(got, ref.float(), self.tol, what)

    def gap_bound(self, ref):
        return 100 * self.tol * max(1.0, ref.abs().max().item())


class ValidLayer:
    """one valid strided conv + bias + LeakyReLU(0.2) of a patch encoder (model.retrieval._ConvPatchEncoder._conv asks rfuse.routes.valid): spec =
    (n, cin, s, cout, k, stride); ``nxt``: the layer that would read the output (the grid form writes split form for it)"""
    params = ('layers.0.weight', 'layers.0.bias')
    IMAGES = {'convv': '_packed', 'convvl': '_packed_lds', 'convvv': '_packed_valu', 'convvs': '_packed_vsplit', 'convvpg': '_packed_vpg'}

    def __init__(self, kind, route, mode, spec, in_split=False, nxt=None):
        self.kind, self.route, self.mode, self.spec, self.in_split, self.nxt, self.tol = kind, route, mode, spec, in_split, nxt, 1e-5

    def make(self):
        from model.retrieval import _ConvPatchEncoder
        n, cin, s, cout, k, stride = self.spec
        nf = cout if cin == 1 else math.gcd(cin, cout)
        one_layer = type('OneLayerEncoder', (_ConvPatchEncoder,), {'SPEC': ((0 if cin == 1 else cin // nf, cout // nf, k, stride),)})
        return one_layer(nf, 8)

    def draw(self, name, shape, gen):
        if len(shape) == 1:
            return rnd(gen, *shape)
        return rnd(gen, *shape, scale=1.0 / math.sqrt(np.prod(shape[1:])))

    def inputs(self, gen):
        n, cin, s, cout, k, stride = self.spec
        return (rnd(gen, n, cin, s, s, s),)

    def to_device(self, ops, xs):
        x = xs[0].to(DEV)
        return (helpers.to_split_acts(ops, x) if self.in_split else x,)

    def _next(self):
        return None if self.nxt is None else self.nxt + ((lambda: True),)

    def asked_route(self, mod, xd):
        from rfuse import routes
        return routes.valid(mod._ask(mod.layers[0], xd[0].shape), self.in_split, self._next())[0]

    def run(self, mod, xd):
        out = mod._conv(mod.layers[0], xd[0], self._next())
        return out.data if self.in_split else out               # (a SplitActs: its bytes, viewed as the fp32 tensor it replaces)

    def values(self, out):
        from rfuse import ops
        return helpers.from_split_acts(ops.SplitActs(out)) if self.in_split else out

    def images_held(self, mod):
        return {k for k, attr in self.IMAGES.items() if getattr(mod.layers[0], attr)._key is not None}

    def samples(self):
        return [self.spec[0] - 1]

    def ref(self, sd, xs, idx):
        x = xs[0][idx]
        if self.in_split:                                       # the values the split-form input stands for (as test_conv3d_valid_leaky_split_pg)
            from rfuse import ops
            x = helpers.from_split_acts(helpers.to_split_acts(ops, x.to(DEV))).cpu()
        return F.leaky_relu(F.conv3d(x.double(), sd['layers.0.weight'].double(), sd['layers.0.bias'].double(), stride=self.spec[5]), 0.2)

    def check_close(self, got, ref, what):
        if self.in_split:                                       # test_conv3d_valid_leaky_split_pg: absolute
            err = (got.double().cpu() - ref).abs().max().item()
            assert err <= 1e-5, f'{what}: max abs err {err:.3e} > 1e-5'
        else:
            close(got, ref.float(), self.tol, what)

    def gap_bound(self, ref):
        return 100 * 1e-5 if self.in_split else 100 * self.tol * max(1.0, ref.abs().max().item())


class LinearLayer:
    """model.attention.LinearParams through rf_linear (ReLU fused), bound of test_linear"""
    kind, route, mode, tol = 'linear', 'linear', 'split', 1e-5
    params = ('weight', 'bias')

    def make(self):
        from model.attention import LinearParams
        return LinearParams(64, 128)

    def draw(self, name, shape, gen):
        return rnd(gen, *shape, scale=1.0 / math.sqrt(shape[1])) if len(shape) == 2 else rnd(gen, *shape)

    def inputs(self, gen):
        return (rnd(gen, 37, 64),)

    def to_device(self, ops, xs):
        return (xs[0].to(DEV),)

    def asked_route(self, mod, xd):
        return mod._packed.kind                                 # no form choice: the layer has one image

    def run(self, mod, xd):
        from rfuse import ops
        return mod.apply_to(xd[0], ops.ACT_RELU)

    def values(self, out):
        return out

    def images_held(self, mod):
        return {'linear'} if mod._packed._key is not None else set()

    def samples(self):
        return list(range(37))

    def ref(self, sd, xs, idx):
        return F.relu(F.linear(xs[0][idx].double(), sd['weight'].double(), sd['bias'].double()))

    def check_close(self, got, ref, what):
        close(got, ref.float(), self.tol, what)

    def gap_bound(self, ref):
        return 100 * self.tol * max(1.0, ref.abs().max().item())


class AttnMlpLayer(LinearLayer):
    """AttentionFeatureEncoder(16, 32, 2) through the fused 4-layer kernel (ops.PackedAttnMLP), bound of test_attn_mlp_rows_matches_float64"""
    kind, route, mode, tol = 'attn_mlp', 'attn_mlp_fused', 'split', 2e-6
    params = ('encoder.0.weight', 'encoder.2.weight', 'encoder.4.bias', 'encoder.6.bias')

    def make(self):
        from model.attention import AttentionFeatureEncoder
        return quiet(lambda: AttentionFeatureEncoder(16, 32, 2))

    def draw(self, name, shape, gen):
        return rnd(gen, *shape, scale=0.15)

    def inputs(self, gen):
        return (rnd(gen, 70, 128),)

    def asked_route(self, mod, xd):
        from rfuse import routes
        return 'attn_mlp_fused' if routes.attn_mlp_fused(mod.n_in, mod.n_out) else 'per_layer'

    def run(self, mod, xd):
        return mod(xd[0])

    def images_held(self, mod):
        held = {'linear'} if any(mod.encoder[i]._packed._key is not None for i in (0, 2, 4, 6)) else set()
        return held | ({'attn_mlp'} if mod._fused._key is not None else set())

    def samples(self):
        return list(range(70))

    def ref(self, sd, xs, idx):
        h = xs[0][idx].double()
        for i in (0, 2, 4, 6):
            h = h @ sd['encoder.%d.weight' % i].double().t() + sd['encoder.%d.bias' % i].double()
            if i < 6:
                h = F.leaky_relu(h, 0.01)
        return h


LAYERS = {c.kind: c for c in [
    # SingleConv: (n, c0, c1, edge, cout) -- the sample counts are the smallest the forms' support queries accept
    GcrLayer('conv3s', 'split_box', 'split', (256, 8, 0, 8, 16), 1e-5),
    GcrLayer('conv3e2', 'e2', 'split', (16, 8, 0, 2, 16), 1e-5),
    GcrLayer('conv3ups', 'up_split', 'split', (256, 8, 8, 8, 48), 1e-5),
    GcrLayer('conv3up', 'up_fp32', 'fp32', (256, 8, 8, 8, 48), 1e-5),
    GcrLayer('conv3', 'generic', 'fp32', (256, 8, 0, 8, 16), 2e-5),
    # patch-encoder layers: the first entry of VALID_CASES (tests/test_nonfinite_gpu.py) of each form that rfuse.routes.valid sends there
    ValidLayer('convv', 'gather', 'split', (3, 1, 8, 16, 3, 1)),
    ValidLayer('convvl', 'lds', 'fp32', (3, 48, 20, 48, 3, 2)),
    ValidLayer('convvv', 'valu', 'split', (3, 1, 48, 12, 5, 1)),
    ValidLayer('convvs', 'split', 'split', (2, 12, 44, 24, 3, 1)),
    ValidLayer('convvpg', 'grid', 'split', (3, 12, 64, 20, 3, 1), in_split=True, nxt=(3, 20, 62, 24, 3, 1)),      # (3, 64, 20) of test_conv3d_valid_leaky_split_pg
    LinearLayer(), AttnMlpLayer()]}

CHANGES = ('inplace', 'sgd', 'adam', 'load_state_dict', 'new_parameter', 'via_cpu', 'same_storage')


def build(layer, seed):
    """the layer's module on the device with seeded parameters, written in place (every parameter then has version >= 1)"""
    mod, gen = layer.make(), torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            p.copy_(layer.draw(name, tuple(p.shape), gen))
    return mod.to(DEV).eval()


def fresh_copy(layer, mod):
    """a newly constructed module (own images, own range values) holding mod's present parameters"""
    other = layer.make().to(DEV).eval()
    other.load_state_dict(cpu_state(mod))
    return other


def apply_change(mod, pname, change, new, grad=None, lr=1.0):
    """make parameter ``pname`` of ``mod`` hold ``new`` (CPU tensor) in the way ``change`` names; the optimisers take one step of ``lr`` along ``grad`` instead"""
    own, attr = owner_of(mod, pname)
    p = getattr(own, attr)
    if change == 'inplace':
        with torch.no_grad():
            p.mul_(0.0).add_(new.to(DEV))
    elif change in ('sgd', 'adam'):
        p.grad = grad.to(DEV)
        opt = torch.optim.SGD(mod.parameters(), lr=lr) if change == 'sgd' else torch.optim.Adam(mod.parameters(), lr=lr)
        opt.step()                                              # (Adam: default foreach on the device)
        p.grad = None
    elif change == 'load_state_dict':
        sd = cpu_state(mod)
        sd[pname] = new
        mod.load_state_dict(sd)
    elif change == 'new_parameter':
        setattr(own, attr, nn.Parameter(new.to(DEV)))
    elif change == 'via_cpu':
        mod.cpu()
        with torch.no_grad():
            getattr(own, attr).copy_(new)
        mod.to(DEV)
    elif change == 'same_storage':
        version, address = p._version, p.data_ptr()
        assert version >= 1
        q = nn.Parameter(p.data)                                # the same storage under a fresh version counter
        with torch.no_grad():
            while q._version < version - 1:
                q.add_(0.0)
            q.copy_(new.to(DEV))
        assert (q._version, q.data_ptr(), q.shape, q.device) == (version, address, p.shape, p.device) and q is not p
        setattr(own, attr, q)
    else:
        raise ValueError(change)
    del p


_refs = {}


def reference(layer, key, sd, xs):
    """float64 evaluation on the layer's reference samples, computed once per distinct parameter set"""
    if key not in _refs:
        _refs[key] = layer.ref(sd, xs, layer.samples())
    return _refs[key]


@pytest.mark.parametrize('change', CHANGES)
@pytest.mark.parametrize('kind', list(LAYERS))
def test_packed_image_follows_its_parameters(ops, kind, change):
    """one image kind x one way of changing a parameter, for each of the layer's parameters in turn (a module built anew for each): see the module docstring"""
    layer = LAYERS[kind]
    seed = 1000 + list(LAYERS).index(kind)
    xs = layer.inputs(torch.Generator().manual_seed(seed + 500))
    idx = layer.samples()
    with arith(layer.mode), torch.no_grad():
        xd = layer.to_device(ops, xs)
        for pi, pname in enumerate(layer.params):
            mod = build(layer, seed)
            asked = layer.asked_route(mod, xd)
            assert asked == layer.route, f'{kind}: this shape is meant to run route {layer.route!r}, rfuse.routes names {asked!r}'
            before = layer.run(mod, xd)                                              # packs the image from the old parameters
            assert layer.images_held(mod) == {kind}, f'{kind}: the forward packed {layer.images_held(mod)}'
            sd_old = cpu_state(mod)
            ref_old = reference(layer, (kind, 'old'), sd_old, xs)
            layer.check_close(layer.values(before)[idx], ref_old, f'{kind}: before the change')
            gen = torch.Generator().manual_seed(seed + 50 + pi)
            new = layer.draw(pname, tuple(sd_old[pname].shape), gen)
            # SGD at lr 1 along old - new lands on `new` up to rounding; the first Adam step moves every element by lr against the sign of its gradient: lr = the
            # parameter's own spread, so either step is as big a change as a new draw
            grad = sd_old[pname] - new if change == 'sgd' else rnd(gen, *new.shape)
            apply_change(mod, pname, change, new, grad, lr=1.0 if change == 'sgd' else float(sd_old[pname].std()))
            after = layer.run(mod, xd)
            sd_new = cpu_state(mod)
            assert not torch.equal(sd_new[pname], sd_old[pname]), f'{kind}.{pname}: {change} changed nothing'
            assert all(torch.equal(sd_new[k], sd_old[k]) for k in sd_old if k != pname)
            want = layer.run(fresh_copy(layer, mod), xd)
            assert same_bits(after, want), \
                f'{kind}.{pname} after {change}: not the bits of a fresh module with the new parameters (max diff {(after - want).abs().max().item():.3e})'
            exact = change not in ('sgd', 'adam')                                    # the other changes land on `new` itself: one reference for all of them
            if exact:
                assert torch.equal(sd_new[pname], new)
            ref_new = reference(layer, (kind, pname, 'new' if exact else change), sd_new, xs)
            layer.check_close(layer.values(after)[idx], ref_new, f'{kind}.{pname} after {change} vs float64')
            gap = (ref_new - ref_old).abs().max().item()
            assert gap >= layer.gap_bound(ref_new), f'{kind}.{pname}: the change moves the float64 result by {gap:.3e} only'
    print(f'\nderived-state matrix: {kind:9s} route {layer.route!r} (CONV_ARITH {layer.mode!r}), change {change}: {", ".join(layer.params)}')


# ------------------------------------------------------------------------------- range decisions under the same changes

def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


RANGE_LAYER = GcrLayer('conv3s', 'split_box', 'split', (256, 8, 0, 8, 16), 1e-5)
# one element out of the split forms' range (ops.SPLIT_MAX_ABS_*): |w| > 65504 / 16 / 8; |gamma| sqrt(512 elements of a group) > 65504 * 16; |beta| > it
OUT_OF_RANGE = {'conv.weight': ((3, 5, 1, 1, 1), 3.0e4), 'groupnorm.weight': ((2,), 1.0e5), 'groupnorm.bias': ((7,), 2.0e6)}


def run_as(layer, mod, xd, mode):
    with arith(mode), torch.no_grad():
        return layer.run(mod, xd)


def move_element(mod, pname, change, index, value):
    """parameter ``pname`` with element ``index`` set to (about) ``value``, by ``change``: the optimisers step along a gradient that is zero everywhere else
    (SGD: lr 1, gradient old - value; Adam: its first step is lr * sign(gradient))"""
    old = cpu_state(mod)[pname]
    new, grad = old.clone(), torch.zeros_like(old)
    new[index] = value
    delta = float(old[index]) - value
    grad[index] = delta if change == 'sgd' else math.copysign(1.0, delta)
    apply_change(mod, pname, change, new, grad, lr=1.0 if change == 'sgd' else abs(delta))


@pytest.mark.parametrize('change', ['sgd', 'adam', 'new_parameter', 'via_cpu', 'same_storage'])
@pytest.mark.parametrize('pname', list(OUT_OF_RANGE))
def test_range_decision_follows_the_parameters(ops, pname, change):
    """test_split_forms_fall_back_to_fp32_outside_their_range under the other ways of changing a parameter: out of range the layer gives the fp32 route's
    bits, back in range the split route's again -- each time those of a freshly built layer holding the same parameters, whose images and range values are new"""
    layer, (index, value) = RANGE_LAYER, OUT_OF_RANGE[pname]
    xd = layer.to_device(ops, layer.inputs(torch.Generator().manual_seed(31)))
    mod = build(layer, 32)
    group_elements = 512
    in_range = lambda m: ops.split_range_ok(m.conv.weight, m.groupnorm.weight, m.groupnorm.bias, group_elements)
    assert in_range(mod)
    split0, fp320 = run_as(layer, mod, xd, 'split'), run_as(layer, mod, xd, 'fp32')                 # both images and all three ranges are now cached
    assert not same_bits(split0, fp320), 'inside the range the split kernel is the one that runs'
    home = float(cpu_state(mod)[pname][index])

    move_element(mod, pname, change, index, value)
    assert abs(float(cpu_state(mod)[pname][index])) >= 0.99 * value
    assert not in_range(mod), f'{pname} after {change}: still reported in range'
    got = run_as(layer, mod, xd, 'split')
    fresh = fresh_copy(layer, mod)
    assert torch.isfinite(got).all()
    assert same_bits(got, run_as(layer, fresh, xd, 'fp32')), f'out-of-range {pname} after {change}: the layer did not take the fp32 kernels'
    assert same_bits(got, run_as(layer, mod, xd, 'fp32'))

    move_element(mod, pname, change, index, home)
    assert in_range(mod), f'{pname} back home after {change}: still reported out of range'
    back = run_as(layer, mod, xd, 'split')
    fresh = fresh_copy(layer, mod)
    assert same_bits(back, run_as(layer, fresh, xd, 'split')), f'{pname} back in range after {change}: not the split route\'s bits'
    assert not same_bits(back, run_as(layer, fresh, xd, 'fp32'))


def test_one_optimiser_step_refreshes_every_range_at_once(ops, monkeypatch):
    """Three layers, every parameter changed by ONE optimiser step, exactly one layer (the middle one) now out of range.  The first range asked for afterwards
    is that of a layer that stayed in range: the miss refreshes all stale parameters in one torch._foreach_norm (one host sync per training step), and every
    layer must then have taken the right route."""
    layer = RANGE_LAYER
    xd = layer.to_device(ops, layer.inputs(torch.Generator().manual_seed(41)))
    mods = nn.ModuleList([build(layer, 42 + i) for i in range(3)])
    for m in mods:
        run_as(layer, m, xd, 'split')                                                               # every parameter's range has been asked for once
    gen = torch.Generator().manual_seed(43)
    for p in mods.parameters():
        p.grad = (rnd(gen, *p.shape) * 1e-3).to(DEV)
    mods[1].conv.weight.grad[3, 5, 1, 1, 1] = -3.0e4
    torch.optim.SGD(mods.parameters(), lr=1.0).step()
    calls, singles = [], []
    real_norm, real_abs = torch._foreach_norm, torch.Tensor.abs
    monkeypatch.setattr(torch, '_foreach_norm', lambda ts, *a, **kw: (calls.append(len(ts)), real_norm(ts, *a, **kw))[1])
    monkeypatch.setattr(torch.Tensor, 'abs', lambda self, *a, **kw: (singles.append(tuple(self.shape)), real_abs(self, *a, **kw))[1])
    first = mods[2]
    assert ops.split_range_ok(first.conv.weight, first.groupnorm.weight, first.groupnorm.bias, 512)
    outs = [run_as(layer, m, xd, 'split') for m in mods]
    monkeypatch.undo()
    assert len(calls) == 1 and calls[0] >= 9 and singles == [], f'range refresh after one step: {calls} batched reductions, single ones of {singles}'
    for i, (m, out) in enumerate(zip(mods, outs)):
        fresh = fresh_copy(layer, m)
        want_mode, other = ('fp32', 'split') if i == 1 else ('split', 'fp32')
        assert same_bits(out, run_as(layer, fresh, xd, want_mode)), f'layer {i}: not the {want_mode} route\'s bits'
        if i != 1:
            assert not same_bits(out, run_as(layer, fresh, xd, other))


def test_attention_mlp_range_and_bias_changes(ops):
    """ops.PackedAttnMLP: a change of one bias alone re-packs (its image carries the biases); one of the four weights out of the f16 pairs' range selects the
    fp32-MFMA form -- beside the per-layer rf_linear route (ops.USE_FUSED_ATTN_MLP = False), within test_attn_mlp_rows_matches_float64's bound"""
    layer = LAYERS['attn_mlp']
    xd = layer.to_device(ops, layer.inputs(torch.Generator().manual_seed(51)))

    def per_layer(m):
        ops.USE_FUSED_ATTN_MLP = False
        try:
            return run_as(layer, m, xd, 'split')
        finally:
            ops.USE_FUSED_ATTN_MLP = True
    mod = build(layer, 52)
    first = run_as(layer, mod, xd, 'split')
    with torch.no_grad():
        mod.encoder[4].bias[17] += 0.5
    moved = run_as(layer, mod, xd, 'split')
    assert not same_bits(moved, first)
    assert same_bits(moved, run_as(layer, fresh_copy(layer, mod), xd, 'split')), 'a bias changed: the fused image was not packed again'
    close(moved, per_layer(mod), 2e-6, 'fused vs per-layer rf_linear after a bias change')
    for i in (0, 2, 4, 6):
        mod = build(layer, 52)
        split_form = run_as(layer, mod, xd, 'split')
        assert not same_bits(split_form, run_as(layer, mod, xd, 'fp32')), 'inside the range the split-operand form is the one that runs'
        with torch.no_grad():
            mod.encoder[i].weight[5, 3] = 3.0e4                                                   # x 16 > 65504
        assert mod._fused.get([mod.encoder[j] for j in (0, 2, 4, 6)])[1] is None, f'encoder.{i}.weight out of range: the split image is still offered'
        got = run_as(layer, mod, xd, 'split')
        assert torch.isfinite(got).all()
        assert same_bits(got, run_as(layer, fresh_copy(layer, mod), xd, 'fp32')), f'encoder.{i}.weight out of range: not the fp32-MFMA form\'s bits'
        close(got, per_layer(mod), 2e-6, f'fp32-MFMA form vs per-layer rf_linear, encoder.{i}.weight out of range')


# ------------------------------------------------------------------------------------------- cross-stream ordering of a pack

# Only images that hold multiplicands and nothing else (k_conv3_pack, k_conv3_split_pack, k_linear_pack write weights, their f16 pieces and zero padding; the
# kernels read no size or offset from them): a reader that overtook the pack would compute wrong numbers from the poisoned buffer, and nothing else.
STREAM_LAYERS = {'conv3': LAYERS['conv3'], 'conv3s': LAYERS['conv3s'], 'linear': LAYERS['linear']}


@pytest.fixture(scope='module')
def two_streams(ops):
    """One pair for all cases.  Streams share the process's few hardware queues round-robin, and two streams on ONE queue are ordered by it, wait or no wait:
    take a second stream that is seen to overtake the first (its small kernel is done while the first stream's ballast still runs), the last candidate otherwise."""
    s1, ballast, probe = torch.cuda.Stream(DEV), torch.ones(64 * 1024 * 1024, device=DEV), torch.zeros(64, device=DEV)
    for _candidate in range(4):
        s2 = torch.cuda.Stream(DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            for _ in range(20):
                ballast.mul_(1.0)
            busy = torch.cuda.Event()
            busy.record()
        with torch.cuda.stream(s2):
            probe.add_(1.0)
            done = torch.cuda.Event()
            done.record()
        done.synchronize()
        overtook = not busy.query()
        torch.cuda.synchronize()
        if overtook:
            break
    return s1, s2


@pytest.mark.parametrize('kind', list(STREAM_LAYERS))
def test_pack_is_ordered_before_readers_on_other_streams(ops, two_streams, kind):
    """The image is packed on whichever stream first needs it (ops._PackedReady).  A few milliseconds of unrelated work sit in front of the pack on stream 1;
    stream 2 then runs the same layer with no synchronisation at all and must still read the finished image -- on first use, and again after a weight change,
    when the re-pack has to forget which streams were allowed to read without waiting."""
    layer = STREAM_LAYERS[kind]
    xd = layer.to_device(ops, layer.inputs(torch.Generator().manual_seed(61)))
    mod = build(layer, 62)
    ballast = torch.ones(64 * 1024 * 1024, device=DEV)                                              # 256 MB: twenty passes over it take a few milliseconds
    s1, s2 = two_streams
    # both streams have run the layer once (another module, OTHER weights): the caching allocator then serves the measured forwards from the streams' own free
    # blocks, with no device-wide allocation in between, and a recycled image block holds a different image
    warm = build(layer, 63)
    for s in (s1, s2):
        with torch.cuda.stream(s):
            run_as(layer, warm, xd, layer.mode)
    torch.cuda.synchronize()
    del warm
    for round_ in ('first use', 'after a weight change'):
        if round_ != 'first use':
            with torch.no_grad():
                owner_of(mod, layer.params[0])[0].weight.mul_(-1.5)
        with arith(layer.mode):
            assert layer.asked_route(mod, xd) == layer.route                                        # (and the range check's host sync happens here, not on stream 1)
        serial = run_as(layer, fresh_copy(layer, mod), xd, layer.mode)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            for _ in range(20):
                ballast.mul_(1.0)
            out1 = run_as(layer, mod, xd, layer.mode)                                               # packs here, behind the ballast
        with torch.cuda.stream(s2):
            out2 = run_as(layer, mod, xd, layer.mode)
        torch.cuda.synchronize()
        assert layer.images_held(mod) == {kind}
        assert same_bits(out1, serial), f'{kind}, {round_}: the packing stream\'s own result differs from the serial one'
        assert same_bits(out2, serial), f'{kind}, {round_}: a reader on another stream did not wait for the pack'


# ------------------------------------------------------------------------------------------------------------ feature cache

def test_feature_cache_is_refused_after_the_backbone_changed(gpu):
    """PatchDatabase.feature_cache holds the retrieval backbone's features of every database row: once the backbone's weights change, refine(use_feature_cache=True)
    must refuse the old cache (naming build_feature_cache, like the error for a missing one), and after a rebuild match the full path again within
    test_feature_cache_mode_matches_full_path's bound"""
    from rfuse import configs as rf_configs
    from rfuse import synthetic
    from rfuse.database import PatchDatabase
    from rfuse.engine import RefinementEngine
    cfg = rf_configs.get_config('C3')
    db = synthetic.make_database(33, cfg, 64 * 6 + 10)
    eng = RefinementEngine(cfg, gpu, PatchDatabase(db['emb'], db['meta'], db['volumes'], gpu))
    shapes = {name: {k: tuple(v.shape) for k, v in m.state_dict().items()} for name, m in eng.modules().items()}
    eng.load_state_dicts({name: helpers.seeded_sd(shapes[name], 400 + len(name)) for name in shapes})
    x = torch.from_numpy(np.stack([synthetic.make_chunk(700 + b, cfg)['input_raw'] for b in range(2)])).to(gpu)
    eng.database.build_feature_cache(eng.retrieval_backbone, cfg, rows_per_batch=128)
    first = eng.refine(x, use_feature_cache=True)
    assert maxerr(first.cpu(), eng.refine(x).cpu()) <= 1e-5
    eng.load_state_dicts({'retrieval_backbone': helpers.seeded_sd(shapes['retrieval_backbone'], 977)})
    full = eng.refine(x)
    assert maxerr(full.cpu(), first.cpu()) > 1e-3, 'the new backbone weights move the field: a stale cache would be visible'
    with pytest.raises(RuntimeError, match='build_feature_cache'):
        eng.refine(x, use_feature_cache=True)
    eng.database.build_feature_cache(eng.retrieval_backbone, cfg, rows_per_batch=128)
    assert maxerr(eng.refine(x, use_feature_cache=True).cpu(), full.cpu()) <= 1e-5
    with torch.no_grad():
        next(eng.retrieval_backbone.parameters()).mul_(1.0)                                         # any in-place write counts: versions, not values, are compared
    with pytest.raises(RuntimeError, match='build_feature_cache'):
        eng.refine(x, use_feature_cache=True)
