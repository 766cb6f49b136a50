"""CPU: the input families of tests/conditioning.py have the properties they state, and they DISCRIMINATE: on near-constant, constant and large-mean
inputs the two-term fp32 form of GroupNorm  x * scale' + shift'  misses the conv kernels' 1e-5 bar against float64, the centre-first form with
float64 statistics that the kernels claim (csrc/common.h: gn_affine) stays a tenth of it.  So a kernel that folds the centre into the shift fails
tests/test_conditioning_gpu.py, which it could not on relu(randn)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conditioning as cnd

BAR = 1e-5
CASES = [(16, 16, 8, 8), (1, 8, 16, 8), (16, 16, 16, 8)]                 # (cin, cout, edge, groups)


def _problem(case):
    cin, cout, edge, groups = case
    gen = torch.Generator().manual_seed(sum(case))
    x, fams = cnd.mixed(gen, len(cnd.FAMILIES), cin, edge, groups)
    gamma, beta = 1 + 0.2 * torch.randn(cin, generator=gen), 0.2 * torch.randn(cin, generator=gen)
    w = torch.randn(cout, cin, 3, 3, 3, generator=gen) / np.sqrt(27 * cin)
    ref = F.relu(F.conv3d(F.group_norm(x.double(), cnd.gn_groups(cin, groups), gamma.double(), beta.double(), 1e-5), w.double(), padding=1))
    return x, fams, gamma, beta, w, ref


@pytest.mark.parametrize('case', CASES)
def test_families_separate_the_centre_form_from_the_two_term_form(case):
    cin, cout, edge, groups = case
    x, fams, gamma, beta, w, ref = _problem(case)
    conv = lambda y: F.relu(F.conv3d(y, w, padding=1))
    centre = cnd.per_sample_errors(conv(cnd.gn_centre_form_fp32(x, gamma, beta, groups)), ref)
    two = cnd.per_sample_errors(conv(cnd.gn_two_term_fp32(x, gamma, beta, groups)), ref)
    torch_fp32 = cnd.per_sample_errors(F.relu(F.conv3d(F.group_norm(x, cnd.gn_groups(cin, groups), gamma, beta, 1e-5), w, padding=1)), ref)
    print()
    for fam, a, b, c in zip(fams, centre.tolist(), two.tolist(), torch_fp32.tolist()):
        print('%s %-14s centre form %.1e | two-term form %.1e | torch fp32 %.1e' % (case, fam, a, b, c))
    for fam, a, b, c in zip(fams, centre.tolist(), two.tolist(), torch_fp32.tolist()):
        assert a <= 0.1 * BAR, (fam, a)
        if fam in ('near_constant', 'constant', 'big_mean'):
            assert b > BAR, (fam, b)          # (torch's own fp32 group_norm is printed for information: which form it takes depends on its build)


def test_centre_form_triple_carries_what_the_rounded_mean_loses():
    gen = torch.Generator().manual_seed(5)
    x, _ = cnd.mixed(gen, 9, 16, 8, 8)
    gamma, beta = 1 + 0.2 * torch.randn(16, generator=gen), 0.2 * torch.randn(16, generator=gen)
    a = cnd.affine_centre_form(x, gamma, beta, 8).double()
    mean, rstd = cnd.group_stats64(x, 8)
    assert torch.equal(a[..., 0].float(), mean.float())
    two_term = a[..., 2] - a[..., 0] * a[..., 1]
    want = beta.double()[None] - mean * gamma.double()[None] * rstd
    assert float((two_term - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('c,edge,groups', [(16, 8, 8), (1, 8, 8), (56, 4, 8), (6, 8, 6), (64, 1, 8)])
def test_family_properties(c, edge, groups):
    gen = torch.Generator().manual_seed(c + edge)
    n, g = 4, cnd.gn_groups(c, groups)
    vox = edge ** 3
    xs = {fam: cnd.make(fam, gen, n, c, edge, groups) for fam in cnd.FAMILIES}
    for fam, x in xs.items():
        assert x.dtype == torch.float32 and tuple(x.shape) == (n, c, edge, edge, edge) and bool(torch.isfinite(x).all()), fam
    var = lambda x: x.double().reshape(n, g, -1).var(-1, unbiased=False)
    assert bool((xs['constant'] == 3.0).all()) and float(var(xs['constant']).max()) == 0.0
    nc = xs['near_constant']
    assert 0.0 < float(var(nc).max()) < 1e-7 and float((nc - 3.0).abs().max()) < 1e-3             # var << eps = 1e-5
    sat = xs['saturated']
    assert float(sat.max()) == 3.0 and float(sat.min()) >= 0.0 and float((sat == 3.0).float().mean()) > 0.9
    assert float((xs['big_mean'].double().mean() - 1000.0).abs()) < 1.0
    sp = xs['spike'].reshape(n, g, c // g, vox)
    assert bool(((sp != 0).sum(dim=(2, 3)) == 1).all()) and bool((sp[:, :, 0].max(dim=2).values == 5.0).all())     # one voxel per group, in its first channel
    mean, rstd = cnd.group_stats64(xs['spike'], g)
    peak = ((xs['spike'].double().reshape(n, c, -1).max(dim=2).values - mean) * rstd).reshape(n, g, c // g)[:, :, 0]
    elems = (c // g) * vox
    if elems > 1:                                                        # attains sqrt(group elements) but for eps: (5 - 5/N) / sqrt(25 (N-1) / N^2 + eps)
        assert bool((peak <= np.sqrt(elems)).all()) and bool((peak >= 0.98 * np.sqrt(elems - 1)).all())
    dead = xs['dead_groups'].reshape(n, g, -1)
    if g < 2:
        assert float(dead.abs().max()) == 0.0
    else:
        assert float(dead[:, :g // 2].abs().max()) == 0.0 and bool((dead[:, g // 2:].abs().amax(dim=2) > 0).all())
    assert float(xs['scaled_up'].max()) > 2.0 ** 39 and 0.0 < float(xs['scaled_down'].max()) < 2.0 ** -37
    assert float(xs['relu_randn'].min()) == 0.0


def test_mixed_covers_every_family_and_names_each_sample():
    gen = torch.Generator().manual_seed(1)
    x, fams = cnd.mixed(gen, 20, 8, 4, 8)
    nf = len(cnd.FAMILIES)
    assert fams == [cnd.FAMILIES[i % nf] for i in range(20)]
    for i, fam in enumerate(fams):
        if fam == 'constant':
            assert bool((x[i] == 3.0).all())
        if fam == 'big_mean':
            assert float(x[i].mean()) > 900
    s0, s1, f2 = cnd.mixed_pair(gen, 10, 8, 16, 8, 8)
    assert tuple(s0.shape) == (10, 8, 8, 8, 8) and tuple(s1.shape) == (10, 16, 4, 4, 4) and f2 == fams[:10]
    assert bool((s0[3] == 3.0).all()) and bool((s1[3] == 3.0).all())
    assert cnd.mixed_pair(gen, 4, 0, 16, 8, 8)[0] is None
    x3, f3 = cnd.mixed(gen, 3, 8, 4, 8, families=('near_constant', 'big_mean', 'saturated'))
    assert f3 == ['near_constant', 'big_mean', 'saturated'] and float(x3[1].mean()) > 900
    assert cnd.reference_subset(100) == list(range(18)) + list(range(91, 100)) and cnd.reference_subset(5) == list(range(5))


def test_per_sample_close_bounds_each_sample_by_its_own_size():
    ref = torch.zeros(3, 4, dtype=torch.float64)
    ref[0], ref[1], ref[2] = 1000.0, 1.0, 1e-9
    got = ref.clone()
    got[1, 0] += 5e-4                                                    # 5e-7 of the loudest sample, 5e-4 of its own
    fams = ['a', 'b', 'c']
    with pytest.raises(AssertionError, match="'b'"):
        cnd.per_sample_close(got, ref, 1e-5, fams, 'unit')
    got = ref.clone()
    got[2, 1] += 1e-12                                                   # 1e-3 of a quiet gradient sample: passes with the forward floor, fails with the gradient floor
    cnd.per_sample_close(got, ref, 1e-5, fams, 'unit')
    with pytest.raises(AssertionError, match="'c'"):
        cnd.per_sample_close(got, ref, 1e-5, fams, 'unit', floor=1e-30)
    got = ref.clone()
    got[0, 0] = float('nan')
    with pytest.raises(AssertionError, match="'a'"):
        cnd.per_sample_close(got, ref, 1e-5, fams, 'unit')
    with pytest.raises(AssertionError):
        cnd.tensor_close(got, ref, 1e-5, 'unit')
    for k in [k for k in cnd.TABLE if k[0] == 'unit']:
        del cnd.TABLE[k]
