"""CPU: the oracle side of the non-finite contract (tests/test_nonfinite_gpu.py checks the kernels against it).

The dependency cones of tests/nonfinite.py are combinatorial; here they are held against float64 torch, and the float32 oracle
(oracle/refpath.forward_full) is pinned on a batch with one NaN voxel: that chunk's df is NaN throughout (its GroupNorm statistics
come from the data), the other chunk's df is the clean run's, bit for bit."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
from nonfinite import (assert_bit_equal_nan, assert_close_nonfinite, bit_equal_nan, cone_conv, cone_pool2, cone_up2, point_mask)
from oracle import refpath
from rfuse import configs as rf_configs

NAN = float('nan')


def test_comparators():
    a = torch.tensor([1.0, NAN, -0.0, float('inf')])
    assert bit_equal_nan(a, a.clone())
    assert not bit_equal_nan(a, torch.tensor([1.0, NAN, 0.0, float('inf')]))       # signed zeros differ in their bits
    assert not bit_equal_nan(a, torch.tensor([1.0, 2.0, -0.0, float('inf')]))
    with pytest.raises(AssertionError, match='NaN masks differ'):
        assert_close_nonfinite(torch.tensor([1.0, 0.0]), torch.tensor([1.0, NAN]), 1e-5, 'relu(nan) as 0')
    with pytest.raises(AssertionError, match=r'\+inf masks differ'):
        assert_close_nonfinite(torch.tensor([1.0, 65504.0]), torch.tensor([1.0, float('inf')]), 1e-5, 'clamped inf')
    with pytest.raises(AssertionError, match='max abs err'):
        assert_close_nonfinite(torch.tensor([1.1, NAN]), torch.tensor([1.0, NAN]), 1e-5, 'finite part')
    assert_close_nonfinite(torch.tensor([1.0, NAN, float('-inf')]), torch.tensor([1.0 + 1e-7, NAN, float('-inf')]), 1e-5)
    with pytest.raises(AssertionError, match='other bits'):
        assert_bit_equal_nan(torch.tensor([1.0, NAN]), torch.tensor([1.0 + 1e-7, NAN]))


@pytest.mark.parametrize('edge,k,stride,padding', [(8, 3, 1, 1), (5, 3, 1, 1), (9, 3, 2, 0), (7, 5, 1, 0), (6, 2, 1, 0)])
def test_conv_cone_equals_float64_torch(edge, k, stride, padding):
    """the combinatorial cone of a few NaN voxels (corners and faces included) = the NaN mask of a float64 conv with weights free of zeros"""
    gen = torch.Generator().manual_seed(edge * 10 + k)
    cin, cout = 3, 4
    x = torch.randn(2, cin, edge, edge, edge, generator=gen, dtype=torch.float64)
    w = torch.randn(cout, cin, k, k, k, generator=gen, dtype=torch.float64)
    w[w == 0] = 1e-3
    pts = [(0, 1, 0, 0, 0), (0, 2, edge - 1, edge // 2, edge - 1), (1, 0, edge // 2, 0, edge - 1)]
    for p in pts:
        x[p] = NAN
    y = F.conv3d(x, w, padding=padding, stride=stride)
    cone = cone_conv(point_mask(x.shape, pts), cout, k, stride, padding)
    assert torch.equal(torch.isnan(y), cone)
    assert torch.equal(torch.isnan(F.max_pool3d(y, 2)), cone_pool2(cone)) if min(y.shape[2:]) >= 2 else True


def test_up_cone_equals_float64_torch():
    x = torch.rand(1, 2, 4, 4, 4, dtype=torch.float64)
    pts = [(0, 1, 3, 0, 2)]
    x[pts[0]] = NAN
    up = F.interpolate(x, scale_factor=2, mode='nearest')
    assert torch.equal(torch.isnan(up), cone_up2(point_mask(x.shape, pts)))


def _shapes(cfg):
    import model
    with contextlib.redirect_stdout(io.StringIO()):
        mods = {'unet_backbone': model.get_unet_backbone(cfg), 'decoder': model.get_decoder(cfg),
                'retrieval_backbone': model.get_retrieval_backbone(cfg), 'patched_attention_block': model.get_attention_block(cfg)}
    return {k: {n: tuple(v.shape) for n, v in m.state_dict().items()} for k, m in mods.items()}


def test_oracle_forward_full_isolates_a_nan_chunk():
    """float32 oracle, two chunks of C3: a NaN voxel in chunk 1's input makes its df NaN throughout and leaves chunk 0's bit-equal to the clean
    batch; a NaN voxel in one retrieved 64^3 volume of chunk 0 makes chunk 0's df non-finite somewhere and leaves chunk 1's bit-equal"""
    cfg = rf_configs.get_config('C3')
    x_in, retr = helpers.chunk_inputs(cfg, 3, 2)
    shapes = _shapes(cfg)
    sds = {m: helpers.seeded_sd(shapes[m], 3000 + i) for i, m in enumerate(('unet_backbone', 'decoder', 'retrieval_backbone', 'patched_attention_block'))}
    trunc = rf_configs.truncations(cfg)[1]
    torch.set_num_threads(8)
    with torch.no_grad():
        clean = refpath.forward_full(sds, cfg, torch.from_numpy(x_in), torch.from_numpy(retr), trunc)
        x_bad = x_in.copy()
        s = x_in.shape[-1]
        x_bad[1, 0, 5, s // 2, s - 1] = np.nan
        bad = refpath.forward_full(sds, cfg, torch.from_numpy(x_bad), torch.from_numpy(retr), trunc)
        r_bad = retr.copy()
        r_bad[0, 1, 17, 0, 33] = np.nan
        bad_r = refpath.forward_full(sds, cfg, torch.from_numpy(x_in), torch.from_numpy(r_bad), trunc)
    assert torch.isfinite(clean).all()
    assert torch.isnan(bad[1]).all()
    assert_bit_equal_nan(bad[0], clean[0], 'chunk without the NaN input voxel')
    assert (~torch.isfinite(bad_r[0])).any()
    assert_bit_equal_nan(bad_r[1], clean[1], 'chunk without the NaN retrieval voxel')
