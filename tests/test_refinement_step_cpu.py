"""CPU: the restatement of the refinement trainer's steps (tests/refinement_step_ref.py) against what the reference's own methods gave
(tests/golden/refinement_step.npz, tools/gen_refinement_step_golden.py), float32 against float32 on the same host; and what of
``rfuse.training.RefinementStep`` needs no GPU: the parameter lists, the hyper-parameters, the guards, the binding of the tenth header."""
import numpy as np
import pytest
import torch

import helpers
import refinement_step_ref as ref

FIX = helpers.load_fixture('refinement_step')
CASES = [str(c) for c in FIX['cases']]
# the generator records loss_shape's results in call order: training_step_full and validation_step call it in these orders (trainer :78-80, :131-132)
SHAPE_CALLS = {0: ('',), 1: ('',), 3: ('_fuse', '_back', '_retr'), 'val': ('_full', '_nn1')}


def fixture_scalars(case, phase):
    names = [str(n) for n in FIX[case + '_scalar_names']]
    out = {}
    for name, value in zip(names, FIX[case + '_scalars']):
        stem, _, tag = name.rpartition('_')
        if stem in ('shape', 'l1', 'normal') and len(tag) == 1:
            name = stem + SHAPE_CALLS[phase]['abc'.index(tag)]
        out[name] = float(value)
    return out


@pytest.fixture(scope='module')
def problems():
    cache = {}

    def get(cfg_name):
        if cfg_name not in cache:
            mods = ref.make_modules(ref.rf_configs.get_config(cfg_name))
            shapes = {k: {n: tuple(v.shape) for n, v in m.state_dict().items()} for k, m in mods.items()}
            cache[cfg_name] = ref.problem(cfg_name, shapes)
        return cache[cfg_name]
    return get


@pytest.mark.parametrize('case', CASES)
def test_restatement_is_the_references_step(problems, case):
    """losses to 1e-5 relative, the occupancy rows exactly, every optimised parameter's gradient norm to 1e-3 relative"""
    cfg_name, tag = case.split('_')
    phase = 'val' if tag == 'val' else int(tag[1:])
    cfg, sds, data, noise = problems(cfg_name)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    leaves = ref.leaves(sds, torch.float32)
    if phase == 'val':
        out = ref.validation_step(leaves, cfg, data, noise=noise)
    else:
        out = ref.training_step(phase, leaves, cfg, data, noise=noise)
        out['loss'].sum().backward()
    want = fixture_scalars(case, phase)
    for name, value in want.items():
        got = float(torch.as_tensor(out[name]).detach().double().sum())
        print('%s %-18s restated %.9g  reference %.9g' % (case, name, got, value))
        assert abs(got - value) <= 1e-5 * abs(value), (name, got, value)
    if case + '_occ' in FIX:
        rows = out['occupancy_attn'].numpy().astype(bool)
        assert np.array_equal(np.packbits(rows), FIX[case + '_occ'])
        assert int(rows.sum()) == int(FIX[case + '_stats'][0])
    if phase == 'val':
        counts = [[int(out['occ' + s].sum()), int(out['occ_target'].sum()), int((out['occ' + s] & out['occ_target']).sum())] for s in ('_full', '_nn1')]
        assert counts == FIX[case + '_metric_counts'].tolist()
        return
    assert ref.parameter_names(leaves, phase) == [str(n) for n in FIX[case + '_param_names']]
    norms, want_norms = ref.grad_norms(leaves, phase), FIX[case + '_grad_norms']
    worst = float(np.max(np.abs(norms - want_norms) / np.maximum(want_norms, 1e-30)))
    print('%s gradient norms: worst relative difference %.3e over %d parameters' % (case, worst, len(norms)))
    assert np.all(np.abs(norms - want_norms) <= 1e-3 * want_norms)


def test_the_fixture_is_the_problem_the_gpu_tests_rest_on():
    """every slice non-empty and all of them taken (under 1280 rows in total), so that the contrastive term sees every occupied row; few voxels near the
    threshold, so that at most a handful of rows may differ between a float32 and a float64 evaluation"""
    for case in ('C3_p3', 'C1_p3'):
        rows = np.unpackbits(FIX[case + '_occ']).astype(bool)
        groups, counts = ref.contrastive_ref.select(rows, 8, ref.HPARAMS['max_rows'])
        assert len(groups) == 8 and counts[0] == counts[1] < 1280
        assert FIX[case + '_stats'][1] <= 0.007 * rows.size


def make_step(phase, cfg_name='C3', **hparams):
    from rfuse.training import RefinementStep
    cfg = ref.rf_configs.get_config(cfg_name)
    return RefinementStep.from_config(cfg, phase, ref.make_modules(cfg), **hparams), cfg


@pytest.mark.parametrize('phase', [0, 1, 2, 3])
def test_parameters_are_the_references_optimiser_lists(phase):
    side = {'loss_side_task_retr': 0.5, 'loss_side_task_unet': 0.25} if phase == 3 else {}
    step, _ = make_step(phase, **side)
    assert [n for n, _ in step.named_parameters()] == [str(n) for n in FIX['C3_p%d_param_names' % phase]]
    params = step.parameters()
    assert all(a is b for a, (_, b) in zip(params, step.named_parameters())) and len({id(p) for p in params}) == len(params)


def test_hyper_parameters():
    from rfuse.training import RefinementStep
    step, cfg = make_step(0)
    assert {k: step.hparams[k] for k in ('weight_occupied', 'loss_reconstruction', 'loss_normal', 'attn_temprature', 'max_rows', 'loss_attn_contrastive')} == {
        'weight_occupied': 8, 'loss_reconstruction': 1, 'loss_normal': 0.5, 'attn_temprature': 0.05, 'max_rows': 1280, 'loss_attn_contrastive': 0.01}
    assert step.K == cfg['K'] and 'loss_side_task_retr' not in step.hparams and 'loss_side_task_unet' not in step.hparams
    mods = ref.make_modules(cfg)
    with pytest.raises(TypeError, match='loss_side_task_retr, loss_side_task_unet'):
        RefinementStep.from_config(cfg, 3, mods)
    with pytest.raises(TypeError, match='loss_side_task_unet'):
        RefinementStep.from_config(cfg, 3, mods, loss_side_task_retr=1.0)
    with pytest.raises(TypeError, match='unknown'):
        RefinementStep.from_config(cfg, 0, mods, attn_temperature=0.1)          # the reference spells it attn_temprature
    with pytest.raises(ValueError):
        RefinementStep.from_config(cfg, 4, mods)
    step = RefinementStep.from_config(cfg, 3, mods, loss_side_task_retr=1.0, loss_side_task_unet=2.0, weight_occupied=4, attn_temprature=0.1, max_rows=64)
    assert step.shape_loss.weight_occupied == 4 and step.loss_attn.temperature == 0.1 and step.loss_attn.max_rows == 64


def test_cpu_tensors_raise():
    from rfuse import ops
    step, cfg = make_step(0)
    s_in = cfg['dataset_train']['input_chunk_size']
    batch = {'input': torch.zeros(1, 1, s_in, s_in, s_in), 'target': torch.zeros(1, 1, 64, 64, 64), 'retrieval': torch.zeros(1, cfg['K'], 64, 64, 64)}
    flags = [p.requires_grad for m in step.networks().values() for p in m.parameters()]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        step.training_step(batch)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        step.validation_step(batch)
    with pytest.raises(TypeError):
        step.training_step({'target': batch['target']})
    assert flags == [p.requires_grad for m in step.networks().values() for p in m.parameters()]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.attn_occupancy_rows(torch.zeros(1, 1, 8, 8, 8), 0.1, 0.02, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.pointwise_tanh_backward(torch.zeros(1, 2, 8), torch.zeros(1, 1, 8), torch.zeros(1, 1, 8), torch.zeros(1, 2, 1, 1, 1))


def test_the_tenth_header_is_bound_and_built():
    import sys
    from pathlib import Path
    from rfuse import _lib
    assert set(_lib.STEP_SIGNATURES) == {'rf_pointwise_tanh_backward', 'rf_pointwise_tanh_backward_ws_bytes', 'rf_pointwise_tanh_backward_grid_threads',
                                         'rf_attn_occupancy_rows'}
    assert _lib.is_status('rf_pointwise_tanh_backward', _lib.STEP_SIGNATURES) and _lib.is_status('rf_attn_occupancy_rows', _lib.STEP_SIGNATURES)
    assert not set(_lib.STEP_SIGNATURES) & set(_lib.SIGNATURES)
    sys.path.insert(0, str(Path(_lib.__file__).resolve().parents[1] / 'csrc'))
    import build
    assert 'refinement_step.hip' in build.SOURCES and '-ffp-contract=off' in build.EXTRA_FLAGS['refinement_step.hip']
