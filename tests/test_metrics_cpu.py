"""CPU: the evaluation metrics' host side (rfuse/metrics.py; reference util/metrics.py:6-89) -- construction with the reference's arguments, state
names, reset, compute() of an empty metric, f1, the refusal of CPU input, the reference-generated fixture against a numpy brute force, and the
cross-rank sum of compute() over gloo."""
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = Path(__file__).resolve().parents[1]

STATES = {'IoU': 'iou_sum', 'Chamfer3D': 'cd_sum', 'Precision': 'precision_sum', 'Recall': 'recall_sum'}


def fixture_updates(golden_dir):
    z = np.load(golden_dir / 'metrics.npz')
    out, u = [], 0
    while 'u%d_shape' % u in z.files:
        shape = tuple(int(s) for s in z['u%d_shape' % u])
        n = int(np.prod(shape))
        grids = [np.unpackbits(z['u%d_%s' % (u, k)])[:n].astype(bool).reshape(shape) for k in ('pred', 'target')]
        out.append((grids[0], grids[1], z['u%d_stats' % u], z['u%d_states' % u]))
        u += 1
    return out, z['compute']


def brute_stats(pred, target):
    """numpy float64 brute force: n_pred, n_target, n_inter, s_tp, s_pt per volume"""
    rows = []
    for p, t in zip(pred[:, 0], target[:, 0]):
        P, T = np.argwhere(p).astype(np.float64), np.argwhere(t).astype(np.float64)
        s = [0, 0]
        if len(P) and len(T):
            for i, (a, b) in enumerate(((T, P), (P, T))):
                s[i] = int(sum(((a[k:k + 256, None] - b[None]) ** 2).sum(-1).min(1).sum() for k in range(0, len(a), 256)))
        rows.append([len(P), len(T), int((p & t).sum())] + s)
    return np.array(rows, np.int64)


def test_construction_state_names_reset_and_empty_compute():
    from rfuse import metrics
    ms = torch.nn.ModuleList([getattr(metrics, n)(compute_on_step=False) for n in STATES])
    for m, (name, state) in zip(ms, STATES.items()):
        assert type(m).__name__ == name and m.compute_on_step is False
        assert list(m.buffers()) == [] and list(m.parameters()) == []    # states are plain attributes (rfuse/metrics.py docstring)
        assert getattr(m, state).dtype == torch.float32 and getattr(m, state).shape == ()
        assert torch.isnan(m.compute())                      # 0 / 0, as the reference's float state / float total
        getattr(m, state).fill_(3.0)
        m.total.fill_(4.0)
        assert m.compute().item() == 0.75
        m.reset()
        assert getattr(m, state).item() == 0.0 and m.total.item() == 0.0
    assert ms.state_dict() == {}                             # as torchmetrics': checkpoints carry no metric keys
    ms.double()                                              # ... but .to() / .double() / .cuda() move and cast them
    assert all(getattr(m, s).dtype == torch.float64 and m.total.dtype == torch.float64 for m, s in zip(ms, STATES.values()))
    metrics.IoU(compute_on_step=True, process_group=None, dist_sync_on_step=False)
    p, r = torch.tensor(0.5), torch.tensor(0.25)
    assert metrics.f1(p, r).item() == pytest.approx(2 * 0.5 * 0.25 / 0.75)


def test_cpu_input_has_no_fallback():
    from rfuse import metrics
    x = torch.zeros(2, 1, 4, 4, 4, dtype=torch.bool)
    for cls in (metrics.IoU, metrics.Chamfer3D, metrics.Precision, metrics.Recall):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            cls(compute_on_step=False)(x, x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        metrics.occupancy_stats(x.float(), x.float(), threshold=0.5)


def test_fixture_is_self_consistent(golden_dir):
    """the counts and squared-distance sums the reference's classes saw (through the exact stand-in) are what a brute force over the stored grids
    gives, and the stored states follow from them by the reference's float32 expressions"""
    ups, compute = fixture_updates(golden_dir)
    assert len(ups) == 3 and sum(len(p) for p, _, _, _ in ups) == 9
    acc = np.zeros(8, np.float64)
    for pred, target, stats, states in ups:
        np.testing.assert_array_equal(brute_stats(pred, target), stats)
        n_p, n_t, n_i, s_tp, s_pt = (stats[:, k] for k in range(5))
        union = n_p + n_t - n_i
        f = np.float32
        iou = [f(i) / (f(un) + f(1e-5)) for i, un in zip(n_i, union) if un > 0]
        ok = (n_p > 0) & (n_t > 0)
        cd = [f(f(a / nt) + f(b / npp)) for a, b, nt, npp, v in zip(s_tp, s_pt, n_t, n_p, ok) if v]
        acc += [sum(iou), len(iou), sum(cd), len(cd), sum(f(i) / (f(x) + f(1e-5)) for i, x in zip(n_i, n_p)), len(n_p),
                sum(f(i) / (f(x) + f(1e-5)) for i, x in zip(n_i, n_t)), len(n_t)]
        np.testing.assert_allclose(states, acc, rtol=1e-6)
        assert (states[1::2] == acc[1::2]).all()
    np.testing.assert_allclose(compute, acc[0::2] / acc[1::2], rtol=1e-6)
    assert ups[0][2][3].tolist() == [1, 1, 0, 3 * 63 ** 2, 3 * 63 ** 2]          # single voxels at opposite corners


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _sum_worker(rank, world, port, out_dir, ddp):
    for p in (str(REPO), str(REPO / 'retrieval-fuse_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from rfuse import metrics
    net = torch.nn.Module()
    net.lin = torch.nn.Linear(3, 1)
    net.metrics = torch.nn.ModuleList([getattr(metrics, name)(compute_on_step=False) for name in STATES])
    for m, state in zip(net.metrics, STATES.values()):
        getattr(m, state).fill_(float(1 + 5 * rank))             # rank 0: 1 / 2, rank 1: 6 / 4 -> (1 + 6) / (2 + 4)
        m.total.fill_(float(2 + 2 * rank))
    if ddp:
        # the reference trainer's setting (Lightning DDP, broadcast_buffers=True): training steps between validation passes, states never reset
        net.forward = lambda x: net.lin(x)
        model = torch.nn.parallel.DistributedDataParallel(net)
        for step in range(2):
            model(torch.full((4, 3), float(rank + step))).sum().backward()
    lines = []
    for m, (name, state) in zip(net.metrics, STATES.items()):
        v = m.compute().item()
        lines.append('%s %r %r %r' % (name, v, getattr(m, state).item(), m.total.item()))
    (Path(out_dir) / ('rank%d.txt' % rank)).write_text('\n'.join(lines))
    dist.destroy_process_group()


@pytest.mark.parametrize('ddp', [False, True])
def test_compute_sums_states_across_ranks(tmp_path, ddp):
    """torchmetrics' dist_reduce_fx='sum': compute() on every rank sees the sum of all ranks' states; the local states stay as they were -- also when
    the metrics sit in a module that DistributedDataParallel wraps and trains (its buffer broadcast must not reach them)"""
    mp.spawn(_sum_worker, args=(2, _free_port(), str(tmp_path), ddp), nprocs=2, join=True)
    for rank in range(2):
        lines = (tmp_path / ('rank%d.txt' % rank)).read_text().splitlines()
        assert len(lines) == 4
        for line in lines:
            name, v, s, t = line.split()
            assert float(v) == pytest.approx(7 / 6, rel=1e-6), line
            assert float(s) == 1 + 5 * rank and float(t) == 2 + 2 * rank, line
