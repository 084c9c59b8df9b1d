"""The slot queue of the persistent kernels (`next_slot` of ipm_solve_kernel / ipm_rollout_kernel, omg-tools_amd/csrc/omgx_device.h `queue_leave`).

A handle with more agents than resident workgroups hands its launch slots out through an atomic counter that the workgroup leaving
last resets for the next launch; a handle whose grid covers its batch gets no counter at all.  Which workgroup solves an agent
changes nothing about its result, so the same agents solved through the queue (one handle of n_slabs + 8 agents) and without it
(two handles of at most n_slabs agents each) must give THE SAME BITS, and a queue that was not reset -- or was reset under an add
still in flight -- shows in the launch statistics: a launch would solve fewer agents than the batch holds, or one twice."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)
NAMES = ('x', 'lam', 'status', 'iters')


def _resident_workgroups():
    """n_slabs of the config-2 class on this device: what a handle with more agents than that launches (`workspace()`)."""
    from omgtools import workloads
    from omgtools.backend import BatchSolver
    problem, _ = workloads.holonomic_p2p(8)
    probe = BatchSolver(problem.father.template, 4096, options=OPTS)
    try:
        n_slabs = int(probe.workspace()['n_slabs'])
    finally:
        probe.close()
    assert 8 <= n_slabs < 4096
    return n_slabs


def _handles():
    """(one, halves, B, n_slabs): the batch of n_slabs + 8 agents on one handle and as two handles of half of it each."""
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    n_slabs = _resident_workgroups()
    B = n_slabs + 8
    dev = torch.device('cuda', 0)
    problem, P = workloads.holonomic_p2p(B)
    one = BatchP2P(problem, P, ops='hip', device=dev, options=OPTS)
    halves = []
    for lo, hi in ((0, B // 2), (B // 2, B)):
        problem_h, P_h = workloads.holonomic_p2p(B)
        halves.append(BatchP2P(problem_h, dict(P_h, p=P_h['p'][lo:hi], x0=P_h['x0'][lo:hi]), ops='hip', device=dev, options=OPTS))
    assert one.solver.workspace()['n_slabs'] == n_slabs < B                   # the queue is in use
    for h in halves:
        assert h.solver.workspace()['n_slabs'] == h.B <= n_slabs              # a workgroup per agent: no queue
    return one, halves, B, n_slabs


def _assert_same_bits(one, halves, what):
    for name in NAMES:
        got = one.host(name)
        ref = np.concatenate([h.host(name) for h in halves])
        assert np.array_equal(got, ref), (what, name, int((got != ref).sum()))


def _close(one, halves):
    one.solver.close()
    for h in halves:
        h.solver.close()


def test_queue_and_no_queue_solve_the_same_bits_and_every_launch_counts_the_batch():
    import torch
    one, halves, B, _ = _handles()
    try:
        stats = torch.zeros((6, 4), dtype=torch.int64, device=one.dev)
        one.solver.set_stats(stats)
        one.solve_cold(bends=())
        for h in halves:
            h.solve_cold(bends=())
        _assert_same_bits(one, halves, 'cold')
        for k in range(3):
            crossed = one.step()
            for h in halves:
                assert h.step() == crossed
            _assert_same_bits(one, halves, 'step %d' % k)
        one.solver.set_stats(None)
        torch.cuda.synchronize()
        s = stats.cpu().numpy()
        print('agents per launch (cold, 3 steps, unused, unused):', s[:, 3].tolist(), 'of', B)
        assert (s[:4, 3] == B).all(), s[:, 3]                                 # every launch solved every agent once
        assert (s[4:] == 0).all()
    finally:
        _close(one, halves)


def test_rollout_queue_and_no_queue_solve_the_same_bits():
    import torch
    one, halves, B, _ = _handles()
    try:
        K = 2
        stats = torch.zeros((K + 3, 4), dtype=torch.int64, device=one.dev)
        for m in [one] + halves:
            m.solve_cold(bends=())
        one.solver.set_stats(stats)
        crossed = one.rollout(K)
        for h in halves:
            assert h.rollout(K) == crossed
        _assert_same_bits(one, halves, 'rollout')
        # the queue was left reset: a second launch of either kind hands every agent out once again
        one.rollout(1)
        one.step()
        for h in halves:
            h.rollout(1)
            h.step()
        _assert_same_bits(one, halves, 'rollout, rollout, step')
        one.solver.set_stats(None)
        torch.cuda.synchronize()
        s = stats.cpu().numpy()
        print('agents per step (rollout of 2, rollout of 1, step, unused):', s[:, 3].tolist(), 'of', B)
        assert (s[:K + 2, 3] == B).all(), s[:, 3]
        assert (s[K + 2:] == 0).all()
    finally:
        _close(one, halves)
