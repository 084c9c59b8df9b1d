"""The lean instance of the solve kernel (`ipm_solve_kernel<..., LEAN>`, `omgx_batch_last_instance`): a launch that uses none of the
optional features -- stop rule, fused store / signals, ADMM centre, prepared setup, restart pass or restart guesses, absolute
tolerances, refinement -- runs an instance with that code compiled out; every other launch runs the full one.  The library picks
per launch from the handle's state.  Both instances run the same statements on the agents they solve: the SAME BITS.

The comparison: the plain receding-horizon loop (lean) against the same loop with the stop rule installed with a NEGATIVE tolerance
-- a criterion that never holds (norms are not negative), so every agent is still solved at every update, by the full instance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_STEPS = 12      # (enough updates of 0.1 s to cross a knot of the config-2 horizon: asserted below)
KEYS = ('x', 'lam', 'p', 'status', 'iters')


def _parts(mpc):
    return mpc.parts if hasattr(mpc, 'parts') else [mpc]


def _instances(mpc):
    if hasattr(mpc, 'synchronize'):
        mpc.synchronize()
    return [m.solver.workspace()['last_instance'] for m in _parts(mpc)]


def _close(mpc):
    mpc.close() if hasattr(mpc, 'parts') else mpc.solver.close()


def _loop(B, n_streams, rule, build=None, n_steps=N_STEPS, check=None, **kw):
    """Cold solve (no restart guesses: they are a feature of the full instance) + n_steps steps; the five arrays after every launch and
    the instance every launch ran.  build(B) -> (problem, P): another class than config 2 (tests/test_gpu_workspace_cells.py); kw: of
    the loop (`update_time`); check(solver): called with every handle ahead of its first launch."""
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P, StreamedP2P
    problem, P = (build or workloads.holonomic_p2p)(B)
    dev = torch.device('cuda', 0)
    opts = dict(tol=1e-3, max_iter=300)
    mpc = BatchP2P(problem, P, ops='hip', device=dev, options=opts, **kw) if n_streams == 1 else \
        StreamedP2P(problem, P, n_streams=n_streams, device=dev, options=opts, **kw)
    try:
        if check is not None:
            for m in _parts(mpc):
                check(m.solver)
        if rule:
            mpc.stop_at_arrival(stop_tol=-1.0)
        log, inst, crossed = [], [], 0
        mpc.solve_cold(bends=())
        for k in range(n_steps + 1):
            if k:
                crossed += int(bool(mpc.step()))
            log.append(dict((key, mpc.host(key).copy()) for key in KEYS))
            inst.append(_instances(mpc))
        under_way = None if not rule else mpc.host('under_way')
    finally:
        _close(mpc)
    return log, inst, crossed, under_way


@pytest.mark.parametrize('B,n_streams', [(64, 1), (1024, 3)])
def test_lean_and_full_instance_same_bits_across_a_crossing(B, n_streams):
    plain, inst_plain, crossed, _ = _loop(B, n_streams, rule=False)
    ruled, inst_ruled, crossed_r, under_way = _loop(B, n_streams, rule=True)
    assert crossed >= 1 and crossed_r == crossed
    assert all(i == [1] * n_streams for i in inst_plain), inst_plain        # lean at every launch of the plain loop
    assert all(i == [0] * n_streams for i in inst_ruled), inst_ruled        # full at every launch with the rule installed
    assert (under_way == 1).all()                                           # the rule stopped nobody: every agent solved at every update
    assert (plain[0]['iters'] > 0).all()                                    # (the cold solves did run)
    for k, (a, b) in enumerate(zip(plain, ruled)):
        for key in KEYS:
            print('launch %d %s: %d of %d entries differ' % (k, key, int((a[key] != b[key]).sum()), a[key].size))
            assert np.array_equal(a[key], b[key]), (k, key)


def test_toggling_a_feature_between_launches_switches_the_instance():
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    B = 16
    problem, P = workloads.holonomic_p2p(B)
    mpc = BatchP2P(problem, P, ops='hip', device=torch.device('cuda', 0), options=dict(tol=1e-3, max_iter=300))
    try:
        assert _instances(mpc) == [0]                     # (nothing launched yet)
        mpc.solve_cold(bends=())
        assert _instances(mpc) == [1]
        mpc.stop_at_arrival(stop_tol=-1.0)                # stop rule on, off
        mpc.step()
        assert _instances(mpc) == [0]
        mpc.stop_at_arrival(on=False)
        mpc.step()
        assert _instances(mpc) == [1]
        mpc.record_signals(sample_time=0.01, max_updates=8)      # the log inside the solve on, off
        mpc.step()
        assert _instances(mpc) == [0]
        mpc.record_signals(on=False)
        mpc.step()
        assert _instances(mpc) == [1]
        mpc.solver.set_prepare(True)                      # the setup kernel on, off
        mpc.step()
        assert _instances(mpc) == [0]
        mpc.solver.set_prepare(False)
        mpc.step()
        assert _instances(mpc) == [1]
    finally:
        mpc.solver.close()


def test_restarts_and_absolute_tolerances_run_the_full_instance():
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    B = 16
    problem, P = workloads.holonomic_p2p(B)
    dev = torch.device('cuda', 0)
    mpc = BatchP2P(problem, P, ops='hip', device=dev, options=dict(tol=1e-3, max_iter=300))
    try:
        mpc.solve_cold()                                  # restart guesses inside the launch (omgx_batch_set_restarts)
        assert _instances(mpc) == [0]
        mpc.step()                                        # (taken off again after the cold solve)
        assert _instances(mpc) == [1]
    finally:
        mpc.solver.close()
    mpc = BatchP2P(problem, P, ops='hip', device=dev, options=dict(tol=1e-3, max_iter=300, compl_inf_tol=1e-4, constr_viol_tol=1e-4))
    try:
        mpc.solve_cold(bends=())
        assert _instances(mpc) == [0]
        mpc.step()
        assert _instances(mpc) == [0]
    finally:
        mpc.solver.close()


def test_stop_tolerance_contract_of_the_library():
    """`omgx_batch_set_stop` on a real handle: a negative tolerance (also -inf) is accepted -- a rule that never holds --, a NaN is
    refused with OMGX_E_INVALID and leaves the rule off (the next launch is lean again)."""
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = workloads.holonomic_p2p(8)
    mpc = BatchP2P(problem, P, ops='hip', device=torch.device('cuda', 0), options=dict(tol=1e-3, max_iter=300))
    try:
        mpc.solve_cold(bends=())
        for tol in (-1.0, -np.inf):
            mpc.stop_at_arrival(stop_tol=tol)
            mpc.step()
            assert _instances(mpc) == [0] and (mpc.host('under_way') == 1).all() and (mpc.host('iters') > 0).any()
        with pytest.raises(Exception):
            mpc.stop_at_arrival(stop_tol=float('nan'))
        mpc.step()
        assert _instances(mpc) == [1]
    finally:
        mpc.solver.close()
