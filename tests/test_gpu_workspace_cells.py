"""The kernel instances of every workspace cell of the wave path (tests/workspace_cells.py has the table and the sweep behind it):
per cell the full, lean and refine solve instances, the six rollout instances and the eval instance, each launched through the
feature it belongs to and compared as that feature's own GPU test compares it on the headline class -- whose helpers are imported,
not restated.  8 agents per class; the per-step loops take updates of 0.4 knot intervals, so that the third crosses a knot
(tests/test_gpu_factor_instances.py); the rollout variants keep the update time 0.1 s and the sample time 0.01 s of their features'
tests (the disturbance and the log are laid out on that grid) and run two updates past the first knot crossing of the class.

Every case states its cell from the plan (`build_class`) and from the handle (`solver.workspace()`) before it launches anything."""
import functools

import numpy as np
import pytest

from workspace_cells import CASES, WAVE_CASES, build_class, threads

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)
N = 8
TOL_X_PORT = 1e-4                  # device loop against the host build: the bound of tests/test_gpu_factor_instances.py
KEYS = ('x', 'lam', 'p', 'status', 'iters')
ids = lambda cases: [c.id for c in cases]


def _builder(case, drift=False):
    """build(n) -> (problem, P) for the imported helpers.  drift: the obstacles set moving by the script file's `_drift` -- the first
    eight of them, as many as a rollout moves (include/omgx.h omgx_obstacle_script) -- here, not through the helpers' own flag."""
    def build(n):
        problem, P, _ = build_class(case, n)
        if drift:
            import types
            from test_gpu_obstacle_script import _drift
            _drift(types.SimpleNamespace(father=problem.father, environment=types.SimpleNamespace(obstacles=problem.environment.obstacles[:8])), P)
        return problem, P
    return build


def _checker(case):
    """Called by an imported helper with the handle it made: the handle reports the cell of the table."""
    plan = build_class(case, 1)[2]
    return lambda solver: _assert_cell(case, solver, plan)


@functools.lru_cache(maxsize=None)
def _knot_time(case):
    return float(build_class(case, 1)[0].knot_time)


def _update_time(case):
    return 0.4 * _knot_time(case)        # updates at 0.4, 0.8, 1.2 knot intervals: the third crosses a knot


@functools.lru_cache(maxsize=None)
def _steps_over_a_crossing(case):
    """(K, k_cross): updates of 0.1 s up to two past the first knot crossing of the class, and the update that crosses."""
    from omgtools.splines import step_clock
    t, k = 0.0, 0
    while True:
        t, _, _, crossed = step_clock(t, 0.1, _knot_time(case), 10.0)
        k += 1
        if crossed:
            return k + 2, k


def _assert_cell(case, solver, plan):
    info = solver.workspace()
    assert info['mode'] == plan['ws_mode'] == case.mode and info['lds_bytes'] == plan['lds_bytes'], (case.id, info, plan['ws_mode'], plan['lds_bytes'])
    return info


def _device(case, **options):
    import torch
    from omgtools.batch import BatchP2P
    problem, P, plan = build_class(case, N)
    gpu = BatchP2P(problem, P, ops='hip', device=torch.device('cuda', 0), options=dict(OPTS, **options), update_time=_update_time(case))
    _assert_cell(case, gpu.solver, plan)
    return gpu


@functools.lru_cache(maxsize=None)
def _host_loop(case, refine):
    """Cold solve and three steps of the host build (computed once per class and option, read-only from then on)."""
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    from test_gpu_factor_instances import _loop
    problem, P, _ = build_class(case, N)
    ref = BatchP2P(problem, P, ops=port_binding, options=dict(OPTS, refine=refine), update_time=_update_time(case))
    ref.n_threads = 8
    return _loop(ref, 3)


def _device_loop(case, refine):
    from test_gpu_factor_instances import _loop
    gpu = _device(case, refine=refine)
    try:
        got, crossed = _loop(gpu, 3)
        inst = gpu.solver.workspace()['last_instance']
        lo, hi = gpu.tpl.entry_range(gpu.veh.label, 'splines_seg0', 'var')
    finally:
        gpu.solver.close()
    return got, crossed, inst, lo, hi


@pytest.mark.parametrize('case', CASES, ids=ids(CASES))
def test_per_step_loop_matches_the_host_build(case):
    """Statuses and iteration counts equal, spline coefficients within TOL_X_PORT, after the cold solve and each of three steps.  The
    class off the wave path has no rollout instance: `rollout` is an error there, not a fall-back."""
    from omgtools.backend import OmgxError
    want, crossed_ref = _host_loop(case, 0)
    got, crossed, inst, lo, hi = _device_loop(case, 0)
    assert crossed == crossed_ref == 1
    if case.wave_path:
        assert inst == 1                                    # (the plain loop of a wave-path class runs the lean instance)
    for k, ((x, st, it), (xr, st_r, it_r)) in enumerate(zip(got, want)):
        worst = float(np.abs(x[:, lo:hi] - xr[:, lo:hi]).max())
        print('%s mode %d, %d per CU, %d threads, %s: iters %s, max |coefficient diff| %.2e (bound %.0e)'
              % (case.id, case.mode, case.per_cu, threads(case), 'cold' if k == 0 else 'step %d' % k, it.tolist(), worst, TOL_X_PORT))
        assert np.array_equal(st, st_r), (k, st, st_r)
        assert np.array_equal(it, it_r), (k, it, it_r)
        assert worst < TOL_X_PORT, (k, worst)
    if not case.wave_path:
        gpu = _device(case)
        try:
            gpu.solve_cold(bends=())
            with pytest.raises(OmgxError):
                gpu.rollout(2)
        finally:
            gpu.solver.close()


@pytest.mark.parametrize('case', WAVE_CASES, ids=ids(WAVE_CASES))
def test_lean_and_full_instance_same_bits(case):
    """The plain loop (lean instance) against the loop with the stop rule that never holds (full instance), as
    tests/test_gpu_lean_instance.py: the five arrays the same bits after every launch."""
    from test_gpu_lean_instance import _loop
    kw = dict(build=_builder(case), n_steps=3, update_time=_update_time(case), check=_checker(case))
    plain, inst_plain, crossed, _ = _loop(N, 1, rule=False, **kw)
    ruled, inst_ruled, crossed_r, under_way = _loop(N, 1, rule=True, **kw)
    assert crossed == crossed_r == 1
    assert all(i == [1] for i in inst_plain), inst_plain
    assert all(i == [0] for i in inst_ruled), inst_ruled
    assert (under_way == 1).all() and (plain[0]['iters'] > 0).all()
    for k, (a, b) in enumerate(zip(plain, ruled)):
        for key in KEYS:
            assert np.array_equal(a[key], b[key]), (case.id, k, key, int((a[key] != b[key]).sum()))


@pytest.mark.parametrize('case', WAVE_CASES, ids=ids(WAVE_CASES))
def test_refined_loop_takes_the_decisions_of_the_host_build(case):
    """`refine` = 1 runs the refine instance (reported as 0: not the lean one); the bounds of `test_refined_steps_match_port`
    (tests/test_gpu_solver.py) at tol 1e-3: statuses equal and 0, iteration counts within 1, x within 1e-6."""
    want, crossed_ref = _host_loop(case, 1)
    got, crossed, inst, lo, hi = _device_loop(case, 1)
    assert crossed == crossed_ref == 1 and inst == 0
    for k, ((x, st, it), (xr, st_r, it_r)) in enumerate(zip(got, want)):
        worst, d_it = float(np.abs(x - xr).max()), int(np.abs(it - it_r).max())
        print('%s refine, %s: iters %s, largest difference of a count %d, max |x diff| %.2e (bound 1e-6), max |coefficient diff| %.2e'
              % (case.id, 'cold' if k == 0 else 'step %d' % k, it.tolist(), d_it, worst, float(np.abs(x[:, lo:hi] - xr[:, lo:hi]).max())))
        assert np.array_equal(st, st_r) and (st == 0).all(), (k, st, st_r)
        assert d_it <= 1, (k, it, it_r)
        assert worst < 1e-6, (k, worst)


@pytest.mark.parametrize('case', WAVE_CASES, ids=ids(WAVE_CASES))
def test_rollout_equals_the_stepwise_loop_bit_for_bit(case):
    """`rollout(3)` against 3 x `step` on a twin, as tests/test_gpu_rollout.py: the five arrays and the per-step logs."""
    import torch
    from test_gpu_rollout import _pair
    a, b = _pair(N, build=_builder(case), update_time=_update_time(case))
    try:
        _assert_cell(case, a.solver, build_class(case, 1)[2])
        K = 3
        it_log = torch.zeros((K, N), dtype=torch.int32, device=a.dev)
        st_log = torch.full((K, N), -1, dtype=torch.int32, device=a.dev)
        crossings = a.rollout(K, iters_log=it_log, status_log=st_log)
        it_ref, st_ref, crossed_ref = [], [], 0
        for _ in range(K):
            crossed_ref += int(b.step())
            it_ref.append(b.iters.clone()); st_ref.append(b.status.clone())
        torch.cuda.synchronize()
        assert crossings == crossed_ref == 1
        assert abs(a.time - b.time) < 1e-12
        assert torch.equal(it_log, torch.stack(it_ref)) and torch.equal(st_log, torch.stack(st_ref))
        assert (it_log > 0).all()
        for name in KEYS:
            assert torch.equal(getattr(a, name), getattr(b, name)), (case.id, name)
    finally:
        a.solver.close(); b.solver.close()


@pytest.mark.parametrize('with_script', [False, True], ids=['plant', 'plant_script'])
@pytest.mark.parametrize('case', WAVE_CASES, ids=ids(WAVE_CASES))
def test_plant_rollouts_equal_the_stepwise_loop(case, with_script):
    """The plant instance and the plant-with-script instance of the cell, set up and compared as
    tests/test_gpu_plant.py / tests/test_gpu_obstacle_script.py do."""
    import test_gpu_obstacle_script as sc
    import test_gpu_plant as pl
    K, k_cross = _steps_over_a_crossing(case)
    build = _builder(case)
    if with_script:
        ev = sc._events(N, t_max=0.1 * K, n_obst=min(case.n_obs, 8), t_cross=0.1 * k_cross - 0.05)
        a, b = (sc._mk(N, events=ev, plant=True, build=_builder(case, drift=True), max_updates=K + 1) for _ in range(2))
    else:
        a, b = (pl._mk(N, max_updates=K + 1, build=build) for _ in range(2))
    try:
        _assert_cell(case, a.solver, build_class(case, 1)[2])
        crossings = a.rollout(K)
        for _ in range(K):
            b.step()
        sc._equal(a, b, True) if with_script else pl._equal_everywhere(a, b)
        s, ps = a.signals(), a.plant_state()
        assert crossings == 1 and (s['count'] == 1 + 10 * (K + 1)).all() and not s['overflow'].any()
        assert (ps['n_upd'] == K + 1).all() and not ps['overflow'].any()
    finally:
        pl._close(a, b)


@pytest.mark.parametrize('case', WAVE_CASES, ids=ids(WAVE_CASES))
def test_script_rollout_equals_the_stepwise_loop(case):
    """The script instance of the cell, as tests/test_gpu_obstacle_script.py: drifting obstacles, six events per agent, one of them
    inside the knot-crossing update; and the script acted."""
    import test_gpu_obstacle_script as sc
    K, k_cross = _steps_over_a_crossing(case)
    build = _builder(case, drift=True)
    ev = sc._events(N, t_max=0.1 * K, n_obst=min(case.n_obs, 8), t_cross=0.1 * k_cross - 0.05)      # (events on every moving obstacle)
    a, b = (sc._mk(N, events=ev, build=build) for _ in range(2))
    c = sc._mk(N, cold=False, build=build)
    try:
        _assert_cell(case, a.solver, build_class(case, 1)[2])
        crossings = a.rollout(K)
        for _ in range(K):
            b.step()
        sc._equal(a, b)
        assert crossings == 1 and len(a.obst) == min(case.n_obs, 8)
        for _ in range(K):
            c._advance_obstacles(0.0, 0.1)
        ox, _, _, nd = a.obst[0]
        assert not np.array_equal(c.p[:, ox:ox + nd].cpu().numpy(), a.p[:, ox:ox + nd].cpu().numpy())
    finally:
        sc._close(a, b, c)


@pytest.mark.parametrize('plant', [False, True], ids=['mission', 'plant_mission'])
@pytest.mark.parametrize('case', WAVE_CASES, ids=ids(WAVE_CASES))
def test_mission_in_one_launch_is_the_mission_step_by_step(case, plant):
    """The mission instances of the cell, as tests/test_mission_gpu.py: `rollout(K)` against K x `rollout(1)`, logs included.  Two
    goals: the one in p moved to 0.3 m from the start, with a stop tolerance of 0.28 m (just inside: the cold solve, which applies the
    rule too, still runs, and the switch falls into the first few updates), then the class's own goal, which every other agent flies
    -- six updates more than the plain cases, so that the second leg's own clock crosses a knot; the others stop at the first."""
    import torch
    import test_mission_gpu as ms
    from mission_cases import fly, snapshot
    from test_gpu_plant import _near_targets
    K, k_cross = _steps_over_a_crossing(case)
    K += 6
    far = {}

    def build(n):
        problem, P = _builder(case)(n)
        lo = problem.father.template.entry_range(problem.vehicles[0].label, 'poseT', 'par')[0]
        far['goals'] = P['p'][:, lo:lo + 2].copy()
        _near_targets(problem, P, agents=range(n))
        return problem, P
    kw = dict(max_iter_step=40) if plant else {}
    n_goals = (np.arange(N) % 2).astype(np.int32)
    pair = []
    try:
        for _ in range(2):
            m, _P = ms._device(N, plant, stop_tol=0.28, warmup=0, mission=False, build=build, **kw)
            assert (m.host('under_way') != 0).all()           # (nobody arrived in the cold solve)
            pair.append(m)
            m.mission(far['goals'][:, None, :], n_goals)
        one, many = pair
        _assert_cell(case, one.solver, build_class(case, 1)[2])
        it_log = torch.zeros((K, N), dtype=torch.int32, device=one.dev)
        st_log = torch.full((K, N), -1, dtype=torch.int32, device=one.dev)
        one.rollout(K, iters_log=it_log, status_log=st_log)
        hist = fly(many, K)
        ms._same_bits(one, many, hist)
        assert np.array_equal(it_log.cpu().numpy(), np.array([h['iters'] for h in hist]))
        assert np.array_equal(st_log.cpu().numpy(), np.array([h['status'] for h in hist]))
        assert abs(one.time - many.time) < 1e-12
        st = snapshot(one)
        print('%s: leg %s, arrivals at the first goal %s' % (case.id, st['leg'].tolist(), st['arrivals'][:, 0].tolist()))
        assert (st['arrivals'][n_goals >= 1, 0] >= 0).any() and st['leg'].max() >= 1          # at least one switch happened
        assert (st['leg'][n_goals == 0] == 0).all()
        # ... and a switched agent is still under way on its second leg, solved at the last step, its leg clock past a knot crossing
        second = (st['leg'] == 1) & st['under_way'] & (st['clock'] >= k_cross) & (it_log[-1].cpu().numpy() > 0)
        assert second.any(), (st['leg'], st['clock'], k_cross)
    finally:
        for m in pair:
            m.solver.close()


@pytest.mark.parametrize('case', CASES, ids=ids(CASES))
def test_eval_instance_matches_the_oracle(case):
    """`omgx_batch_eval` of the cell at seeded random points against oracle/nlp_numpy.py, to the 1e-10 of tests/test_gpu_eval.py."""
    from test_gpu_eval import oracle_parity
    problem, P, _ = build_class(case, 3)
    oracle_parity(problem, P, 3, case.id, check=_checker(case))
