"""`BatchP2P.mission` on the host twin (`HostP2P`, oracle port as solver): a list of goals per agent flown inside `rollout` -- the leg
switch is the reference's `reinitialize` + first update with `enforce_states` (pure assignments and numpy's linspace), an agent
without further goals is the stop-rule loop bit for bit, and from a leg start on an agent is the bits of a fresh batch built from its
leg-start row and guess.  The device loop is held against this twin in tests/test_mission_gpu.py."""
import numpy as np
import pytest

from mission_cases import STOP_TOL, fly, mission_batch, mission_goals

OPTS = dict(tol=1e-3, max_iter=300)


def _host(n=8, **kw):
    from oracle import port_binding
    return mission_batch(n, port_binding, OPTS, **kw)


@pytest.fixture(scope='module')
def flight():
    """One mission of 8 agents on the host, 70 updates by `rollout(1)`, every update's arrays kept."""
    m, P = _host()
    return m, P, fly(m, 70)


def test_agents_switch_finish_and_carry_on_at_different_updates(flight):
    """The mission the tests fly does what they need: every agent with a further goal starts its second leg within 40 updates, and one
    agent has finished its whole mission while another is still under way -- and the protocol's own invariants: a leg has at least one
    update, `under_way` goes only at the last goal, `arrivals` holds the steps at which `leg` moved."""
    m, P, hist = flight
    n_goals = m._ms['n_goals']
    leg = np.array([h['leg'] for h in hist])
    under = np.array([h['under_way'] for h in hist])
    arrivals = hist[-1]['arrivals']
    assert set(n_goals.tolist()) == {0, 1, 2, 3}
    assert (leg[39][n_goals >= 1] >= 1).all()                         # (1) the second leg has begun within K = 40 updates
    assert any((~under[k]).any() and under[k].any() and (leg[k][~under[k]] == n_goals[~under[k]]).all() for k in range(40))      # (2)
    assert (np.diff(leg, axis=0) >= 0).all() and (np.diff(leg, axis=0) <= 1).all() and (leg <= n_goals).all()
    for b in range(m.B):
        moved = [k for k in range(len(hist)) if leg[k, b] != (leg[k - 1, b] if k else 0)]
        assert arrivals[b, :len(moved)].tolist() == moved and len(set(moved)) == len(moved)
        for k in moved:                                               # a leg start is a cold solve on the leg's own clock 0
            assert hist[k]['clock'][b] == 0 and hist[k]['p'][b, m.o_t] == 0.0 and hist[k]['iters'][b] >= 1
        gone = np.flatnonzero(~under[:, b])
        if len(gone):
            assert leg[gone[0], b] == n_goals[b] and arrivals[b, n_goals[b]] == gone[0] and not under[gone[0]:, b].any()
            assert (np.array([h['iters'][b] for h in hist[gone[0]:]]) == 0).all()
        else:
            assert arrivals[b, leg[-1, b]] == -1
    assert (np.array([h['status'] for h in hist]) == 0).all()


def test_the_leg_switch_is_the_references_reinitialize(cfg2_small):
    """`mission_advance` (the switch without the solve) on a batch every agent of which meets a wide stop rule: the coefficients are
    `np.linspace(p[state0], goal, L)` per axis -- the bits --, every other variable the first guess's, the multipliers zero, poseT the
    goal, input0 and t zero, state0 where the vehicle is, clock 0; an agent without a further goal stops instead and keeps everything."""
    m, P = _host(warmup=3, mission=False)
    m.stop_at_arrival(stop_tol=100.0)                                 # (from here on every agent has arrived, wherever it is)
    goals, n_goals = mission_goals(m)
    m.mission(goals, n_goals)
    st = m.mission_state()
    assert (st['clock'] == 3).all() and (st['leg'] == 0).all() and (st['arrivals'] == -1).all()
    before = dict((nm, getattr(m, nm).copy()) for nm in ('x', 'lam', 'p'))
    m.mission_advance()
    n, L, o_pose = m.n_dim, m.L, m._ms['o_pose']
    for b in range(m.B):
        if n_goals[b] == 0:
            assert not m.under_way[b] and st['arrivals'][b, 0] == 0 and st['leg'][b] == 0 and st['clock'][b] == 3
            for nm in before:
                assert np.array_equal(getattr(m, nm)[b], before[nm][b])
            continue
        s = before['p'][b, m.o_state0:m.o_state0 + n]
        want = np.asarray(P['x0'][0], dtype=float).copy()
        want[m.o_spl:m.o_spl + n * L] = np.concatenate([np.linspace(s[k], goals[b, 0, k], L) for k in range(n)])
        assert np.array_equal(m.x[b], want) and not m.lam[b].any()
        pw = before['p'][b].copy()
        pw[o_pose:o_pose + n], pw[m.o_input0:m.o_input0 + n], pw[m.o_t] = goals[b, 0], 0.0, 0.0
        assert np.array_equal(m.p[b], pw)
        assert m.under_way[b] and st['leg'][b] == 1 and st['clock'][b] == 0 and st['arrivals'][b].tolist() == [0, -1, -1, -1]


def test_without_further_goals_a_mission_is_the_stop_rule_loop():
    """n_goals = 0 everywhere: `rollout(1)` with a mission on is `step()` under `stop_at_arrival`, bit for bit, for every agent under
    way; an agent that has stopped keeps the plan it had at that step (the stepwise loop goes on shifting it: tests/test_gpu_rollout.py)."""
    ruled, _ = _host(6, mission=False)
    flown, _ = _host(6, mission=False)
    goals, _ = mission_goals(flown)
    flown.mission(goals, np.zeros(6, dtype=np.int32))
    was = np.ones(6, dtype=bool)
    x_at_stop = {}
    for k in range(27):
        ruled.step(); flown.rollout(1)
        now = ruled.under_way.copy()
        assert np.array_equal(flown.under_way, now), k
        for nm in ('x', 'lam', 'p', 'iters', 'status'):
            assert np.array_equal(getattr(flown, nm)[now], getattr(ruled, nm)[now]), (k, nm)
        assert (flown.iters[~now] == 0).all()
        for b in np.flatnonzero(was & ~now):
            x_at_stop[b] = ruled.x[b].copy()
        was = now
    assert 0 < was.sum() < 6 and abs(flown.time - ruled.time) < 1e-12
    for b, xb in x_at_stop.items():
        assert np.array_equal(flown.x[b], xb)
    assert (flown.mission_state()['leg'] == 0).all() and np.array_equal(flown.mission_state()['arrivals'][:, 0] >= 0, ~was)


def test_from_a_leg_start_on_an_agent_is_a_fresh_batch(flight):
    """The leg-start solve and the updates behind it, over a knot crossing of the leg's own clock, are the bits of a fresh `HostP2P`
    built from the agent's leg-start row of p and the linspace guess, run with `solve_cold(bends=())` and `step()`."""
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    m, P, hist = flight
    n, L, checked = m.n_dim, m.L, 0
    for b in range(m.B):
        for k in range(1, len(hist) - 13):
            if hist[k]['leg'][b] == hist[k - 1]['leg'][b] or not all(h['under_way'][b] and h['leg'][b] == hist[k]['leg'][b] for h in hist[k:k + 13]):
                continue
            s_old = hist[k - 1]['p'][b, m.o_state0:m.o_state0 + n]
            goal = m._ms['goals'][b, hist[k]['leg'][b] - 1]
            guess = np.asarray(P['x0'][0], dtype=float).copy()
            guess[m.o_spl:m.o_spl + n * L] = np.concatenate([np.linspace(s_old[a], goal[a], L) for a in range(n)])
            fresh = BatchP2P(m.problem, dict(P, p=hist[k]['p'][b:b + 1], x0=guess[None]), ops=port_binding, options=OPTS)
            fresh.solve_cold(bends=())
            crossings = 0
            for j in range(13):
                if j:
                    crossings += int(fresh.step())
                for nm in ('x', 'lam', 'p', 'iters', 'status'):
                    assert np.array_equal(getattr(fresh, nm)[0], hist[k + j][nm][b]), (b, k, j, nm)
                assert hist[k + j]['clock'][b] == j
            assert crossings == 1
            checked += 1
            break
    assert checked >= 2


@pytest.mark.parametrize('tag', ['ideal', 'plant'])
def test_a_goal_change_is_what_the_reference_hands_its_solver(tag):
    """tests/golden/mission_holonomic.npz (generate_mission_golden.py): the reference's own `Holonomic` + `Point2point` + `Deployer` through a
    run, `set_terminal_conditions`, `Deployer.reset()` and two more updates, its solver replaced by a recorder that returns stored plans.
    The host twin, fed the same plans, hands its solver the same x0 and p at the leg's first update (the linspace guess from the stale
    state0, the enforced state, input0 = 0, t = 0, a cold solve) and the same p at the second, and logs the same columns: to 1e-12 with
    the ideal options (assignments, linspace and the existing prediction), within the deviation of the reference's odeint that the
    plant fixture records where the vehicle is simulated."""
    import os
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    g = np.load(os.path.join(here, 'mission_holonomic.npz'), allow_pickle=True)
    ode = np.load(os.path.join(here, 'plant_holonomic.npz'))
    problem, P = workloads.holonomic_p2p(1)
    tpl = problem.father.template
    for lay, ours in ((g['var_layout'], tpl.var_layout), (g['par_layout'], tpl.par_layout)):
        for nm, off, r, c in lay:
            assert ours[tuple(nm.split('/'))] == (off, r, c), nm
    n_run, plans, calls = int(g['n_run']), g[tag + '_coeffs'], []

    class Replayer(object):
        def solve(self, tpl, p, x, lam_g0=None, status0=None, n_threads=1, dw_state=None, **kw):
            calls.append((x[0].copy(), p[0].copy(), kw['warm_start'], lam_g0))
            out = x.copy()
            out[0, m.o_spl:m.o_spl + plans[0].size] = plans[len(calls) - 1].reshape(-1)
            return dict(x=out, lam_g=np.ones((1, tpl.n_con)), status=np.zeros(1, dtype=np.int32), iters=np.ones(1, dtype=np.int32))
    m = BatchP2P(problem, dict(P, p=g[tag + '_p'][:1].copy(), x0=g[tag + '_x0'][:1].copy()), ops=Replayer(), options=OPTS,
                 update_time=float(g['update_time']))
    m.record_signals(sample_time=float(g['sample_time']), max_updates=n_run + 2)
    if tag == 'plant':
        m.plant(sample_time=float(g['sample_time']), max_updates=n_run + 2)
    m.stop_at_arrival(stop_tol=-1.0)                                  # (a rule that never holds: the run ends where the replay ends it)
    m.solve_cold(bends=())
    m.mission(g['goal_new'][None, None, :])
    for k in range(1, n_run + 2):
        m.stop_tol = 1e9 if k == n_run else -1.0                      # (... which is here)
        m.rollout(1)
    assert len(calls) == n_run + 2 and m.mission_state()['arrivals'].tolist() == [[n_run - 1, -1]]
    assert [c[2] for c in calls] == [0] + [1] * (n_run - 1) + [0, 1] and calls[n_run][3] is None
    # where the simulated vehicle's state enters -- state0, and at the leg start the guess that begins at the stale state0 -- the
    # reference's odeint deviates from the exact integral of its own input: the bound the plant tests use, 10 x the recorded deviation
    tol_state = 1e-12 if tag == 'ideal' else 10 * float(ode['ode_dev_chained'])
    s0 = slice(m.o_state0, m.o_state0 + 2)
    for k, (x, p, _, _) in enumerate(calls):
        rest = np.ones(tpl.n_par, dtype=bool)
        rest[s0] = False
        assert np.abs(p[rest] - g[tag + '_p'][k][rest]).max() <= 1e-12, (k, 'p')
        assert np.abs(p[s0] - g[tag + '_p'][k][s0]).max() <= tol_state, (k, 'state0')
        blk = np.zeros(tpl.n_var, dtype=bool)
        blk[m.o_spl:m.o_spl + plans[0].size] = k == n_run
        assert np.abs(x[~blk] - g[tag + '_x0'][k][~blk]).max() <= 1e-12, (k, 'x0')
        assert np.abs(x[blk] - g[tag + '_x0'][k][blk]).max(initial=0.0) <= tol_state, (k, 'guess')
    assert (calls[n_run][1][m.o_input0:m.o_input0 + 2] == 0.0).all() and calls[n_run][1][m.o_t] == 0.0
    sig = m.signals()
    n_col = g[tag + '_state'].shape[1]
    assert sig['count'].tolist() == [n_col]
    assert np.abs(sig['state'][0][:, :n_col] - g[tag + '_state']).max() <= tol_state
    assert np.abs(sig['input'][0][:, :n_col] - g[tag + '_input']).max() <= 1e-12


def test_what_a_mission_refuses(cfg2_small):
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = workloads.holonomic_p2p(4)
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    goals = np.zeros((4, 2, 2))
    with pytest.raises(RuntimeError, match='stop_at_arrival'):
        m.mission(goals)
    with pytest.raises(RuntimeError, match='mission'):
        m.mission_state()
    with pytest.raises(NotImplementedError, match='device launch'):
        m.rollout(1)                                                  # without a mission a host batch still has no rollout
    m.stop_at_arrival(stop_tol=STOP_TOL)
    for bad in (np.zeros((4, 2, 3)), np.zeros((3, 2, 2)), np.zeros((4, 0, 2)), np.zeros((4, 2)), np.full((4, 2, 2), np.nan)):
        with pytest.raises(ValueError, match='goals'):
            m.mission(bad)
    for bad in (np.array([0, 1, 2, 3]), np.array([0, 1, -1, 2]), np.array([0, 1, 2]), np.array([0., 1., 2., 1.])):
        with pytest.raises(ValueError, match='n_goals'):
            m.mission(goals, bad)
    x0 = np.array(P['x0'], dtype=float)
    x0[2, 0 if m.o_spl > 0 else m.o_spl + m.n_spl * m.L] += 1.0
    odd = BatchP2P(problem, dict(P, x0=x0), ops=port_binding, options=OPTS)
    odd.stop_at_arrival(stop_tol=STOP_TOL)
    with pytest.raises(ValueError, match='first guess'):
        odd.mission(goals)
    m.obstacle_script(events=dict(time=np.full((4, 1), 0.55), obstacle=np.zeros((4, 1), dtype=int), kind=np.ones((4, 1), dtype=int),
                                  value=np.full((4, 1, 2), 0.1)))
    with pytest.raises(NotImplementedError, match='obstacle script'):
        m.mission(goals)
    m.obstacle_script(on=False)
    m.mission(goals, np.array([0, 1, 2, 2]))
    assert m.mission_state()['arrivals'].shape == (4, 3)
    with pytest.raises(RuntimeError, match='rollout\\(1\\)'):
        m.step()
    with pytest.raises(NotImplementedError, match='mission'):
        m.obstacle_script(events=dict(time=np.full((4, 1), 0.55), obstacle=np.zeros((4, 1), dtype=int), kind=np.ones((4, 1), dtype=int),
                                      value=np.full((4, 1, 2), 0.1)))
    m.time = 0.05
    with pytest.raises(ValueError, match='update grid'):
        m.mission(goals)
    m.time = 0.0
    m.stop_at_arrival(on=False)                                       # the rule goes, and the mission with it
    assert m._ms is None and m.under_way is None
    m.solve_cold(bends=())
    m.step()
    pool = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    pool.stop_at_arrival(stop_tol=STOP_TOL)
    pool.pool = object()
    with pytest.raises(NotImplementedError, match='host pool'):
        pool.mission(goals)
    quad_problem, quad_P = workloads.quadrotor_p2p(2)
    quad = BatchP2P(quad_problem, quad_P, ops=port_binding, options=OPTS)
    quad.plant(model='quadrotor')
    quad.stop_at_arrival(stop_tol=1e-2)
    with pytest.raises(NotImplementedError):
        quad.mission(np.zeros((2, 1, 2)))
