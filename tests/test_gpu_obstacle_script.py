"""Obstacle scripts on the device (`omgx_batch_obstacles_advance`, `omgx_batch_set_obstacle_script`): the reference's obstacle
trajectories `simulation={'trajectories': ...}`.  One routine serves the stand-alone launch and the script instances of the rollout
kernel, so both must write THE SAME BITS as the numpy statement `splines.advance_obstacles_scripted`; they must meet the reference's
`Obstacle.simulate` (tests/golden/obstacle_script.npz); and a loop whose script never fires, or that has none, must not change."""
import numpy as np
import pytest

from test_obstacle_script_cpu import fixture_script, state_row

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)


def _drift(problem, P):
    tpl = problem.father.template
    rng = np.random.default_rng(5)
    for obs in problem.environment.obstacles:
        ov, oa = (tpl.entry_range(obs.label, nm, 'par') for nm in ('v', 'a'))
        P['p'][:, ov[0]:ov[1]] = rng.uniform(-0.03, 0.03, size=(len(P['p']), ov[1] - ov[0]))
        P['p'][:, oa[0]:oa[1]] = rng.uniform(-0.01, 0.01, size=(len(P['p']), oa[1] - oa[0]))


def _events(n, seed=3, t_max=1.2, n_obst=3, t_cross=0.95):
    """Six random events per agent over the 12 updates (on and off the update grid, all three kinds, all three obstacles), one of
    them moved into the knot-crossing update 0.9 -> 1.0.  (t_max, n_obst, t_cross: of another class than config 2.)"""
    from omgtools.batch import random_obstacle_script
    ev = random_obstacle_script(n, n_obst, 2, 6, t_max, 0.03, seed=seed)
    ev['time'][:, 3] = t_cross
    return ev


def _mk(n, events=None, drift=False, cold=True, plant=False, cls=None, build=None, max_updates=16, **kw):
    """build(n) -> (problem, P): another class than config 2 (tests/test_gpu_workspace_cells.py)."""
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P, input_disturbance
    problem, P = (build or workloads.holonomic_p2p)(n)
    if drift:
        _drift(problem, P)
    m = (cls or BatchP2P)(problem, P, device=torch.device('cuda', 0), options=OPTS, **kw)
    if plant:
        m.plant(sample_time=0.01, max_updates=max_updates,
                disturbance=input_disturbance(n, 2, max_updates, 10, 1001, fc=0.1, stdev=0.02, seed=7))
        m.record_signals(sample_time=0.01, max_updates=max_updates)
    if events is not None:
        m.obstacle_script(events)
    if cold:
        m.solve_cold(bends=())
    return m


def _equal(a, b, plant=False):
    import torch
    extra = []
    if plant:
        sa, sb, pa, pb = a.signals(), b.signals(), a.plant_state(), b.plant_state()
        extra = [(sa[k], sb[k], k) for k in ('splines', 'count', 'overflow')] + [(pa[k], pb[k], k) for k in pa]
    torch.cuda.synchronize()
    for name in ('x', 'lam', 'p', 'status', 'iters'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for u, v, name in extra:
        assert torch.equal(u, v), name


def _close(*ms):
    for m in ms:
        if hasattr(m, 'close'):
            m.close()
        else:
            m.solver.close()


def test_stand_alone_kernel_equals_the_numpy_statement_and_meets_the_reference():
    """No solve involved.  (a) The fixture's scripts through `omgx_batch_obstacles_advance`, chained over the 60 updates and restarted
    from the reference's state per update: the bits of `advance_obstacles_scripted`, and the reference's states within 10 x its own
    odeint deviation.  (b) Random scripts, 8 agents x 3 obstacles x 6 events over 15 updates, on the obstacle entries of the
    config-2 parameter rows: the same bits as the numpy statement after every update."""
    import torch
    from omgtools.splines import advance_obstacles_scripted
    from omgtools.batch import random_obstacle_script
    script, obst, p0, g = fixture_script()
    bound = 10 * float(g['ode_dev'])
    m = _mk(1, cold=False)
    n_par = m.p.shape[1]
    assert n_par >= p0.shape[1]
    dev = m.p.device
    args = dict(time=torch.as_tensor(script['time'], device=dev), what=torch.as_tensor(script['what'], device=dev),
                value=torch.as_tensor(script['value'], device=dev), obstacles=obst, what_host=script['what'])
    for chained in (False, True):
        p, t, worst = torch.zeros((1, n_par), dtype=torch.float64, device=dev), 0.0, 0.0
        host = np.zeros((1, n_par))
        p[:, :p0.shape[1]] = torch.as_tensor(p0, device=dev)
        host[:, :p0.shape[1]] = p0
        for k in range(60):
            if not chained:
                host[:, :p0.shape[1]] = state_row(g, k)
                p.copy_(torch.as_tensor(host, device=dev))
            m.solver.obstacles_advance(p, args, t, 0.1)
            advance_obstacles_scripted(host, obst, script, t, t + 0.1, dt=0.1)
            t = t + 0.1
            got = p.cpu().numpy()
            assert np.array_equal(got, host), (chained, k)
            worst = max(worst, float(np.abs(got[:, :p0.shape[1]] - state_row(g, k + 1)).max()))
        print('%s: against the reference %.2e (bound %.2e)' % ('chained' if chained else 'per update', worst, bound))
        assert worst <= bound
    _close(m)
    # (b)
    m = _mk(8, events=random_obstacle_script(8, 3, 2, 6, 1.5, 0.05, seed=11), drift=True, cold=False)
    assert len(m.obst) == 3
    host, t = m.p.cpu().numpy().copy(), 0.0
    sc = dict(time=m._sc['time'].cpu().numpy(), what=m._sc['what'].cpu().numpy(), value=m._sc['value'].cpu().numpy())
    fired = 0
    for k in range(15):
        before = host.copy()
        m._advance_obstacles(t, t + 0.1)
        advance_obstacles_scripted(host, m.obst, sc, t, t + 0.1, dt=0.1)
        fired += int(((sc['time'] > t + 1e-9) & (sc['time'] <= t + 0.1 + 1e-9)).sum())
        t = t + 0.1
        assert np.array_equal(m.p.cpu().numpy(), host), k
        assert not np.array_equal(before, host)
    assert fired == 8 * 6
    _close(m)


@pytest.mark.parametrize('n,plant', [(8, False), (520, False), (8, True)])
def test_rollout_equals_the_stepwise_loop_bit_for_bit(n, plant):
    """`rollout(12)` against 12 `step()` calls with a script on (drifting obstacles, an event inside the knot-crossing update), for 8
    agents, for more agents (520) than the 512 resident workgroups, so that the slot hand-out runs in the script instance, and with
    the plant and the log on (the plant's script instance)."""
    ev = _events(n)
    a, b = (_mk(n, events=ev, drift=True, plant=plant) for _ in range(2))
    crossings = a.rollout(12)
    for _ in range(12):
        b.step()
    _equal(a, b, plant)
    assert crossings == 1
    # the script acted: the obstacle entries are not those of the plain motion
    c = _mk(n, drift=True, cold=False)
    for _ in range(12):
        c._advance_obstacles(0.0, 0.1)
    ox, _, _, nd = a.obst[0]
    assert not np.array_equal(c.p[:, ox:ox + nd].cpu().numpy(), a.p[:, ox:ox + nd].cpu().numpy())
    _close(a, b, c)


def test_streamed_sub_batches_equal_one_handle():
    """`StreamedP2P(n_streams=3)` against one handle, 48 agents, the cold solve and 12 steps with per-agent scripts: every sub-batch
    gets its rows -- the same bits."""
    from omgtools.batch import StreamedP2P
    ev = _events(48)
    a = _mk(48, events=ev, drift=True, cls=StreamedP2P, n_streams=3)
    b = _mk(48, events=ev, drift=True)
    for _ in range(12):
        a.step(); b.step()
    _equal(a, b)
    assert a.parts[1]._sc['time'].shape[0] == a.bounds[1][1] - a.bounds[1][0]
    _close(a, b)


def test_a_script_that_never_fires_is_the_plain_loop_bit_for_bit():
    """A script whose events lie beyond the run against no script at all, per step and as a rollout; the plain loop still launches the
    solve instance it launched before (`omgx_batch_last_instance`), the scripted one the same."""
    n = 16
    ev = dict(time=np.full((n, 2), 50.0), obstacle=np.tile([0, 2], (n, 1)), kind=np.tile([1, 0], (n, 1)), value=np.ones((n, 2, 2)))
    a, b = _mk(n, events=ev, drift=True), _mk(n, drift=True)
    assert a._sc is not None and b._sc is None and a.obst == b.obst
    for k in range(6):
        a.step(); b.step()
        _equal(a, b)
    assert a.solver.workspace()['last_instance'] == b.solver.workspace()['last_instance']
    a.rollout(6); b.rollout(6)
    _equal(a, b)
    _close(a, b)


def test_on_false_restores_the_plain_statements():
    n = 16
    ev = _events(n)
    a, b = _mk(n, events=ev, drift=True), _mk(n, drift=True)
    a.obstacle_script(on=False)
    assert a._sc is None
    for k in range(3):
        a.step(); b.step()
    a.rollout(3); b.rollout(3)
    _equal(a, b)
    # ... and after a rollout that HAD the script registered with the handle: the obstacle entries move by the plain statements
    from omgtools.splines import advance_obstacles
    c = _mk(n, events=ev, drift=True)
    c.rollout(2)
    c.obstacle_script(on=False)
    host = c.p.cpu().numpy().copy()
    c.rollout(3)
    for _ in range(3):
        advance_obstacles(host, c.obst, 0.1)
    got = c.p.cpu().numpy()
    for ox, ov, oa, nd in c.obst:
        for o in (ox, ov, oa):
            assert np.array_equal(got[:, o:o + nd], host[:, o:o + nd]), o
    _close(a, b, c)
