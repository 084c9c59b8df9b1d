"""Obstacle scripts (`BatchP2P.obstacle_script`) on the host loop, the numpy statement `splines.advance_obstacles_scripted`, and the
C-ABI surface of the device version: the reference's obstacle trajectories `simulation={'trajectories': {...}}`
(`environment/obstacle.py:172-264`).  Fixture: tests/golden/obstacle_script.npz (generator: tests/golden/
generate_obstacle_script_golden.py, the reference's own `Obstacle.simulate`)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OPTS = dict(tol=1e-3, max_iter=300)


class _Script(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('time', 'what', 'value', 'what_host', 'obst')] + [(n, ctypes.c_int32) for n in ('n_ev', 'n_obst')]


def fixture_script():
    """(script, obst, p0, g): the fixture's events as one agent's script over a parameter row that holds nothing but the 4
    obstacles -- obstacle q: x at 6 q, v at 6 q + 2, a at 6 q + 4."""
    g = np.load(os.path.join(GOLD, 'obstacle_script.npz'))
    E = len(g['ev_time'])
    value = np.zeros((1, E, 3))
    value[0, :, :2] = g['ev_value']
    script = dict(time=g['ev_time'][None, :].copy(), what=(3 * g['ev_obstacle'] + g['ev_kind'])[None, :].astype(np.int32), value=value)
    obst = [(6 * q, 6 * q + 2, 6 * q + 4, 2) for q in range(4)]
    return script, obst, state_row(g, 0), g


def state_row(g, k):
    return np.stack([g['position'][k], g['velocity'][k], g['acceleration'][k]], axis=1).reshape(1, -1).copy()      # [1, 4 * 3 * 2]


def test_abi_surface_of_the_obstacle_script():
    """The header declares OMGX_HAS_OBSTACLE_SCRIPT, the struct and the two entry points, the library exports them, the ABI version is
    still 9; every refusal names the entry and the field, ahead of `null handle` (no device needed)."""
    from omgtools.backend import LIB_PATH, CObstacleScript
    header = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    assert re.search(r'#define\s+OMGX_HAS_OBSTACLE_SCRIPT\s+1\b', header) and re.search(r'#define\s+OMGX_VERSION\s+9\b', header)
    assert 'typedef struct omgx_obstacle_script' in header
    lib = ctypes.CDLL(LIB_PATH)
    lib.omgx_version.restype = ctypes.c_int
    lib.omgx_last_error.restype = ctypes.c_char_p
    assert lib.omgx_version() == 9
    for name in ('omgx_batch_obstacles_advance', 'omgx_batch_set_obstacle_script'):
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
        assert hasattr(lib, name), name
    assert [f[0] for f in CObstacleScript._fields_] == [f[0] for f in _Script._fields_] and ctypes.sizeof(CObstacleScript) == ctypes.sizeof(_Script) == 48
    V, D = ctypes.c_void_p, ctypes.c_double
    lib.omgx_batch_obstacles_advance.argtypes = [V, V, ctypes.POINTER(_Script), D, D]
    lib.omgx_batch_set_obstacle_script.argtypes = [V, ctypes.POINTER(_Script), V, ctypes.c_int32]
    dummy = np.zeros(8)                                   # (never dereferenced: the checks come first)
    t_abs = np.array([0.0, 0.1, 0.2])

    def spec(n_dim=2, **kw):
        obst = np.array([[0, 2, 4, n_dim], [6, 8, 10, 2]], dtype=np.int32)
        f = dict(time=dummy.ctypes.data, what=dummy.ctypes.data, value=dummy.ctypes.data, what_host=None, obst=obst.ctypes.data, n_ev=4, n_obst=2)
        f.update(kw)
        sp = _Script(**f)
        sp._keep = obst
        return sp
    for kw, word in [(dict(n_ev=0), b'n_ev'), (dict(n_ev=33), b'n_ev'), (dict(n_obst=0), b'n_obst'), (dict(n_obst=9), b'n_obst'),
                     (dict(n_dim=4), b'n_dim'), (dict(n_dim=0), b'n_dim'), (dict(time=None), b'null time'), (dict(obst=None), b'obst')]:
        sp = spec(**kw)
        assert lib.omgx_batch_obstacles_advance(None, dummy.ctypes.data, ctypes.byref(sp), 0.0, 0.1) == -1, kw
        assert lib.omgx_last_error().startswith(b'obstacles_advance:') and word in lib.omgx_last_error(), (kw, lib.omgx_last_error())
        assert lib.omgx_batch_set_obstacle_script(None, ctypes.byref(sp), t_abs.ctypes.data, 3) == -1, kw
        assert lib.omgx_last_error().startswith(b'set_obstacle_script:') and word in lib.omgx_last_error(), (kw, lib.omgx_last_error())
    good = spec()
    assert lib.omgx_batch_obstacles_advance(None, None, ctypes.byref(good), 0.0, 0.1) == -1 and b'obstacles_advance: null p' in lib.omgx_last_error()
    assert lib.omgx_batch_obstacles_advance(None, dummy.ctypes.data, ctypes.byref(good), 0.0, 0.0) == -1
    assert lib.omgx_last_error().startswith(b'obstacles_advance:') and b'dt' in lib.omgx_last_error()
    assert lib.omgx_batch_set_obstacle_script(None, ctypes.byref(good), None, 3) == -1 and b'set_obstacle_script: null t_abs' in lib.omgx_last_error()
    assert lib.omgx_batch_set_obstacle_script(None, ctypes.byref(good), t_abs.ctypes.data, 1) == -1
    assert lib.omgx_last_error().startswith(b'set_obstacle_script:') and b'n_t' in lib.omgx_last_error()
    assert lib.omgx_batch_obstacles_advance(None, dummy.ctypes.data, ctypes.byref(good), 0.0, 0.1) == -1 and b'null handle' in lib.omgx_last_error()
    assert lib.omgx_batch_set_obstacle_script(None, ctypes.byref(good), t_abs.ctypes.data, 3) == -1 and b'null handle' in lib.omgx_last_error()
    assert lib.omgx_batch_set_obstacle_script(None, None, None, 0) == -1 and b'null handle' in lib.omgx_last_error()


@pytest.mark.parametrize('chained', [False, True])
def test_numpy_statement_meets_the_reference(chained):
    """The reference's own `Obstacle.simulate` over 60 updates of 0.1 s (on-grid, off-grid and off-sample jumps of all three kinds, two
    kinds at one time, two events in one update, an obstacle at rest until its first event): position, velocity and acceleration at
    every update boundary within 10 x the deviation of the reference's odeint from the exact motion (recorded in the fixture; an
    event applied one sample late deviates by `late_dev`, ten times that or more).  Restarted from the reference's state per update,
    and chained over all 60 with the loop's own clock t += 0.1."""
    from omgtools.splines import advance_obstacles_scripted
    script, obst, p, g = fixture_script()
    bound = 10 * float(g['ode_dev'])
    assert float(g['late_dev']) >= bound
    dt, t, worst = float(g['update_time']), 0.0, np.zeros(3)
    for k in range(60):
        if not chained:
            p = state_row(g, k)
        advance_obstacles_scripted(p, obst, script, t, t + dt, dt=dt)
        t = t + dt
        err = np.abs(p - state_row(g, k + 1)).reshape(4, 3, 2).max(axis=(0, 2))
        worst = np.maximum(worst, err)
    print('%s: position %.2e velocity %.2e acceleration %.2e (bound %.2e)' % ('chained' if chained else 'per update', worst[0], worst[1], worst[2], bound))
    assert worst.max() <= bound


def test_a_script_that_never_fires_is_the_plain_motion_bit_for_bit():
    from omgtools.splines import advance_obstacles, advance_obstacles_scripted
    rng = np.random.default_rng(5)
    obst = [(0, 3, 6, 3), (9, 11, 13, 2), (15, 16, 17, 1)]
    p = rng.normal(size=(6, 20))
    q = p.copy()
    script = dict(time=np.tile([7.0, 8.5, np.inf], (6, 1)), what=np.tile([1, 4, 0], (6, 1)).astype(np.int32), value=rng.normal(size=(6, 3, 3)))
    t = 0.0
    for k in range(15):
        advance_obstacles(p, obst, 0.1)
        advance_obstacles_scripted(q, obst, script, t, t + 0.1, dt=0.1)
        t = t + 0.1
        assert np.array_equal(p, q), k
    assert np.array_equal(p[:, 18:], q[:, 18:]) and p[0, 19] == q[0, 19]      # (and nothing but the obstacles' entries moved)


def test_an_event_on_the_boundary_and_one_half_a_nanosecond_later_give_the_same_bits():
    from omgtools.splines import advance_obstacles, advance_obstacles_scripted
    rng = np.random.default_rng(6)
    obst = [(0, 2, 4, 2), (6, 8, 10, 2)]
    p0 = rng.normal(size=(3, 12))
    t_prev = 0.1 + 0.1 + 0.1 + 0.1          # (the loop's clock: 0.4 as it accumulates)
    t_now = t_prev + 0.1
    out = []
    for t_e in (t_now, t_now + 5e-10, t_now - 5e-10):
        script = dict(time=np.full((3, 1), t_e), what=np.full((3, 1), 4, dtype=np.int32), value=np.tile([[[0.25, -0.5, 0.0]]], (3, 1, 1)))
        p = p0.copy()
        advance_obstacles_scripted(p, obst, script, t_prev, t_now, dt=0.1)
        out.append(p)
        # ... and belongs to this update, not to the next
        again = p.copy()
        advance_obstacles_scripted(again, obst, script, t_now, t_now + 0.1, dt=0.1)
        plain = p.copy()
        advance_obstacles(plain, obst, 0.1)
        assert np.array_equal(again, plain)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    # up to the jump the plain motion's bits
    plain = p0.copy()
    advance_obstacles(plain, obst, 0.1)
    plain[:, 8:10] += [0.25, -0.5]
    assert np.array_equal(out[0], plain)


def _host_loop(problem, P, events, n_steps=12):
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    if events is not None:
        m.obstacle_script(events)
    m.solve_cold()
    hist = []
    for k in range(n_steps):
        m.step()
        hist.append(dict(x=m.x.copy(), p=m.p.copy(), status=m.status.copy(), time=m.time))
    return m, hist


def test_host_loop_with_a_script(cfg2_small):
    """8 agents of config 2, cold solve and 12 steps across the knot crossing of the update 0.9 -> 1.0; the (resting) obstacle 1 of
    every agent is set moving at 0.35 (off the update grid), turned inside the crossing update (0.95) and pushed once more on the
    grid (1.1).  p's obstacle entries follow the numpy statement; every solve still succeeds; the plans are the unscripted loop's
    bit for bit up to the update that holds the first event and differ from it afterwards."""
    from omgtools.splines import advance_obstacles_scripted
    problem, P = cfg2_small
    B = 8
    events = dict(time=np.tile([0.35, 0.95, 1.1], (B, 1)), obstacle=np.full((B, 3), 1), kind=np.tile([1, 1, 0], (B, 1)),
                  value=np.tile([[0.05, -0.03], [-0.02, 0.04], [0.01, 0.01]], (B, 1, 1)) * (1.0 + 0.1 * np.arange(B))[:, None, None])
    m, hist = _host_loop(problem, P, events)
    plain, hist0 = _host_loop(problem, P, None)
    assert len(plain.obst) == 0 and len(m.obst) == 1      # (the resting obstacle joined the moving ones)
    ox, ov, oa, nd = m.obst[0]
    assert np.any(P['p'][:, ox:ox + nd] != 0.) and not np.any(P['p'][:, ov:ov + nd]) and not np.any(P['p'][:, oa:oa + nd])
    # the numpy statement, on a row of its own
    ref, t = np.array(P['p'], dtype=float), 0.0
    crossed_at = None
    for k, h in enumerate(hist):
        advance_obstacles_scripted(ref, m.obst, m._sc, t, t + 0.1, dt=0.1)
        t = t + 0.1
        assert h['time'] == t
        for o in (ox, ov, oa):
            assert np.array_equal(h['p'][:, o:o + nd], ref[:, o:o + nd]), (k, o)
        assert (h['status'] == 0).all(), (k, h['status'])
        same = np.array_equal(h['x'], hist0[k]['x'])
        assert same == (k < 3), (k, same)                  # (0.35 lies in the fourth update, 0.3 -> 0.4)
    # closed form of the whole script for agent 0: v = 0 until 0.35
    v1, v2, dx = events['value'][0, 0], events['value'][0, 1], events['value'][0, 2]
    end = P['p'][0, ox:ox + nd] + v1 * (t - 0.35) + v2 * (t - 0.95) + dx
    assert np.abs(hist[-1]['p'][0, ox:ox + nd] - end).max() <= 1e-13
    assert np.abs(hist[-1]['p'][0, ov:ov + nd] - (v1 + v2)).max() <= 1e-15


def test_obstacle_script_refusals(cfg2_small):
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = workloads.holonomic_p2p(2)                 # from its bundle: no obstacle simulation
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    with pytest.raises(ValueError) as e:
        m.obstacle_script()
    assert 'events' in str(e.value)
    ev = dict(time=np.full((2, 1), 0.5), obstacle=np.zeros((2, 1), dtype=int), kind=np.ones((2, 1), dtype=int), value=np.ones((2, 1, 2)))
    m.obstacle_script(ev)                                   # (with events a bundle's problem takes a script)
    assert m._sc is not None and len(m.obst) == 1
    m.obstacle_script(on=False)
    assert m._sc is None
    problem, P = cfg2_small
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    with pytest.raises(ValueError):                        # (front end, but no obstacle has a trajectory)
        m.obstacle_script()
    ev = dict(time=np.full((8, 1), 0.5), obstacle=np.zeros((8, 1), dtype=int), kind=np.ones((8, 1), dtype=int), value=np.ones((8, 1, 2)))
    m.time = 0.5
    with pytest.raises(ValueError) as e:                   # an event at the current time has passed
        m.obstacle_script(ev)
    assert 'current time' in str(e.value)
    m.time = 0.0
    with pytest.raises(ValueError) as e:                   # the reference folds an event at 0 into the initial state
        m.obstacle_script(dict(ev, time=np.zeros((8, 1))))
    assert 'current time' in str(e.value)
    many = dict(time=np.tile(0.1 + 0.01 * np.arange(33), (8, 1)), obstacle=np.zeros((8, 33), dtype=int), kind=np.ones((8, 33), dtype=int),
                value=np.ones((8, 33, 2)))
    with pytest.raises(ValueError) as e:
        m.obstacle_script(many)
    assert '33' in str(e.value)
    m.obstacle_script(dict((k, v[:, :32]) for k, v in many.items()))      # (32 are taken)
    assert m._sc['time'].shape == (8, 32)
    with pytest.raises(ValueError):
        m.obstacle_script(dict(ev, obstacle=np.full((8, 1), 3)))           # (config 2 has obstacles 0 .. 2)
    assert m._sc['time'].shape == (8, 32)                                  # (a refused call leaves the script as it was)
    m.pool = object()
    with pytest.raises(NotImplementedError):
        m.obstacle_script(ev)


def test_the_front_end_hands_its_script_over():
    """A problem built with `simulation={'trajectories': ...}` -- the obstacle of the reference's `examples/
    p2p_holonomic_multiproblem.py:35-38` -- gives its script with `events=None`: sorted, the event at time 0 left out (it is the
    initial state), the same for every agent; the resting obstacle joins the moving ones, the one without a script does not."""
    import omgtools.backend as be
    from omgtools import workloads as wl
    from omgtools.batch import BatchP2P
    from omgtools.environment import Environment, Obstacle
    from omgtools.problems import Point2point
    from omgtools.shapes import Circle, Square
    from omgtools.vehicles import Holonomic
    from oracle import port_binding
    vehicle = Holonomic()
    vehicle.define_knots(knot_intervals=11)
    vehicle.set_initial_conditions([-1.5, -1.5])
    vehicle.set_terminal_conditions([1.5, 1.5])
    environment = Environment(room={'shape': Square(5.)})
    environment.add_obstacle(Obstacle({'position': [0., 0.]}, shape=Circle(0.3)))
    traj = {'velocity': {'time': [4., 3.], 'values': [[0., 0.15], [-0.15, 0.0]]},
            'acceleration': {'time': [0., 3.], 'values': [[0.5, 0.5], [0.0, 0.01]]}}
    environment.add_obstacle(Obstacle({'position': [1.5, 0.5]}, shape=Circle(0.3), simulation={'trajectories': traj}))
    saved = be.create_nlp
    be.create_nlp = lambda tpl, opt, name='': (None, 0.)     # template only, no device
    try:
        problem = Point2point(vehicle, environment, options={'horizon_time': 10., 'verbose': 0})
        problem.init()
    finally:
        be.create_nlp = saved
    tpl = problem.father.template
    P = wl.fill_holonomic_p2p(tpl, vehicle.label, problem.label, [o.label for o in environment.obstacles], len(vehicle.basis), 3, 11, 10.)
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    n_before = len(m.obst)
    m.obstacle_script()
    assert len(m.obst) == n_before + 1
    slot = len(m.obst) - 1
    ox = tpl.entry_range(environment.obstacles[1].label, 'x', 'par')[0]
    assert m.obst[slot][0] == ox and m.obst[slot][3] == 2
    sc = m._sc
    assert np.array_equal(sc['time'], np.tile([3., 3., 4.], (3, 1)))
    assert np.array_equal(sc['what'], np.tile([3 * slot + 1, 3 * slot + 2, 3 * slot + 1], (3, 1)))
    assert np.array_equal(sc['value'], np.tile([[-0.15, 0., 0.], [0., 0.01, 0.], [0., 0.15, 0.]], (3, 1, 1)))


def test_random_obstacle_script_is_seeded_and_shaped():
    from omgtools.batch import random_obstacle_script
    a = random_obstacle_script(8, 3, 2, 6, 1.5, 0.05, seed=2)
    assert a['time'].shape == (8, 6) and a['obstacle'].shape == (8, 6) and a['kind'].shape == (8, 6) and a['value'].shape == (8, 6, 2)
    assert (np.diff(a['time'], axis=1) >= 0).all() and a['time'].min() > 0 and a['time'].max() <= 1.5 + 1e-12
    assert a['obstacle'].min() >= 0 and a['obstacle'].max() <= 2 and a['kind'].min() >= 0 and a['kind'].max() <= 2
    on_grid = np.abs(a['time'] / 0.1 - np.round(a['time'] / 0.1)) < 1e-9
    assert on_grid.any() and not on_grid.all()
    b = random_obstacle_script(8, 3, 2, 6, 1.5, 0.05, seed=2)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a['time'], random_obstacle_script(8, 3, 2, 6, 1.5, 0.05, seed=3)['time'])
