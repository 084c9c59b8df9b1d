"""The plant in the loop (`BatchP2P.plant`) on the host loop, and the C-ABI surface of the device version: the simulated vehicle of the
reference's default options `ideal_prediction=False, ideal_update=False` with an input disturbance (`Vehicle.simulate` / `Vehicle.predict`,
`vehicles/vehicle.py:326-337, 370-390`).  Fixture: tests/golden/plant_holonomic.npz (generator: tests/golden/generate_plant_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OPTS = dict(tol=1e-3, max_iter=300)


def plan_inputs(knots, coeffs, t_rel, T, sample_time, n_samp, shift=0):
    """Nominal inputs of a plan by scipy's B-splines (no code shared with the package): d/dt spline at (t_rel + i sample_time) / T,
    i = shift .. shift + n_samp; coeffs [..., L] -> [..., n_samp + 1]."""
    from scipy.interpolate import BSpline
    u = (t_rel + (shift + np.arange(n_samp + 1)) * sample_time) / T
    return np.moveaxis(BSpline(knots, np.moveaxis(coeffs, -1, 0), 3).derivative()(u), 0, -1) / T


def plan_positions(knots, coeffs, t_rel, T):
    from scipy.interpolate import BSpline
    return BSpline(knots, np.moveaxis(coeffs, -1, 0), 3)(np.asarray(t_rel) / T)


def trapezoid(s0, a, h):
    return s0[..., None] + h * np.cumsum((a[..., :-1] + a[..., 1:]) / 2.0, axis=-1)


def replay_fixture(rep, g, p, predict, simulate, chained, get, put):
    """The fixture's plans and disturbance through an executor's simulate / predict (`predict(tau, t_rel)`, `simulate()`), x and
    p[o_t] set per update as tests/test_signals_cpu.py does; unchained: the plant's state is set to the fixture's start-of-update
    state ahead of every simulate.  get / put: read / write an array of the executor.  Returns the predicted state0 / input0."""
    n_upd, T, upd = len(g['t_rel']), float(g['horizon_time']), float(g['update_time'])
    state0, input0 = np.full((n_upd, 4, 2), np.nan), np.full((n_upd, 4, 2), np.nan)
    for k in range(n_upd):
        if k:
            predict((float(g['t_rel'][k - 1]) + upd) / T, float(g['t_rel'][k]))      # (reads the plan and the t of update k - 1)
            pk = get(rep.p)
            state0[k], input0[k] = pk[:, rep.o_state0:rep.o_state0 + 2], pk[:, rep.o_input0:rep.o_input0 + 2]
        x, pp = get(rep.x).copy(), get(rep.p).copy()
        x[:, rep.o_spl:rep.o_spl + 2 * rep.L] = g['coeffs'][k].reshape(4, -1)
        pp[:, rep.o_t] = g['t_rel'][k]
        put(rep.x, x), put(rep.p, pp)
        if k and not chained:
            put(rep.plant_state()['state'], p['state_start'][k])
        simulate()
    return state0, input0


def check_against_fixture(g, p, sig, state0, input0, chained):
    """The three bounds of the issue: input / dinput columns within 1e-10 (pure spline evaluation, the bound of the log test); state
    columns and predicted state0 within 10 x the deviation of the reference's own odeint from the exact integral (recorded in the
    fixture; an off-by-one choice of samples would show a deviation of at least `sample_shift_dev`, ten times that or more);
    against the closed-form cumulative trapezoid written here, 1e-12 (sums of at most 121 terms of order one in fp64)."""
    n_upd, n_samp, st, T = len(g['t_rel']), 10, float(g['sample_time']), float(g['horizon_time'])
    n_col = 1 + n_samp * n_upd
    assert (sig['count'] == n_col).all() and not sig['overflow'].any()
    bound = 10 * float(p['ode_dev_chained' if chained else 'ode_dev'])
    assert float(p['sample_shift_dev']) >= 10 * float(p['ode_dev'])
    err_in = np.abs(sig['input'] - p['input']).max()
    err_din = np.abs(sig['dinput'] - p['dinput']).max()
    err_st = np.abs(sig['state'] - p['state']).max()
    err_s0 = np.abs(state0[1:] - p['state0'][1:]).max()
    err_i0 = np.abs(input0[1:] - p['input0'][1:]).max()
    # closed form: per update, from the state the run itself started the update with
    worst = 0.0
    for k in range(n_upd):
        u = plan_inputs(g['knots'], g['coeffs'][k], float(g['t_rel'][k]), T, st, n_samp)                # [4, 2, n_samp + 1]
        a = u + p['dist'][:, :, k, :]
        start = sig['state'][:, :, k * n_samp] if chained or k == 0 else p['state_start'][k]
        cols = slice(k * n_samp + 1, (k + 1) * n_samp + 1)
        worst = max(worst, np.abs(trapezoid(start, a, st) - sig['state'][:, :, cols]).max(), np.abs(a[..., 1:] - sig['input'][:, :, cols]).max())
        if k:
            prev = sig['state'][:, :, (k - 1) * n_samp] if chained or k == 1 else p['state_start'][k - 1]
            u_prev = plan_inputs(g['knots'], g['coeffs'][k - 1], float(g['t_rel'][k - 1]), T, st, n_samp)
            worst = max(worst, np.abs(trapezoid(prev, u_prev, st)[..., -1] - state0[k]).max())
    print('%s: input %.2e dinput %.2e state %.2e state0 %.2e input0 %.2e (bound %.2e), closed form %.2e'
          % ('chained' if chained else 'per update', err_in, err_din, err_st, err_s0, err_i0, bound, worst))
    assert err_in <= 1e-10 and err_din <= 1e-10 and err_i0 <= 1e-10
    assert err_st <= bound and err_s0 <= bound
    assert worst <= 1e-12


class _Plant(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('state', 'state_prev', 'input_last', 'dist', 'n_upd', 'overflow', 'under_way', 'knots')] + \
               [(n, ctypes.c_int32) for n in ('coeff_off', 'n_spl', 'degree', 'n_knots', 'n_samp', 'max_updates', 'p_t', 'p_state0', 'p_input0',
                                              'p_poseT')] + [(n, ctypes.c_double) for n in ('sample_time', 'inv_T', 'stop_tol')]


def test_abi_surface_of_the_plant():
    """The header declares OMGX_HAS_PLANT, the specification and the three entry points, the library exports them, the ABI version is
    still 9, and a null handle / an inconsistent specification is refused with OMGX_E_INVALID and a message (no device needed)."""
    from omgtools.backend import LIB_PATH, CPlantSpec
    header = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    assert re.search(r'#define\s+OMGX_HAS_PLANT\s+1\b', header) and re.search(r'#define\s+OMGX_VERSION\s+9\b', header)
    assert 'typedef struct omgx_plant_spec' in header
    lib = ctypes.CDLL(LIB_PATH)
    lib.omgx_version.restype = ctypes.c_int
    lib.omgx_last_error.restype = ctypes.c_char_p
    assert lib.omgx_version() == 9
    for name in ('omgx_batch_plant_simulate', 'omgx_batch_plant_predict', 'omgx_batch_set_plant'):
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
        assert hasattr(lib, name), name
    assert [f[0] for f in CPlantSpec._fields_] == [f[0] for f in _Plant._fields_] and ctypes.sizeof(CPlantSpec) == ctypes.sizeof(_Plant) == 128
    V = ctypes.c_void_p
    lib.omgx_batch_set_plant.argtypes = [V, ctypes.POINTER(_Plant), V]
    lib.omgx_batch_plant_simulate.argtypes = [V, V, V, ctypes.POINTER(_Plant), V]
    lib.omgx_batch_plant_predict.argtypes = [V, V, V, ctypes.c_double, ctypes.c_double, ctypes.POINTER(_Plant)]
    knots = np.r_[np.zeros(3), np.linspace(0., 1., 12), np.ones(3)]
    dummy = np.zeros(8)                                   # (never dereferenced: the checks come first)

    def spec(**kw):
        f = dict(state=dummy.ctypes.data, state_prev=dummy.ctypes.data, input_last=dummy.ctypes.data, dist=None, n_upd=dummy.ctypes.data,
                 overflow=None, under_way=None, knots=knots.ctypes.data, coeff_off=0, n_spl=2, degree=3, n_knots=len(knots), n_samp=10,
                 max_updates=12, p_t=0, p_state0=1, p_input0=3, p_poseT=5, sample_time=0.01, inv_T=0.1, stop_tol=1e-3)
        f.update(kw)
        return _Plant(**f)
    for kw, word in [(dict(n_knots=41), b'n_knots'), (dict(n_samp=0), b'n_samp'), (dict(state=None), b'null'), (dict(sample_time=0.0), b'positive')]:
        sp = spec(**kw)
        assert lib.omgx_batch_set_plant(None, ctypes.byref(sp), None) == -1, kw
        assert word in lib.omgx_last_error(), (kw, lib.omgx_last_error())
        assert lib.omgx_batch_plant_simulate(None, None, None, ctypes.byref(sp), None) == -1 and word in lib.omgx_last_error()
        assert lib.omgx_batch_plant_predict(None, None, None, 0.1, 0.1, ctypes.byref(sp)) == -1 and word in lib.omgx_last_error()
    good = spec()
    assert lib.omgx_batch_set_plant(None, ctypes.byref(good), None) == -1 and b'null handle' in lib.omgx_last_error()
    assert lib.omgx_batch_plant_simulate(None, None, None, ctypes.byref(good), None) == -1 and b'null handle' in lib.omgx_last_error()
    assert lib.omgx_batch_plant_predict(None, None, None, 0.1, 0.1, ctypes.byref(good)) == -1 and b'null handle' in lib.omgx_last_error()
    assert lib.omgx_batch_set_plant(None, None, None) == -1


@pytest.mark.parametrize('chained', [False, True])
def test_host_glue_equals_the_reference_plant(cfg2_small, chained):
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = cfg2_small
    g, p = np.load(os.path.join(GOLD, 'signals_holonomic.npz')), np.load(os.path.join(GOLD, 'plant_holonomic.npz'))
    agents = g['agents']
    rep = BatchP2P(problem, dict(P, p=P['p'][agents], x0=P['x0'][agents]), ops=port_binding, options=OPTS)
    assert np.array_equal(np.asarray(rep.basis.knots, dtype=float), g['knots']) and rep.T == float(g['horizon_time'])
    rep.plant(sample_time=float(g['sample_time']), max_updates=12, disturbance=p['dist'])
    rep.record_signals(sample_time=float(g['sample_time']), max_updates=12)

    def put(dst, src):
        dst[...] = src
    state0, input0 = replay_fixture(rep, g, p, rep._plant_predict, rep._plant_simulate, chained, np.asarray, put)
    st = rep.plant_state()
    assert (st['n_upd'] == 12).all() and not st['overflow'].any()
    check_against_fixture(g, p, rep.signals(), state0, input0, chained)


def _closed_loop(problem, P, disturbance):
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    m.plant(sample_time=0.01, max_updates=13, disturbance=disturbance)
    m.record_signals(sample_time=0.01, max_updates=13)
    m.solve_cold()
    hist = []
    for k in range(12):
        # x, t: the plan travelled last and the time it was solved at; prev: where the vehicle was one update ago; start: where it is
        st = m.plant_state()
        h = dict(x=m.x.copy(), t=m.p[:, m.o_t].copy(), prev=st['state_prev'].copy(), start=st['state'].copy())
        m.step()
        h.update(state0=m.p[:, m.o_state0:m.o_state0 + 2].copy(), status=m.status.copy(), x_new=m.x.copy(), t_new=m.p[:, m.o_t].copy(),
                 state=m.plant_state()['state'].copy())
        hist.append(h)
    return m, hist


SEED = 1


def test_closed_loop_on_the_host_loop(cfg2_small):
    """8 agents, cold solve and 12 steps with the plant in the loop.  (a) The state every solve starts from is the state the vehicle
    had one update ago plus the nominal trapezoid of the plan travelled since, recomputed here with scipy's B-splines: 1e-12.  (b) The
    disturbance really entered: the travelled state leaves the plan by more than 1e-4 m somewhere.  (c) Without a disturbance the
    travelled displacement follows the plans' within the error of the trapezoid rule: the planned velocity v is piecewise quadratic,
    the rule's error on one sample interval h is at most h^3 / 12 max|v''| (v'' = the plan's ddinput, the jerk), so over a time t at
    most h^2 / 12 max|ddinput| t; the issue's h^2 max|dinput| t is asserted too.  Condition of the whole test: at every update at
    most one of the 8 solves ends other than Solve_Succeeded (seed picked for it)."""
    from omgtools.batch import input_disturbance
    from scipy.interpolate import BSpline
    problem, P = cfg2_small
    dist = input_disturbance(8, 2, 13, 10, 1001, fc=0.1, stdev=0.02, seed=SEED)
    m, hist = _closed_loop(problem, P, dist)
    knots, T, st = np.asarray(m.basis.knots, dtype=float), m.T, 0.01
    lo, n = m.o_spl, 2 * m.L
    worst, gap = 0.0, 0.0
    for k, h in enumerate(hist):
        assert (h['status'] != 0).sum() <= 1, (k, h['status'])
        c = h['x'][:, lo:lo + n].reshape(8, 2, m.L)
        u = np.stack([plan_inputs(knots, c[b], float(h['t'][b]), T, st, 10) for b in range(8)])
        worst = max(worst, np.abs(h['prev'] + st * np.cumsum((u[..., :-1] + u[..., 1:]) / 2.0, axis=-1)[..., -1] - h['state0']).max())
        c_new = h['x_new'][:, lo:lo + n].reshape(8, 2, m.L)
        end = np.stack([plan_positions(knots, c_new[b], float(h['t_new'][b]) + 0.1, T) for b in range(8)])
        gap = max(gap, np.abs(h['state'] - end).max())
    print('state0 against state_prev + nominal trapezoid: %.2e; travelled state against the plan: %.2e' % (worst, gap))
    assert worst <= 1e-12
    assert gap > 1e-4
    assert (m.plant_state()['n_upd'] == 13).all() and (m.signals()['count'] == 131).all()
    # (c) no disturbance
    m, hist = _closed_loop(problem, P, None)
    drift, t, jerk, acc = np.zeros((8, 2)), 0.0, 0.0, 0.0
    for k, h in enumerate(hist):
        assert (h['status'] != 0).sum() <= 1, (k, h['status'])
        c_new = h['x_new'][:, lo:lo + n].reshape(8, 2, m.L)
        for b in range(8):
            spl = BSpline(knots, c_new[b].T, 3)
            uu = (float(h['t_new'][b]) + np.linspace(0., 0.1, 101)) / T
            drift[b] += (h['state'][b] - h['start'][b]) - (spl(uu[-1]) - spl(uu[0]))
            acc, jerk = max(acc, np.abs(spl.derivative(2)(uu)).max() / T ** 2), max(jerk, np.abs(spl.derivative(3)(uu[:-1] + 1e-9)).max() / T ** 3)
        t += 0.1
        assert np.abs(drift).max() <= st ** 2 / 12 * jerk * t + 1e-13, (k, np.abs(drift).max(), st ** 2 / 12 * jerk * t)
        assert np.abs(drift).max() <= st ** 2 * acc * t + 1e-13, (k, np.abs(drift).max(), st ** 2 * acc * t)
    print('no disturbance: drift %.2e after %.1f s (bounds %.2e / %.2e)' % (np.abs(drift).max(), t, st ** 2 / 12 * jerk * t, st ** 2 * acc * t))


def test_plant_refuses_what_it_does_not_simulate(cfg2_small):
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = workloads.quadrotor_p2p(2)
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    with pytest.raises(NotImplementedError) as e:
        m.plant()
    assert problem.vehicles[0].label in str(e.value)
    problem, P = cfg2_small
    veh = problem.vehicles[0]
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    veh.options['1storder_delay'] = True
    try:
        with pytest.raises(NotImplementedError) as e:
            m.plant()
        assert type(veh).__name__ in str(e.value) and '1storder_delay' in str(e.value)
    finally:
        veh.options['1storder_delay'] = False
    m.pool = object()
    with pytest.raises(NotImplementedError):
        m.plant()
    with pytest.raises(ValueError):
        BatchP2P(problem, P, ops=port_binding, options=OPTS).plant(disturbance=np.zeros((8, 2, 5, 11)))


def test_input_disturbance_is_seeded_and_shaped():
    from omgtools.batch import input_disturbance
    a = input_disturbance(3, 2, 5, 10, 1001, fc=0.1, stdev=0.05, seed=3)
    assert a.shape == (3, 2, 5, 11) and a.dtype == np.float64 and a.flags['C_CONTIGUOUS']
    assert np.array_equal(a, input_disturbance(3, 2, 5, 10, 1001, fc=0.1, stdev=0.05, seed=3))
    assert not np.array_equal(a, input_disturbance(3, 2, 5, 10, 1001, fc=0.1, stdev=0.05, seed=4))
    assert 0.1 * 0.05 < a.std() < 0.05                      # (low-pass filtered: a fraction of the white noise's power is left)
    assert not input_disturbance(3, 2, 5, 10, 1001, fc=0.1, stdev=0.0, seed=3).any()
    b = input_disturbance(3, 2, 5, 10, 1001, fc=0.1, stdev=[0.05, 0.0], mean=[0.0, 0.25], seed=3)
    assert np.abs(b[:, 1] - 0.25).max() < 1e-12 and b[:, 0].std() > 0.005
    # the fixture's realisation is this function's
    p = np.load(os.path.join(GOLD, 'plant_holonomic.npz'))
    assert np.array_equal(p['dist'], input_disturbance(4, 2, 12, 10, 1001, fc=float(p['fc']), stdev=float(p['stdev']), seed=int(p['seed'])))
