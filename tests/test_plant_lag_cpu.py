"""The plant's first-order actuator lag (`BatchP2P.plant(time_constant=...)`, `omgx_batch_set_plant_lag`) on the host loop, and the
C-ABI surface of the device version: the reference's vehicle options `{'1storder_delay': True, 'time_constant': 0.1}`
(`Vehicle.simulate` with `_ode_1storder`, `vehicles/vehicle.py:378-381, 429-431`).  Fixture: tests/golden/plant_lag_holonomic.npz
(generator: tests/golden/generate_plant_lag_golden.py), on the plans of signals_holonomic.npz and the disturbance of
plant_holonomic.npz."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from test_plant_cpu import plan_inputs, trapezoid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OPTS = dict(tol=1e-3, max_iter=300)
LOOP_ARRAYS = ('x', 'p', 'lam', 'status', 'iters')


def lag(v0, a, h, tc, E=None):
    """The recursion of include/omgx.h (OMGX_HAS_PLANT_LAG) written out here: commanded samples a [..., n + 1], v0 [...] -> the
    lagged samples [..., n + 1].  tc, E: scalars or arrays that broadcast against v0."""
    E = np.exp(-h / np.asarray(tc, dtype=float)) if E is None else E
    v = np.empty_like(a)
    v[..., 0] = v0
    for i in range(a.shape[-1] - 1):
        s = (a[..., i + 1] - a[..., i]) / h
        r = tc * s
        v[..., i + 1] = (a[..., i + 1] - r) + ((v[..., i] - a[..., i]) + r) * E
    return v


def fixtures():
    return (np.load(os.path.join(GOLD, 'signals_holonomic.npz')), np.load(os.path.join(GOLD, 'plant_holonomic.npz')),
            np.load(os.path.join(GOLD, 'plant_lag_holonomic.npz')))


def replay_lag_fixture(rep, g, q, predict, simulate, chained, get, put):
    """tests/test_plant_cpu.py `replay_fixture` with the lag: unchained, the plant's state AND its last applied input are set to the
    fixture's start-of-update values ahead of every simulate.  Returns the predicted state0 / input0."""
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
            put(rep.plant_state()['state'], q['state_start'][k])
            put(rep.plant_state()['input_last'], q['input_start'][k])
        simulate()
    return state0, input0


def check_against_lag_fixture(g, p, q, sig, state0, input0, chained):
    """The bounds of the issue against the reference's signals: input columns within 10 x lag_dev, state columns within 10 x ode_dev
    (per update) / 10 x ode_dev_chained (chained), the predicted state0 within the same state bound and input0 within 1e-10 (pure
    spline evaluation) -- the bounds of tests/test_plant_cpu.py with this fixture's recorded deviations --, dinput equal to the
    plan's (1e-10, as there: the reference evaluates the same spline); an off-by-one choice of the commanded samples would show at
    least `sample_shift_dev`, ten times the per-update bounds or more.  Chained, the input columns carry the recursion's own v
    through the run and keep the per-update bound: a deviation in v_0 decays by E^n_samp = exp(-1) per update, so what
    accumulates stays below lag_dev / (1 - exp(-1)) = 1.6 lag_dev.  Against the recursion written in this file, from the run's own
    start values: 1e-12 (as the closed-form check of tests/test_plant_cpu.py)."""
    n_upd, n_samp, st, T, tc = len(g['t_rel']), 10, float(g['sample_time']), float(g['horizon_time']), float(q['time_constant'])
    n_col = 1 + n_samp * n_upd
    assert (sig['count'] == n_col).all() and not sig['overflow'].any()
    lag_dev, ode_dev, ode_ch, shift = (float(q[k]) for k in ('lag_dev', 'ode_dev', 'ode_dev_chained', 'sample_shift_dev'))
    assert shift >= 10 * max(lag_dev, ode_dev)
    bound_in, bound_st = 10 * lag_dev, 10 * (ode_ch if chained else ode_dev)
    err_in = np.abs(sig['input'][:, :, 1:] - q['input'][:, :, 1:]).max()
    err_col0 = np.abs(sig['input'][:, :, 0] - q['input'][:, :, 0]).max()
    err_din = np.abs(sig['dinput'] - q['dinput']).max()
    err_st = np.abs(sig['state'] - q['state']).max()
    err_s0 = np.abs(state0[1:] - q['state0'][1:]).max()
    err_i0 = np.abs(input0[1:] - q['input0'][1:]).max()
    worst = 0.0
    for k in range(n_upd):
        u = plan_inputs(g['knots'], g['coeffs'][k], float(g['t_rel'][k]), T, st, n_samp)                # [4, 2, n_samp + 1]
        a = u + p['dist'][:, :, k, :]
        start = sig['state'][:, :, k * n_samp] if chained or k == 0 else q['state_start'][k]
        v0 = u[..., 0] if k == 0 else (sig['input'][:, :, k * n_samp] if chained else q['input_start'][k])
        v = lag(v0, a, st, tc)
        cols = slice(k * n_samp + 1, (k + 1) * n_samp + 1)
        worst = max(worst, np.abs(trapezoid(start, v, st) - sig['state'][:, :, cols]).max(), np.abs(v[..., 1:] - sig['input'][:, :, cols]).max())
    print('%s: input %.2e (bound %.2e) column 0 %.2e dinput %.2e state %.2e state0 %.2e (bound %.2e) input0 %.2e, recursion written here %.2e'
          % ('chained' if chained else 'per update', err_in, bound_in, err_col0, err_din, err_st, err_s0, bound_st, err_i0, worst))
    assert err_in <= bound_in and err_col0 <= 1e-10 and err_din <= 1e-10 and err_i0 <= 1e-10
    assert err_st <= bound_st and err_s0 <= bound_st
    assert worst <= 1e-12


def test_abi_surface_of_the_plant_lag():
    """The header declares OMGX_HAS_PLANT_LAG and the entry, the library exports it, the ABI version is still 9 and omgx_plant_spec
    still 128 bytes; the argument checks come in the order of the header against a null handle, every message names the entry and
    the field, and "null handle" is the answer only when everything that needs no device is in order."""
    from omgtools.backend import LIB_PATH, PROTOTYPES, CPlantSpec
    header = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    assert re.search(r'#define\s+OMGX_HAS_PLANT_LAG\s+1\b', header) and re.search(r'#define\s+OMGX_VERSION\s+9\b', header)
    assert re.search(r'\bint\s+omgx_batch_set_plant_lag\s*\(', header)
    assert 'no first-order actuator lag.  Per agent' not in header
    lib = ctypes.CDLL(LIB_PATH)
    lib.omgx_version.restype = ctypes.c_int
    lib.omgx_last_error.restype = ctypes.c_char_p
    assert lib.omgx_version() == 9 and hasattr(lib, 'omgx_batch_set_plant_lag') and 'omgx_batch_set_plant_lag' in PROTOTYPES
    assert ctypes.sizeof(CPlantSpec) == 128
    V, D = ctypes.c_void_p, ctypes.c_double
    fn = lib.omgx_batch_set_plant_lag
    fn.argtypes, fn.restype = [V, V, V, ctypes.c_int32, D], ctypes.c_int
    h = 0.01
    tc = np.array([0.1, 0.02, 0.5])
    dec = np.array([math.exp(-h / t) for t in tc])

    def call(tc=tc, dec=dec, n=3, h=h):
        rc = fn(None, None if tc is None else tc.ctypes.data, None if dec is None else dec.ctypes.data, n, h)
        return rc, lib.omgx_last_error()
    # in the order of the checks: each call is wrong in its field AND in every later one it can be, and the first is named
    bad_tc, bad_dec, off_dec = tc.copy(), dec.copy(), dec.copy()
    bad_tc[1], bad_dec[2], off_dec[0] = 0.0, 1.0, dec[0] + 1e-9
    for kw, word in [(dict(dec=None, n=0, h=0.0), b'decay'), (dict(n=0, h=0.0, tc=bad_tc), b'n = 0'), (dict(h=0.0, tc=bad_tc), b'sample_time'),
                     (dict(h=float('nan')), b'sample_time'), (dict(h=-0.01), b'sample_time'), (dict(tc=bad_tc, dec=bad_dec), b'time_constant[1]'),
                     (dict(tc=np.array([0.1, np.inf, 0.5])), b'time_constant[1]'), (dict(tc=np.array([0.1, 0.02, np.nan])), b'time_constant[2]'),
                     (dict(tc=np.array([-0.1, 0.02, 0.5])), b'time_constant[0]'), (dict(dec=bad_dec), b'decay[2]'),
                     (dict(dec=np.array([dec[0], -1e-3, dec[2]])), b'decay[1]'), (dict(dec=off_dec), b'decay[0]')]:
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith(b'plant_lag:') and word in msg and b'null handle' not in msg, (kw, msg)
    # exp underflows to 0 for a tiny time constant: legal
    tiny = np.array([1e-6, 0.02, 0.5])
    rc, msg = call(tc=tiny, dec=np.array([0.0, dec[1], dec[2]]))
    assert rc == -1 and b'null handle' in msg, msg
    rc, msg = call()
    assert rc == -1 and b'null handle' in msg, msg
    rc, msg = call(tc=None, dec=None, n=0, h=0.0)          # (switching the lag off needs the handle only)
    assert rc == -1 and b'null handle' in msg, msg


def _host_loop(problem, P, **kw):
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    return BatchP2P(problem, P, ops=port_binding, options=OPTS, **kw)


@pytest.mark.parametrize('chained', [False, True])
def test_host_glue_equals_the_reference_plant_with_lag(cfg2_small, chained):
    problem, P = cfg2_small
    g, p, q = fixtures()
    agents = g['agents']
    rep = _host_loop(problem, dict(P, p=P['p'][agents], x0=P['x0'][agents]))
    assert np.array_equal(np.asarray(rep.basis.knots, dtype=float), g['knots']) and rep.T == float(g['horizon_time'])
    rep.plant(sample_time=float(g['sample_time']), max_updates=12, disturbance=p['dist'], time_constant=float(q['time_constant']))
    rep.record_signals(sample_time=float(g['sample_time']), max_updates=12)

    def put(dst, src):
        dst[...] = src
    state0, input0 = replay_lag_fixture(rep, g, q, rep._plant_predict, rep._plant_simulate, chained, np.asarray, put)
    st = rep.plant_state()
    assert (st['n_upd'] == 12).all() and not st['overflow'].any()
    sig = rep.signals()
    check_against_lag_fixture(g, p, q, sig, state0, input0, chained)
    assert np.array_equal(st['input_last'], sig['input'][:, :, -1])      # (the last applied input is the lagged one)
    # the lag really acts: the travelled inputs leave the commanded ones of the plain plant by far more than any bound above
    assert np.abs(sig['input'] - p['input']).max() > 100 * float(q['lag_dev'])


# ---- properties of the recursion, in this file's own arithmetic ---------------------------------------------------------------------
def test_constant_command_decays_geometrically():
    """a constant: s = r = 0 and v_n - a = (v_0 - a) E^n, to 1e-15 relative to max(|v_0|, |a|) -- the scale at which the three
    roundings of a step happen (2^-53 of it each, and what earlier steps left decays by E); relative to the decayed difference
    itself no such bound can hold, v_n - a cancels.  With a = 0 a step is the one product v E, and the bound holds relative to
    v_n itself."""
    h, n = 0.01, 10
    for tc in (0.02, 0.1, 0.5):
        E = math.exp(-h / tc)
        a = np.full((3, n + 1), 0.7)
        v0 = np.array([0.0, 1.5, -2.0])
        v = lag(v0, a, h, tc, E)
        rel = np.abs((v[:, n] - 0.7) - (v0 - 0.7) * E ** n) / np.maximum(np.abs(v0), 0.7)
        z = lag(v0, np.zeros((3, n + 1)), h, tc, E)
        rel0 = np.abs(z[1:, n] - v0[1:] * E ** n) / np.abs(v0[1:] * E ** n)
        print('tc %g: deviation from geometric decay %.2e of the scale; a = 0: %.2e of v_n' % (tc, rel.max(), rel0.max()))
        assert rel.max() <= 1e-15 and rel0.max() <= 1e-15 and z[0, n] == 0.0


def test_ramp_is_followed_with_a_constant_delay():
    """a ramp of slope s: v approaches a - tc s monotonically (the gap to it shrinks by E per sample and keeps its sign)."""
    h, n, tc, s = 0.01, 200, 0.1, 0.8
    a = (0.3 + s * h * np.arange(n + 1))[None, :]
    for v0 in (0.0, 1.0):
        v = lag(np.array([v0]), a, h, tc)
        gap = (v - (a - tc * s))[0]
        assert (np.abs(gap[1:]) < np.abs(gap[:-1])).all() and (np.sign(gap[1:40]) == np.sign(gap[0])).all()
        assert abs(gap[-1]) <= abs(gap[0]) * math.exp(-n * h / tc) * (1 + 1e-9) + 1e-15


def test_short_and_long_time_constants():
    """tc = h / 50: the travelled inputs stay within tc max|s| of the commanded ones (from a start on the command).  tc = 1000 h: the
    input moves by less than n h / tc max|a - v_0| over an update."""
    h, n = 0.01, 10
    rng = np.random.default_rng(4)
    a = np.cumsum(rng.normal(0., 0.05, (6, n + 1)), axis=1)
    slope = np.abs(np.diff(a, axis=1) / h).max()
    tc = h / 50
    v = lag(a[:, 0].copy(), a, h, tc)
    print('tc = h / 50: |v - a| %.2e (bound %.2e)' % (np.abs(v - a).max(), tc * slope))
    assert np.abs(v - a).max() <= tc * slope * (1 + 1e-12)
    tc = 1000 * h
    v0 = rng.normal(0., 1., 6)
    v = lag(v0, a, h, tc)
    moved, bound = np.abs(v - v0[:, None]).max(), n * h / tc * np.abs(a - v0[:, None]).max()
    print('tc = 1000 h: moved %.2e (bound %.2e)' % (moved, bound))
    assert 0 < moved < bound


# ---- the public interface -------------------------------------------------------------------------------------------------------
def _run(problem, P, rows, time_constant, steps=3, dist=None):
    m = _host_loop(problem, dict(P, p=P['p'][rows], x0=P['x0'][rows]))
    m.plant(sample_time=0.01, max_updates=steps + 1, disturbance=None if dist is None else dist[rows], time_constant=time_constant)
    m.record_signals(sample_time=0.01, max_updates=steps + 1)
    m.solve_cold()
    for _ in range(steps):
        m.step()
    return m


def _same_run(a, b, rows=slice(None)):
    sa, sb, pa, pb = a.signals(), b.signals(), a.plant_state(), b.plant_state()
    ok = all(np.array_equal(getattr(a, nm)[rows], getattr(b, nm)) for nm in LOOP_ARRAYS)
    ok = ok and all(np.array_equal(sa[nm][rows], sb[nm]) for nm in ('splines', 'count', 'overflow'))
    return ok and all(np.array_equal(pa[nm][rows], pb[nm]) for nm in pa)


def test_scalar_and_per_agent_time_constants(cfg2_small):
    """A scalar equals the same value as an array [B]; two different per-agent values in one batch of 8 each equal that agent's run
    in a batch of its own (host loop: the cold solve and 3 steps, disturbance and log on) -- the same bits."""
    from omgtools.batch import input_disturbance
    problem, P = cfg2_small
    dist = input_disturbance(8, 2, 4, 10, 1001, fc=0.1, stdev=0.02, seed=1)
    every = np.arange(8)
    a = _run(problem, P, every, 0.1, dist=dist)
    b = _run(problem, P, every, np.full(8, 0.1), dist=dist)
    assert _same_run(a, b)
    tcs = np.where(every % 2 == 0, 0.05, 0.3)
    mixed = _run(problem, P, every, tcs, dist=dist)
    assert not np.array_equal(mixed.signals()['input'], a.signals()['input'])
    for rows, tc in ((every[0::2], 0.05), (every[1::2], 0.3)):
        alone = _run(problem, P, rows, tc, dist=dist)
        assert _same_run(mixed, alone, rows), tc
    plain = _run(problem, P, every, None, dist=dist)
    assert np.abs(plain.signals()['input'] - a.signals()['input']).max() > 1e-4      # (the lag is not a no-op)


def test_refusals_leave_the_loop_as_it_was(cfg2_small):
    problem, P = cfg2_small
    veh = problem.vehicles[0]
    m = _host_loop(problem, P)
    m.plant(sample_time=0.01, max_updates=5, time_constant=0.2)
    before = m._pl
    keep = dict((k, (v[0].copy(), v[1].copy()) if k == 'lag' else v) for k, v in before.items())
    for tc in (0.0, -0.1, float('nan'), float('inf'), np.full(7, 0.1), np.full((8, 1), 0.1), np.r_[np.full(7, 0.1), 0.0], 1e20):
        with pytest.raises(ValueError):
            m.plant(sample_time=0.01, max_updates=9, time_constant=tc)
        assert m._pl is before
        assert all(np.array_equal(keep['lag'][i], before['lag'][i]) for i in (0, 1)) and before['max_updates'] == 5
    assert np.array_equal(before['lag'][1], [math.exp(-0.01 / 0.2)] * 8)
    m.plant(on=False)
    assert m._pl is None
    with pytest.raises(RuntimeError):
        m.plant_state()
    # a vehicle with the option set: refused without the argument (the batch reads no vehicle option on its own), taken with it
    veh.options['1storder_delay'] = True
    try:
        with pytest.raises(NotImplementedError) as e:
            m.plant()
        assert type(veh).__name__ in str(e.value) and '1storder_delay' in str(e.value) and "time_constant=vehicle.options['time_constant']" in str(e.value)
        assert m._pl is None
        m.plant(time_constant=0.1)
        lagged = m._pl
        assert lagged['lag'] is not None
        with pytest.raises(NotImplementedError):
            m.plant()
        assert m._pl is lagged                              # (the refused call left the lagged plant in place)
    finally:
        veh.options['1storder_delay'] = False
    m.plant()                                               # no argument: the plain plant, the lag is gone
    assert m._pl['lag'] is None
    m.solve_cold()
    with pytest.raises(RuntimeError):
        m.plant(time_constant=0.1)
    assert m._pl['lag'] is None


def test_feedback_ignores_the_lag_option(cfg2_small):
    """`feedback()` on a vehicle with '1storder_delay' set: `Vehicle.predict(state0=...)` has no lag in it, the measured vehicle is
    outside the loop -- the cold solve and two steps fed measured states give the bits of the same loop with the option off."""
    from scipy.interpolate import BSpline
    problem, P = cfg2_small
    veh = problem.vehicles[0]
    runs = []
    for option in (False, True):
        veh.options['1storder_delay'] = option
        try:
            m = _host_loop(problem, P)
            m.feedback(sample_time=0.01)
            m.solve_cold()
            rng = np.random.default_rng(2)
            knots, T = np.asarray(m.basis.knots, dtype=float), m.T
            for k in range(2):
                c = m.x[:, m.o_spl:m.o_spl + 2 * m.L].reshape(8, 2, m.L)
                S = np.stack([BSpline(knots, c[b].T, 3)(m.p[b, m.o_t] / T) for b in range(8)]) + rng.uniform(-0.03, 0.03, size=(8, 2))
                m.step(states=S)
            runs.append(m)
        finally:
            veh.options['1storder_delay'] = False
    assert all(np.array_equal(getattr(runs[0], nm), getattr(runs[1], nm)) for nm in LOOP_ARRAYS)
