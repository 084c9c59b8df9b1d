"""Measured states fed back into the per-step loop (`BatchP2P.feedback`, `step(states=...)`) on the host loop, and the C-ABI surface
of the device version (`omgx_batch_predict_measured`): the reference's `Deployer.update(current_time, states, ...)` ->
`Vehicle.predict(state0=...)` with its `enforce_states` / `enforce_inputs` forms (`vehicles/vehicle.py:302-337`).  Fixture:
tests/golden/feedback_holonomic.npz (generator: tests/golden/generate_feedback_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_plant_cpu import plan_inputs, trapezoid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OPTS = dict(tol=1e-3, max_iter=300)
LOOP_ARRAYS = ('x', 'p', 'lam', 'status', 'iters')


class _Feedback(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('state', 'input', 'fresh', 'knots')] + \
               [(n, ctypes.c_int32) for n in ('coeff_off', 'n_spl', 'degree', 'n_knots', 'n_samp', 'n_out')] + [('p_off', ctypes.c_int32 * 4)] + \
               [(n, ctypes.c_int32) for n in ('p_t', 'enforce')] + [(n, ctypes.c_double) for n in ('sample_time', 'inv_T')]


def test_abi_surface_of_the_feedback_entry():
    """The header declares OMGX_HAS_FEEDBACK, the specification and the entry, the library exports it, the ABI version is still 9 and
    omgx_plant_spec still 128 bytes; a specification that can be judged without a device is refused with OMGX_E_INVALID and the
    field named, ahead of the "null handle" answer."""
    from omgtools.backend import LIB_PATH, CFeedbackSpec, CPlantSpec
    header = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    assert re.search(r'#define\s+OMGX_HAS_FEEDBACK\s+1\b', header) and re.search(r'#define\s+OMGX_VERSION\s+9\b', header)
    assert 'typedef struct omgx_feedback_spec' in header and re.search(r'\bint\s+omgx_batch_predict_measured\s*\(', header)
    lib = ctypes.CDLL(LIB_PATH)
    lib.omgx_version.restype = ctypes.c_int
    lib.omgx_last_error.restype = ctypes.c_char_p
    assert lib.omgx_version() == 9 and hasattr(lib, 'omgx_batch_predict_measured')
    assert [f[0] for f in CFeedbackSpec._fields_] == [f[0] for f in _Feedback._fields_] and ctypes.sizeof(CFeedbackSpec) == ctypes.sizeof(_Feedback) == 96
    assert ctypes.sizeof(CPlantSpec) == 128
    V = ctypes.c_void_p
    lib.omgx_batch_predict_measured.argtypes = [V, V, V, ctypes.c_double, ctypes.c_double, ctypes.POINTER(_Feedback)]
    knots = np.r_[np.zeros(3), np.linspace(0., 1., 12), np.ones(3)]
    dummy = np.zeros(8)                                   # (never dereferenced: the checks come first)
    d = dummy.ctypes.data

    def spec(**kw):
        f = dict(state=d, input=None, fresh=None, knots=knots.ctypes.data, coeff_off=0, n_spl=2, degree=3, n_knots=len(knots), n_samp=10,
                 n_out=2, p_off=(ctypes.c_int32 * 4)(1, 3, -1, -1), p_t=0, enforce=0, sample_time=0.01, inv_T=0.1)
        f.update(kw)
        return _Feedback(**f)
    for kw, word in [(dict(n_knots=41), b'n_knots'), (dict(n_samp=0), b'n_samp'), (dict(state=None), b'state'), (dict(sample_time=0.0), b'sample_time'),
                     (dict(n_out=5), b'n_out'), (dict(p_off=(ctypes.c_int32 * 4)(-1, 3, -1, -1)), b'p_off[0]'), (dict(n_spl=65), b'n_spl'),
                     (dict(degree=0), b'degree'), (dict(inv_T=0.0), b'inv_T'), (dict(knots=None), b'knots'),
                     (dict(n_samp=4096), b'n_samp')]:        # (2 * 4097 input samples and the staged plan: beyond 64 KiB of LDS)
        sp = spec(**kw)
        assert lib.omgx_batch_predict_measured(None, d, d, 0.1, 0.1, ctypes.byref(sp)) == -1, kw
        msg = lib.omgx_last_error()
        assert msg.startswith(b'predict_measured:') and word in msg and b'null handle' not in msg, (kw, msg)
    good = spec()
    assert lib.omgx_batch_predict_measured(None, d, d, 0.1, 0.1, ctypes.byref(good)) == -1 and b'null handle' in lib.omgx_last_error()
    assert lib.omgx_batch_predict_measured(None, d, d, 0.1, 0.1, None) == -1 and b'null' in lib.omgx_last_error()
    assert lib.omgx_batch_predict_measured(None, None, d, 0.1, 0.1, ctypes.byref(good)) == -1 and b'null x' in lib.omgx_last_error()


def _host_loop(problem, P, **kw):
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    return BatchP2P(problem, P, ops=port_binding, options=OPTS, **kw)


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(getattr(a, nm)[rows], getattr(b, nm)[rows]) for nm in LOOP_ARRAYS)


def test_step_with_states_starts_the_solve_from_the_measurement(cfg2_small):
    """8 agents, the cold solve and three steps fed a state a few centimetres off the plan: p[state0] is that state plus the nominal
    trapezoid of the plan travelled since, recomputed here with scipy's B-splines (1e-12, the closed-form bound of
    tests/test_plant_cpu.py), p[input0] the plan's input at tau (1e-10, pure spline evaluation), p[t] the step's clock."""
    from scipy.interpolate import BSpline
    problem, P = cfg2_small
    m = _host_loop(problem, P)
    m.feedback(sample_time=0.01)
    m.solve_cold()
    knots, T, st = np.asarray(m.basis.knots, dtype=float), m.T, 0.01
    rng = np.random.default_rng(2)
    worst_s, worst_i = 0.0, 0.0
    for k in range(3):
        c = m.x[:, m.o_spl:m.o_spl + 2 * m.L].reshape(8, 2, m.L).copy()
        t_old = m.p[:, m.o_t].copy()
        S = np.stack([BSpline(knots, c[b].T, 3)(t_old[b] / T) for b in range(8)]) + rng.uniform(-0.03, 0.03, size=(8, 2))
        m.step(states=S)
        u = np.stack([plan_inputs(knots, c[b], float(t_old[b]), T, st, 10) for b in range(8)])
        worst_s = max(worst_s, np.abs(trapezoid(S, u, st)[..., -1] - m.p[:, m.o_state0:m.o_state0 + 2]).max())
        at_tau = np.stack([BSpline(knots, c[b].T, 3).derivative()((t_old[b] + 0.1) / T) / T for b in range(8)])
        worst_i = max(worst_i, np.abs(at_tau - m.p[:, m.o_input0:m.o_input0 + 2]).max())
        assert np.abs(m.p[:, m.o_t] - 0.1 * (k + 1)).max() <= 1e-12
    print('state0 against measured + nominal trapezoid: %.2e; input0 against the plan at tau: %.2e' % (worst_s, worst_i))
    assert worst_s <= 1e-12 and worst_i <= 1e-10


def replay_feedback_fixture(rep, g, f, get, put, feed):
    """The fixture's plans and measurements through an executor's `_feedback_predict`, x and p[o_t] set per update as
    tests/test_plant_cpu.py `replay_fixture` does (get / put: read / write an array of the executor, feed: an array as the executor takes
    measurements).  Returns predicted state0 / input0 [12, 4, 2] of the plain form, and of the two
    enforce forms (inputs None, inputs given)."""
    n_upd, T, upd = len(g['t_rel']), float(g['horizon_time']), float(g['update_time'])
    out = [np.full((n_upd, 4, 2), np.nan) for _ in range(6)]
    for k in range(1, n_upd):
        x, pp = get(rep.x).copy(), get(rep.p).copy()
        x[:, rep.o_spl:rep.o_spl + 2 * rep.L] = g['coeffs'][k - 1].reshape(4, -1)
        put(rep.x, x)
        tau = (float(g['t_rel'][k - 1]) + upd) / T
        for q, (inputs, enforce) in enumerate([(None, False), (None, True), (f['given_in'][k], True)]):
            pp[:, rep.o_t] = g['t_rel'][k - 1]
            pp[:, rep.o_state0:rep.o_state0 + 2], pp[:, rep.o_input0:rep.o_input0 + 2] = 7.0, 7.0      # (every entry has to be written)
            put(rep.p, pp)
            rep._feedback_predict(tau, float(g['t_rel'][k]), feed(f['measured'][k]), None if inputs is None else feed(inputs), None, enforce)
            pk = get(rep.p)
            out[2 * q][k], out[2 * q + 1][k] = pk[:, rep.o_state0:rep.o_state0 + 2], pk[:, rep.o_input0:rep.o_input0 + 2]
            assert np.array_equal(pk[:, rep.o_t], np.full(4, g['t_rel'][k]))
    return out


def check_against_feedback_fixture(f, out):
    """Inputs within 1e-10 (pure spline evaluation); states within 10 x the deviation of the reference's own odeint from the exact
    integral (recorded in the fixture; an off-by-one choice of samples would show `sample_shift_dev`, ten times that or more); both
    enforce forms exact, zeros for the input that was not given."""
    s0, i0, es, ei, gs, gi = out
    assert float(f['sample_shift_dev']) >= 10 * float(f['ode_dev'])
    err_s, err_i = np.abs(s0[1:] - f['state0'][1:]).max(), np.abs(i0[1:] - f['input0'][1:]).max()
    print('state0 %.2e (bound %.2e), input0 %.2e' % (err_s, 10 * float(f['ode_dev']), err_i))
    assert err_i <= 1e-10 and err_s <= 10 * float(f['ode_dev'])
    assert np.array_equal(es[1:], f['enf_state0'][1:]) and np.array_equal(ei[1:], f['enf_input0'][1:]) and not ei[1:].any()
    assert np.array_equal(gs[1:], f['enfi_state0'][1:]) and np.array_equal(gi[1:], f['enfi_input0'][1:])


def test_host_glue_equals_the_reference_prediction(cfg2_small):
    problem, P = cfg2_small
    g, f = np.load(os.path.join(GOLD, 'signals_holonomic.npz')), np.load(os.path.join(GOLD, 'feedback_holonomic.npz'))
    agents = g['agents']
    rep = _host_loop(problem, dict(P, p=P['p'][agents], x0=P['x0'][agents]))
    assert np.array_equal(np.asarray(rep.basis.knots, dtype=float), g['knots']) and rep.T == float(g['horizon_time'])
    rep.feedback(sample_time=float(g['sample_time']))

    def put(dst, src):
        dst[...] = src
    check_against_feedback_fixture(f, replay_feedback_fixture(rep, g, f, np.asarray, put, np.asarray))


def test_twin_of_the_plant_and_the_mixed_mask(cfg2_small):
    """Loop A runs with the plant and a disturbance; loop B with feedback, every step fed A's `state_prev` copied before that step:
    the same bits in x, p, lam, status, iters after the cold solve and after each of 12 steps (the tenth crosses a knot).  Loop C is
    fed the same states for half of the agents only: at the first step its agents without a measurement equal, row for row, loop D
    stepped without states, the others loop B (afterwards the histories differ by construction)."""
    from omgtools.batch import input_disturbance
    problem, P = cfg2_small
    A, Bm, Cm, D = (_host_loop(problem, P) for _ in range(4))
    A.plant(sample_time=0.01, max_updates=13, disturbance=input_disturbance(8, 2, 13, 10, 1001, fc=0.1, stdev=0.02, seed=1))
    Bm.feedback(sample_time=0.01)
    Cm.feedback(sample_time=0.01)
    for m in (A, Bm, Cm, D):
        m.solve_cold()
    assert _same(A, Bm) and _same(A, Cm) and _same(A, D)
    mask = np.array([1, 0, 1, 1, 0, 0, 1, 0], dtype=np.int32)
    crossings, moved = 0, 0.0
    for k in range(12):
        prev = A.plant_state()['state_prev'].copy()
        ideal = A.x[:, A.o_spl:A.o_spl + 2 * A.L].reshape(8, 2, A.L) @ A._eval_rows((A.p[0, A.o_t] + 0.1) / A.T)[0]
        crossings += int(A.step())
        Bm.step(states=prev)
        assert _same(A, Bm), k
        moved = max(moved, np.abs(Bm.p[:, Bm.o_state0:Bm.o_state0 + 2] - ideal).max())
        if k == 0:
            Cm.step(states=prev, fresh=mask)
            D.step()
            assert _same(Cm, D, mask == 0) and _same(Cm, Bm, mask == 1)
            assert not np.array_equal(Cm.p[mask == 1], D.p[mask == 1])
    print('12 steps, %d crossing(s); the measured prediction leaves the ideal one by up to %.2e' % (crossings, moved))
    assert crossings == 1 and moved > 1e-4


def test_feedback_refuses_what_it_does_not_do(cfg2_small):
    from omgtools import workloads
    problem, P = workloads.quadrotor_p2p(2)
    m = _host_loop(problem, P)
    with pytest.raises(NotImplementedError) as e:
        m.feedback()
    assert problem.vehicles[0].label in str(e.value)
    problem, P = cfg2_small
    m = _host_loop(problem, P)
    S = np.zeros((8, 2))
    with pytest.raises(RuntimeError):                       # (no feedback() yet)
        m.step(states=S)
    m.feedback(sample_time=0.01)
    with pytest.raises(ValueError):                         # (inputs without enforce)
        m.step(states=S, inputs=S)
    with pytest.raises(ValueError):                         # (inputs without states)
        m.step(inputs=S)
    for kw in (dict(states=np.zeros((7, 2))), dict(states=np.zeros((8, 3))), dict(states=S, fresh=np.ones(7, dtype=np.int32)),
               dict(states=S, inputs=np.zeros((8, 1)), enforce=True)):
        with pytest.raises(ValueError):
            m.step(**kw)
    assert m.time == 0.0                                    # (a refused step does not move the clock)
    with pytest.raises(ValueError):                         # (one sample grid)
        m.plant(sample_time=0.02)
    with pytest.raises(ValueError):
        m.record_signals(sample_time=0.02)
    m.plant(sample_time=0.01)
    with pytest.raises(ValueError):                         # (plant and states: a loop has one source of states)
        m.step(states=S)
    with pytest.raises(ValueError):
        m.feedback(sample_time=0.02)
    m = _host_loop(problem, P)
    m.pool = object()
    with pytest.raises(NotImplementedError):
        m.feedback()
    m.pool = None
    m.feedback()
    m.pool = object()
    with pytest.raises(NotImplementedError):
        m.step(states=S)
