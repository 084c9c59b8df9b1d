"""The Quadrotor's plant (`BatchP2P.plant(model='quadrotor')`, `feedback(model='quadrotor')`; include/omgx.h OMGX_HAS_PLANT_QUADROTOR) on
the host loop, and the C-ABI surface of the device version: the simulated vehicle of the reference's default options with the model's
own `ode` (`vehicles/quadrotor.py:149-152`).  Fixture: tests/golden/plant_quadrotor.npz (generator:
tests/golden/generate_plant_quadrotor_golden.py), from the reference's own `Quadrotor` on 8 updates of solved plans."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OPTS = dict(tol=1e-3, max_iter=300)
N_SAMP = 10


def fixture():
    return np.load(os.path.join(GOLD, 'plant_quadrotor.npz'), allow_pickle=False)


def host_loop(n=4, **kw):
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = workloads.quadrotor_p2p(n)
    return BatchP2P(problem, P, ops=port_binding, options=OPTS, **kw)


def replay_quad_fixture(rep, q, predict, simulate, chained, get, put):
    """The fixture's plans and disturbance through an executor's simulate / predict (`predict(tau, t_rel)`, `simulate()`), x and p[o_t]
    set per update; unchained: the plant's state is set to the fixture's start-of-update state ahead of every simulate.  get / put:
    read / write an array of the executor.  Returns the predicted spl0 / dspl0 / ddspl0 [3, n_upd, 4, 2] (update 0: NaN)."""
    n_upd, T, upd = len(q['t_rel']), float(q['horizon_time']), float(q['update_time'])
    pred = np.full((3, n_upd, 4, 2), np.nan)
    for k in range(n_upd):
        if k:
            predict((float(q['t_rel'][k - 1]) + upd) / T, float(q['t_rel'][k]))      # (reads the plan and the t of update k - 1)
            pk = get(rep.p)
            for o in range(3):
                pred[o, k] = pk[:, rep.p_offs[o]:rep.p_offs[o] + 2]
        x, pp = get(rep.x).copy(), get(rep.p).copy()
        x[:, rep.o_spl:rep.o_spl + 2 * rep.L] = q['coeffs'][k].reshape(4, -1)
        pp[:, rep.o_t] = q['t_rel'][k]
        put(rep.x, x), put(rep.p, pp)
        if k and not chained:
            put(rep.plant_state()['state'], q['state_start'][k])
        simulate()
    return pred


def check_against_quad_fixture(q, sig, pred, chained):
    """The bounds of the issue against the reference's signals: state columns and the predicted spl0 within 10 x the deviation of the
    reference's own odeint from the Runge-Kutta statements (recorded in the fixture: per update, or chained over all of them; an
    off-by-one choice of samples shows at least `sample_shift_dev`, a hundred times the per-update deviation); input columns, dspl0 /
    ddspl0 and the dspl row of the log within 1e-10 absolute (third and lower derivatives of a degree-4 spline evaluated two ways, a
    sqrt and one division on values below about 20: hundreds of ulps at most)."""
    n_upd = len(q['t_rel'])
    n_col = 1 + N_SAMP * n_upd
    assert (sig['count'] == n_col).all() and not sig['overflow'].any()
    ode_dev, ode_ch, shift = (float(q[k]) for k in ('ode_dev', 'ode_dev_chained', 'sample_shift_dev'))
    assert shift >= 100 * ode_dev
    bound = 10 * (ode_ch if chained else ode_dev)
    err_st = np.abs(sig['state'] - q['state']).max()
    err_s0 = np.abs(pred[0, 1:] - q['spl0'][1:]).max()
    err_in = np.abs(sig['input'] - q['input']).max()
    err_d = max(np.abs(pred[1, 1:] - q['dspl0'][1:]).max(), np.abs(pred[2, 1:] - q['ddspl0'][1:]).max())
    err_dspl = np.abs(sig['splines'][:, 1] - q['dspl']).max()
    print('%s: state %.2e spl0 %.2e (bound %.2e) input %.2e dspl0 / ddspl0 %.2e dspl %.2e'
          % ('chained' if chained else 'per update', err_st, err_s0, bound, err_in, err_d, err_dspl))
    assert err_st <= bound and err_s0 <= bound
    assert err_in <= 1e-10 and err_d <= 1e-10 and err_dspl <= 1e-10


def host_replay(chained, q=None):
    q = fixture() if q is None else q
    host = host_loop()
    assert np.array_equal(np.asarray(host.basis.knots, dtype=float), q['knots']) and host.T == float(q['horizon_time'])
    host.plant(sample_time=float(q['sample_time']), max_updates=len(q['t_rel']), disturbance=q['dist'], model='quadrotor',
               gravity=float(q['gravity']))
    host.record_signals(sample_time=float(q['sample_time']), max_updates=len(q['t_rel']))

    def put(dst, src):
        dst[...] = src
    pred = replay_quad_fixture(host, q, host._plant_predict, host._plant_simulate, chained, np.asarray, put)
    return host, pred


@pytest.mark.parametrize('chained', [False, True])
def test_host_twin_equals_the_reference_quadrotor(chained):
    q = fixture()
    host, pred = host_replay(chained, q)
    sig, st = host.signals(), host.plant_state()
    assert (st['n_upd'] == len(q['t_rel'])).all() and not st['overflow'].any()
    assert sig['state'].shape == (4, 5, 81) and sig['input'].shape == (4, 2, 81)
    check_against_quad_fixture(q, sig, pred, chained)
    # what the plant carries is what the log ends with
    assert np.array_equal(st['state'], sig['state'][:, :, -1]) and np.array_equal(st['input_last'], sig['input'][:, :, -1])
    assert np.abs(st['dspl_last'] - sig['splines'][:, 1, :, -1]).max() <= 1e-12      # (the same derivative, its factors in another order)
    assert np.array_equal(st['state_prev'], sig['state'][:, :, -1 - N_SAMP] if chained else q['state_start'][-1])


def test_stop_rule_needs_position_and_plan_velocity():
    """`quadrotor.py:104-110`: the travelled position against poseT AND the plan's velocity at the last travelled sample."""
    m = host_loop()
    m.plant(sample_time=0.01, max_updates=4, model='quadrotor')
    m.stop_at_arrival(stop_tol=1e-2)
    assert m.under_way.all()
    pl, tol = m.plant_state(), 1e-2
    pose = m.p[:, m._pl['o_pose']:m._pl['o_pose'] + 2]
    pl['n_upd'][:] = 1
    pl['state'][:, :2] = pose + np.array([[0.5 * tol, 0.0], [0.0, 0.9 * tol], [3 * tol, 0.0], [0.0, 0.0]])
    pl['state'][:, 2:] = 7.0                                  # (the vehicle's own velocity and pitch are not in the rule)
    pl['dspl_last'][:] = np.array([[0.0, 0.9 * tol], [0.0, 1.5 * tol], [0.0, 0.0], [2 * tol, 0.0]])
    assert np.array_equal(m.arrived(tol), [True, False, False, False])
    p_before = m.p.copy()
    m._plant_predict(0.02, 0.1)
    assert np.array_equal(m.under_way, [False, True, True, True])
    assert np.array_equal(m.p[0], p_before[0]) and (m.p[1:, m.o_t] == 0.1).all()      # (a stopped agent is not predicted)
    # ahead of the first simulate nothing has been travelled: no agent stops
    m2 = host_loop()
    m2.plant(sample_time=0.01, max_updates=4, model='quadrotor')
    m2.stop_at_arrival(stop_tol=1e-2)
    m2.plant_state()['state'][:, :2] = m2.p[:, m2._pl['o_pose']:m2._pl['o_pose'] + 2]
    m2._plant_predict(0.02, 0.1)
    assert m2.under_way.all()


def test_refusals(cfg2_small):
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    m = host_loop()
    label = m.veh.label
    for call in (m.plant, m.feedback):      # without the model: as before, now with the hint
        with pytest.raises(NotImplementedError) as e:
            call()
        assert label in str(e.value) and "model='quadrotor'" in str(e.value)
    with pytest.raises(ValueError):
        m.plant(model='unicycle')
    with pytest.raises(NotImplementedError) as e:
        m.plant(model='quadrotor', time_constant=0.1)
    assert 'lag' in str(e.value)
    with pytest.raises(ValueError):
        m.plant(model='quadrotor', disturbance=np.zeros((4, 5, 200, 11)))      # (the inputs are two, not the five states)
    with pytest.raises(ValueError):
        m.plant(model='quadrotor', sample_time=0.001)                           # (101 samples: more than a lane each)
    assert m._pl is None and m._fb is None
    problem, P = cfg2_small                                                      # a Holonomic batch has no spl0 / dspl0 / ddspl0
    holo = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    for call in (holo.plant, holo.feedback):
        with pytest.raises(ValueError) as e:
            call(model='quadrotor')
        assert 'spl0' in str(e.value)
    # rollout with this plant
    m.plant(model='quadrotor', max_updates=4)
    with pytest.raises(NotImplementedError) as e:
        m.rollout(3)
    assert 'per step' in str(e.value)
    with pytest.raises(ValueError):                                              # (a loop has one source of states)
        m.feedback(model='quadrotor')
        m.step(states=np.zeros((4, 5)))
    m.plant(on=False)
    assert m._pl is None
    # measured states
    m.feedback(model='quadrotor')
    for bad in (np.zeros((4, 2)), np.zeros((5, 5)), np.zeros((4, 6))):
        with pytest.raises(ValueError):
            m.step(states=bad)
    with pytest.raises(ValueError) as e:
        m.step(states=np.zeros((4, 5)), inputs=np.zeros((4, 2)), enforce=True)
    assert 'inputs' in str(e.value)
    with pytest.raises(ValueError):
        m.step(states=np.zeros((4, 5)), fresh=np.ones(3, dtype=np.int32))
    m.feedback(on=False)
    # a host pool runs the step glue in its workers
    m.pool = object()
    try:
        with pytest.raises(NotImplementedError):
            m.plant(model='quadrotor')
        with pytest.raises(NotImplementedError):
            m.feedback(model='quadrotor')
    finally:
        m.pool = None
    assert m._pl is None and m._fb is None


def test_enforce_and_fresh_on_the_host_loop():
    """`Quadrotor.set_initial_conditions`: the measured position, at rest; an agent without a fresh measurement gets the ideal prediction."""
    q = fixture()
    upd, T = float(q['update_time']), float(q['horizon_time'])
    rng = np.random.default_rng(4)
    S = rng.normal(size=(4, 5))
    fresh = np.array([1, 0, 1, 0], dtype=np.int32)
    out = {}
    for mode in ('ideal', 'fed', 'enforce'):
        m = host_loop()
        m.x[:, m.o_spl:m.o_spl + 2 * m.L] = q['coeffs'][0].reshape(4, -1)
        m.p[:, m.o_t] = q['t_rel'][0]
        m._plan_ready = True
        if mode == 'ideal':
            m._predict(upd / T, upd)
        else:
            m.feedback(model='quadrotor')
            m._feedback_predict(upd / T, upd, S, None, fresh, mode == 'enforce')
        out[mode] = m.p.copy()
        o0, o1, o2 = m.p_offs
    assert np.array_equal(out['fed'][[1, 3]], out['ideal'][[1, 3]]) and np.array_equal(out['enforce'][[1, 3]], out['ideal'][[1, 3]])
    assert np.array_equal(out['enforce'][[0, 2], o0:o0 + 2], S[[0, 2], :2]) and not out['enforce'][[0, 2], o1:o2 + 2].any()
    assert np.array_equal(out['fed'][:, o1:o2 + 2], out['ideal'][:, o1:o2 + 2]) and (out['fed'][:, m.o_t] == upd).all()
    assert np.abs(out['fed'][[0, 2], o0:o0 + 2] - out['ideal'][[0, 2], o0:o0 + 2]).min() > 1e-2      # (integrated from S, not from the plan)


def _spec(**kw):
    """A specification that is in order, on a degree-4 plan with 13 knot intervals, and the arrays it points at."""
    from omgtools.backend import CQuadPlantSpec
    knots = np.r_[np.zeros(4), np.linspace(0, 1, 14), np.ones(4)]
    keep = dict(knots=knots, a=np.zeros(64), i=np.zeros(8, dtype=np.int32))
    sp = CQuadPlantSpec()
    for nm in ('state', 'state_prev', 'input_last', 'dspl_last'):
        setattr(sp, nm, keep['a'].ctypes.data)
    sp.n_upd, sp.knots = keep['i'].ctypes.data, knots.ctypes.data
    sp.coeff_off, sp.n_spl, sp.degree, sp.n_knots, sp.n_samp, sp.max_updates, sp.p_t, sp.p_poseT = 0, 2, 4, len(knots), 10, 8, 6, 8
    sp.p_off[0], sp.p_off[1], sp.p_off[2] = 0, 2, 4
    sp.sample_time, sp.inv_T, sp.stop_tol, sp.g = 0.01, 0.2, 1e-2, 9.81
    for k, v in kw.items():
        setattr(sp, k, v)
    sp._keep = keep
    return sp


def test_abi_surface_of_the_quadrotor_plant():
    """The header declares OMGX_HAS_PLANT_QUADROTOR and the two entries, the library exports them, the ABI version is still 9 and
    omgx_plant_spec still 128 bytes; against a null handle the argument checks come in the order of the header, every refusal names the
    entry and the field, and "null handle" is the answer only when everything that needs no device is in order."""
    from omgtools.backend import LIB_PATH, PROTOTYPES, CPlantSpec, CQuadPlantSpec, CSignalsSpec
    header = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    assert re.search(r'#define\s+OMGX_HAS_PLANT_QUADROTOR\s+1\b', header) and re.search(r'#define\s+OMGX_VERSION\s+9\b', header)
    lib = ctypes.CDLL(LIB_PATH)
    lib.omgx_version.restype = ctypes.c_int
    lib.omgx_last_error.restype = ctypes.c_char_p
    assert lib.omgx_version() == 9 and ctypes.sizeof(CPlantSpec) == 128 and ctypes.sizeof(CQuadPlantSpec) == 168
    V, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32
    sim, prd = lib.omgx_batch_plant_quadrotor_simulate, lib.omgx_batch_plant_quadrotor_predict
    for name in ('omgx_batch_plant_quadrotor_simulate', 'omgx_batch_plant_quadrotor_predict'):
        assert re.search(r'\bint\s+%s\s*\(' % name, header) and name in PROTOTYPES
    sim.argtypes, sim.restype = [V, V, V, ctypes.POINTER(CQuadPlantSpec), ctypes.POINTER(CSignalsSpec)], ctypes.c_int
    prd.argtypes, prd.restype = [V, V, V, D, D, ctypes.POINTER(CQuadPlantSpec), V, V, I], ctypes.c_int
    xp = np.zeros(8)
    X = xp.ctypes.data

    def simulate(sp, x=X, p=X, log=None):
        rc = sim(None, x, p, None if sp is None else ctypes.byref(sp), None if log is None else ctypes.byref(log))
        return rc, lib.omgx_last_error()

    def predict(sp, x=X, p=X, tau=0.02, t=0.1, states=None, fresh=None, enforce=0):
        rc = prd(None, x, p, tau, t, None if sp is None else ctypes.byref(sp), states, fresh, enforce)
        return rc, lib.omgx_last_error()
    short = np.r_[np.zeros(4), np.ones(4)]      # (8 knots: fewer than 2 * degree + 2)
    # in the order of the checks: each specification is wrong in its field AND in later ones, and the first is named
    cases = [(dict(state=None, degree=2), b'state'), (dict(dspl_last=None, n_spl=3), b'dspl_last'), (dict(n_upd=None, n_samp=0), b'n_upd'),
             (dict(knots=None, degree=2), b'knots'), (dict(degree=2, n_spl=3, n_samp=64), b'degree = 2'), (dict(degree=6), b'degree = 6'),
             (dict(knots=short.ctypes.data, n_knots=8, n_spl=3), b'n_knots = 8'), (dict(n_knots=41, n_samp=99), b'n_knots = 41'),
             (dict(n_spl=3, n_samp=64), b'n_spl = 3'), (dict(n_spl=1, g=0.0), b'n_spl = 1'), (dict(coeff_off=-1, g=0.0), b'coeff_off'),
             (dict(inv_T=0.0, n_samp=64), b'inv_T'), (dict(n_samp=64, max_updates=0), b'n_samp = 64'), (dict(n_samp=0, g=0.0), b'n_samp = 0'),
             (dict(max_updates=0, sample_time=0.0), b'max_updates'), (dict(sample_time=0.0, g=0.0), b'sample_time'),
             (dict(g=0.0, stop_tol=float('nan')), b'g = 0'), (dict(g=float('nan')), b'g = '), (dict(stop_tol=float('nan')), b'stop_tol')]
    for kw, word in cases:
        for who, call in ((b'plant_quadrotor_simulate:', simulate), (b'plant_quadrotor_predict:', predict)):
            rc, msg = call(_spec(**kw))
            assert rc == -1 and msg.startswith(who) and word in msg and b'null handle' not in msg, (kw, msg)
    for who, call in ((b'plant_quadrotor_simulate:', simulate), (b'plant_quadrotor_predict:', predict)):
        for kw in (dict(sp=None), dict(sp=_spec(), x=None), dict(sp=_spec(), p=None)):
            rc, msg = call(**kw)
            assert rc == -1 and msg.startswith(who) and b'null x / p / specification' in msg, msg
        rc, msg = call(_spec())
        assert rc == -1 and msg == b'null handle', msg
        rc, msg = call(_spec(n_samp=63, dist=None, overflow=None, under_way=None))      # (the largest update: a lane per sample)
        assert rc == -1 and msg == b'null handle', msg
    # the log of a simulate: both arrays or neither, and only with the specification that carries count and cap
    rc, msg = simulate(_spec(log_state=X))
    assert rc == -1 and msg.startswith(b'plant_quadrotor_simulate:') and b'log_state' in msg
    rc, msg = simulate(_spec(log_state=X, log_input=X))
    assert rc == -1 and b'log specification' in msg
    good = _spec()
    cnt = np.zeros(4, dtype=np.int32)
    log = CSignalsSpec(X, cnt.ctypes.data, None, good.knots, 0, 2, 4, good.n_knots, 3, 10, 81, 6, 0.01, 0.2)
    rc, msg = simulate(_spec(log_state=X, log_input=X), log=log)
    assert rc == -1 and msg == b'null handle', msg
    for field, value in (('n_samp', 5), ('sample_time', 0.02), ('degree', 3), ('inv_T', 0.25)):
        other = CSignalsSpec(X, cnt.ctypes.data, None, good.knots, 0, 2, 4, good.n_knots, 3, 10, 81, 6, 0.01, 0.2)
        setattr(other, field, value)
        rc, msg = simulate(_spec(), log=other)
        assert rc == -1 and msg.startswith(b'plant_quadrotor_simulate:') and b"plant's plan" in msg, (field, msg)
    # measured states: the plant's own arrays are not needed, fresh / enforce go with states, the clock must be numbers
    S = np.zeros((4, 5))
    bare = dict(state=None, state_prev=None, input_last=None, dspl_last=None, n_upd=None, max_updates=0)
    rc, msg = predict(_spec(**bare), states=S.ctypes.data, fresh=cnt.ctypes.data, enforce=1)
    assert rc == -1 and msg == b'null handle', msg
    rc, msg = predict(_spec(), fresh=cnt.ctypes.data)
    assert rc == -1 and msg.startswith(b'plant_quadrotor_predict:') and b'fresh / enforce' in msg
    rc, msg = predict(_spec(), enforce=1)
    assert rc == -1 and b'fresh / enforce' in msg
    for kw in (dict(tau=float('nan')), dict(t=float('nan'))):
        rc, msg = predict(_spec(degree=2), **kw)
        assert rc == -1 and msg.startswith(b'plant_quadrotor_predict:') and b'not a number' in msg, msg


def test_fixture_holds_data_only():
    q = fixture()                                             # (allow_pickle=False: no object arrays)
    want = {'knots', 'coeffs', 't_rel', 'dist', 'horizon_time', 'update_time', 'sample_time', 'knot_time', 'gravity', 'state_start',
            'ode_dev', 'ode_dev_chained', 'sample_shift_dev', 'accelerating', 'fc', 'stdev', 'seed', 'state', 'input', 'dspl', 'spl0',
            'dspl0', 'ddspl0'}
    assert set(q.files) == want
    for k in q.files:
        assert q[k].dtype.kind in 'fi', (k, q[k].dtype)
    assert os.path.getsize(os.path.join(GOLD, 'plant_quadrotor.npz')) < 1 << 20
    assert q['coeffs'].shape == (8, 4, 2, 17) and q['dist'].shape == (4, 2, 8, 11) and q['state'].shape == (4, 5, 81)
    assert abs(float(q['knot_time']) - 0.3846) < 1e-4 and float(q['t_rel'][3]) > float(q['t_rel'][4])      # (the knot crossing)
    assert float(q['sample_shift_dev']) >= 100 * float(q['ode_dev']) and np.abs(q['dist']).max() > 1e-3
