"""The travelled-trajectory log (`BatchP2P.record_signals`) on the host loop, and the C-ABI surface of the device version:
what the reference's `Simulator.run` returns as `vehicle.signals` (`Vehicle.simulate` with `ideal_update`,
`vehicles/vehicle.py:359-369`)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'signals_holonomic.npz')
OPTS = dict(tol=1e-3, max_iter=300)


def test_host_log_equals_the_reference_signals(cfg2_small):
    """tests/golden/signals_holonomic.npz (generator: tests/golden/generate_signals_golden.py): the reference's own
    `Holonomic.store` + `Vehicle.simulate` fed with the plans of four agents over 12 updates (update_time 0.1, sample_time 0.01,
    the knot at 0.909 s crossed at t = 1.0).  (a) The host append fed with the same plans and (b) the log of the host loop itself
    equal the reference's state / input / dinput within 1e-10 (the tolerance of tests/test_gpu_glue.py for samples against
    `splines2signals`; values are O(10) m); 1 + 10 * 12 columns."""
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = cfg2_small
    g = np.load(GOLD)
    agents, n_upd = g['agents'], len(g['t_rel'])
    n_col = 1 + 10 * 12
    assert n_upd == 12 and g['state'].shape == (4, 2, n_col)
    want = np.stack([g['state'], g['input'], g['dinput']], axis=1)           # [4, 3, 2, n_col]
    # (a) the golden plans through the host append: pure spline evaluation on both sides
    rep = BatchP2P(problem, dict(P, p=P['p'][agents], x0=P['x0'][agents]), ops=port_binding, options=OPTS)
    assert np.array_equal(np.asarray(rep.basis.knots, dtype=float), g['knots']) and rep.T == float(g['horizon_time'])
    rep.record_signals(sample_time=float(g['sample_time']), max_updates=n_upd)
    for k in range(n_upd):
        rep.x[:, rep.o_spl:rep.o_spl + 2 * rep.L] = g['coeffs'][k].reshape(4, -1)
        rep.p[:, rep.o_t] = g['t_rel'][k]
        rep._signals_append_host(None)
    s = rep.signals()
    assert (s['count'] == n_col).all() and not s['overflow'].any() and s['splines'].shape == (4, 3, 2, n_col)
    err_a = np.abs(s['splines'] - want).max()
    # (b) the host loop itself
    mpc = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    mpc.record_signals(sample_time=0.01, max_updates=n_upd)
    mpc.solve_cold()
    crossings = sum(int(mpc.step()) for _ in range(n_upd - 1))
    s = mpc.signals()
    err_b = max(np.abs(s[nm][agents] - g[nm]).max() for nm in ('state', 'input', 'dinput'))
    print('host append vs reference: %.3e, host loop vs reference: %.3e' % (err_a, err_b))
    assert crossings == 1
    assert (s['count'] == n_col).all() and not s['overflow'].any()
    assert err_a <= 1e-10 and err_b <= 1e-10
    assert np.abs(s['time'][:n_col] - g['time']).max() < 1e-12
    assert s['state'].base is not None and np.shares_memory(s['state'], s['splines'])      # views of the log
    # `record_signals` after `solve_cold` (the order of tests/test_gpu_rollout.py): the same log
    late = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    late.solve_cold()
    late.record_signals(sample_time=0.01, max_updates=n_upd)
    assert (late.signals()['count'] == 11).all()
    for _ in range(n_upd - 1):
        late.step()
    assert np.array_equal(late.signals()['splines'], s['splines']) and np.array_equal(late.signals()['count'], s['count'])


def _meets(sig, b, c, pose, tol):
    return np.linalg.norm(sig['state'][b, :, c] - pose[b]) <= tol * (1 + 1e-9) and np.linalg.norm(sig['input'][b, :, c]) <= tol * (1 + 1e-9)


def test_stop_rule_ends_an_agents_log():
    """With `stop_at_arrival` an agent is appended at the updates it is under way and at no other: count = 1 + n_samp * (updates
    under way), different between agents.  The last logged column of an arrived agent is the state the criterion held on (the
    prediction of the update it stopped at is the plan at that very time), within a relative 1e-9 for two evaluation routines of one
    polynomial; the last column of an agent that the NEXT update still finds under way does not meet it."""
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = workloads.holonomic_p2p(6)
    tol = 2.5                                           # (as tests/test_batch_mpc_cpu.py: some metres out, arrivals at different updates)
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    m.stop_at_arrival(stop_tol=tol)
    m.record_signals(sample_time=0.01, max_updates=50)
    m.solve_cold()
    updates = m.under_way.astype(int).copy()
    for k in range(40):
        m.step()
        updates += m.under_way
    o_pose = m.tpl.entry_range(m.veh.label, 'poseT', 'par')[0]
    pose = m.p[:, o_pose:o_pose + 2]
    s = m.signals()
    count = s['count'].copy()
    print('updates under way:', updates.tolist(), 'count:', count.tolist())
    assert np.array_equal(count, 1 + 10 * updates) and not s['overflow'].any()
    assert len(set(count.tolist())) >= 2 and (~m.under_way).sum() >= 3
    last_before = [(_meets(s, b, count[b] - 1, pose, tol)) for b in range(6)]
    m.step()                                            # the update that tests the last logged state of the agents under way
    s = m.signals()
    for b in range(6):
        if not m.under_way[b]:
            assert _meets(s, b, s['count'][b] - 1, pose, tol), b
            assert s['count'][b] == count[b]            # (stopped: nothing appended)
        else:
            assert not last_before[b], b
            assert s['count'][b] == count[b] + 10
    # the summary of the log: numpy statements on the host loop
    sm = m.summary()
    assert np.array_equal(sm[:, 0], s['count']) and np.allclose(sm[:, 1], (s['count'] - 1) * 0.01, rtol=0, atol=1e-12)
    for b in range(6):
        n = s['count'][b]
        assert abs(sm[b, 5] - np.linalg.norm(s['state'][b, :, n - 1] - pose[b])) < 1e-12
        assert abs(sm[b, 2] - np.linalg.norm(np.diff(s['state'][b, :, :n], axis=1), axis=0).sum()) < 1e-12
        assert abs(sm[b, 3] - np.linalg.norm(s['input'][b, :, :n], axis=0).max()) < 1e-12 and sm[b, 7] == 0.


def test_capacity_overflow_leaves_the_log_alone(cfg2_small):
    """A log one column short of the third update: the append is dropped as a whole -- `overflow` set, `count` and the agent's block
    as they were -- and nothing is written past it."""
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = cfg2_small
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    with pytest.raises(ValueError):
        m.record_signals(sample_time=0.01, cap=10)
    m.record_signals(sample_time=0.01, cap=1 + 10 * 3 - 1)
    m.solve_cold()
    m.step()
    s = m.signals()
    assert (s['count'] == 21).all() and not s['overflow'].any()
    before = s['splines'].copy()
    m.step()
    s = m.signals()
    assert (s['overflow'] == 1).all() and (s['count'] == 21).all() and np.array_equal(s['splines'], before)
    m.record_signals(on=False)
    with pytest.raises(RuntimeError):
        m.signals()


def test_pool_variant_refuses_the_log():
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = workloads.holonomic_p2p(2)
    m = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    m.pool = object()
    with pytest.raises(NotImplementedError):
        m.record_signals()


class _Spec(ctypes.Structure):
    _fields_ = [('log', ctypes.c_void_p), ('count', ctypes.c_void_p), ('overflow', ctypes.c_void_p), ('knots', ctypes.c_void_p),
                ('coeff_off', ctypes.c_int32), ('n_spl', ctypes.c_int32), ('degree', ctypes.c_int32), ('n_knots', ctypes.c_int32),
                ('n_der', ctypes.c_int32), ('n_samp', ctypes.c_int32), ('cap', ctypes.c_int32), ('p_t', ctypes.c_int32),
                ('sample_time', ctypes.c_double), ('inv_T', ctypes.c_double)]


def test_abi_surface_of_the_signal_log():
    """The header declares the three entry points and OMGX_HAS_SIGNALS, the library exports them, the ABI version is still 9, and an
    inconsistent specification is refused with OMGX_E_INVALID and a message by a host-only check (no device, no handle)."""
    from omgtools.backend import LIB_PATH, CSignalsSpec
    header = open(os.path.join(ROOT, 'include', 'omgx.h')).read()
    assert re.search(r'#define\s+OMGX_HAS_SIGNALS\s+1\b', header) and re.search(r'#define\s+OMGX_VERSION\s+9\b', header)
    assert 'typedef struct omgx_signals_spec' in header
    lib = ctypes.CDLL(LIB_PATH)
    lib.omgx_version.restype = ctypes.c_int
    lib.omgx_last_error.restype = ctypes.c_char_p
    assert lib.omgx_version() == 9
    for name in ('omgx_batch_set_signals', 'omgx_batch_signals_append', 'omgx_batch_signals_reduce'):
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
        assert hasattr(lib, name), name
    assert [f[0] for f in CSignalsSpec._fields_] == [f[0] for f in _Spec._fields_] and ctypes.sizeof(CSignalsSpec) == ctypes.sizeof(_Spec) == 80
    lib.omgx_batch_set_signals.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Spec)]
    lib.omgx_batch_signals_append.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_Spec)]
    lib.omgx_batch_signals_reduce.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Spec), ctypes.c_void_p, ctypes.c_void_p]
    knots = np.r_[np.zeros(3), np.linspace(0., 1., 12), np.ones(3)]
    dummy = np.zeros(8)                                   # (never dereferenced: the checks come first)

    def spec(**kw):
        f = dict(log=dummy.ctypes.data, count=dummy.ctypes.data, overflow=None, knots=knots.ctypes.data, coeff_off=0, n_spl=2, degree=3,
                 n_knots=len(knots), n_der=3, n_samp=10, cap=121, p_t=0, sample_time=0.01, inv_T=0.1)
        f.update(kw)
        return _Spec(**f)
    bad = [(dict(cap=10), b'cap'), (dict(n_der=5), b'n_der'), (dict(n_knots=41), b'n_knots'), (dict(p_t=-1), b'p_t'),
           (dict(log=None), b'null'), (dict(sample_time=0.0), b'positive')]
    for kw, word in bad:
        sp = spec(**kw)
        assert lib.omgx_batch_set_signals(None, ctypes.byref(sp)) == -1, kw
        assert word in lib.omgx_last_error(), (kw, lib.omgx_last_error())
        assert lib.omgx_batch_signals_append(None, None, None, None, ctypes.byref(sp)) == -1
        assert word in lib.omgx_last_error()
        assert lib.omgx_batch_signals_reduce(None, ctypes.byref(sp), None, None) == -1
    good = spec()
    assert lib.omgx_batch_set_signals(None, ctypes.byref(good)) == -1 and b'null handle' in lib.omgx_last_error()
    assert lib.omgx_batch_set_signals(None, None) == -1
