"""Free end time in the batched loop, host side: the numpy twins of `omgx_batch_free_t_advance` / `_append` against the package's
restatement of the reference's `shift_spline` and `FreeTPoint2point.init_step`, the branches of one advance call, the whole
manoeuvre on the host executor with the oracle port, and what a free-end-time batch refuses."""
import numpy as np
import pytest

import free_t_cases as ftc
from free_t_cases import UPDATE_TIME as UT, SAMPLE_TIME as ST


def _single_entry_tables(basis, n_cols=2):
    from omgtools.batch import free_t_basis_tables
    fit, proj = free_t_basis_tables(basis)
    L = len(basis)
    return dict(o_T=n_cols * L, coeff_off=0, n_spl=n_cols, degree=basis.degree, knots=np.asarray(basis.knots), p_off=[], p_t=-1, update_time=UT,
                entries=[(0, L, n_cols, 0)], bases=[dict(degree=basis.degree, knots=np.asarray(basis.knots), fit=fit, proj=proj)])


@pytest.mark.parametrize('degree,intervals', [(3, 5), (3, 10), (3, 11), (1, 5), (1, 10), (2, 7)])
def test_twin_is_the_reference_shift(degree, intervals):
    """`free_t_advance_numpy` against `shift_spline_T(basis, s) @ c` (the reference's `shift_spline`, `basics/spline_extra.py:88-99`)
    to 1e-12 max(1, |c|) (measured 4e-15), and T afterwards against `FreeTPoint2point.init_step`'s statements."""
    from omgtools.batch import free_t_advance_numpy
    from omgtools.splines import BSplineBasis, shift_spline_T
    basis = BSplineBasis(np.r_[np.zeros(degree), np.linspace(0., 1., intervals + 1), np.ones(degree)], degree)
    ft = _single_entry_tables(basis)
    L, rng, worst = len(basis), np.random.default_rng(degree * 100 + intervals), 0.0
    for s in (1e-3, 0.0101, 0.05, 0.2, 0.49, 0.9):
        T = UT * (1.0 + 1.0 / s)                         # (T >= 2 update_time: s = update_time / (T - update_time))
        c = rng.normal(0., 2., (2, L))
        x = np.r_[c.reshape(-1), T][None, :].copy()
        free_t_advance_numpy(x, np.zeros((1, 1)), None, UT, ft)
        s_made = UT / (T - UT)
        want = (shift_spline_T(basis, s_made) @ c.T).T
        err = np.abs(x[0, :2 * L].reshape(2, L) - want).max()
        worst = max(worst, err / max(1.0, np.abs(c).max()))
        assert x[0, -1] == T - UT and abs(s_made - s) < 1e-12
    print('largest deviation from shift_spline_T, relative: %.2e' % worst)
    assert worst < 1e-12
    # the shortened update: T < 2 update_time keeps T and moves by T - update_time
    T = 0.16
    c = rng.normal(0., 2., (2, L))
    x = np.r_[c.reshape(-1), T][None, :].copy()
    free_t_advance_numpy(x, np.zeros((1, 1)), None, UT, ft)
    want = (shift_spline_T(basis, (T - UT) / T) @ c.T).T
    assert x[0, -1] == T and np.abs(x[0, :2 * L].reshape(2, L) - want).max() < 1e-12 * max(1.0, np.abs(c).max())


def test_twin_equals_init_step_of_the_problem_class():
    """One advance of the twin on the template's own layout against `FreeTPoint2point.init_step` on the same variables: the five
    entries on two bases, and T."""
    from omgtools.batch import free_t_advance_numpy
    problem, P = ftc.batch()
    ft, m = ftc.tables(problem, P)
    assert len(ft['entries']) == 5 and len(ft['bases']) == 2 and m.tpl.n_var == 53 and m.tpl.n_con == 193 and m.tpl.n_par == 26
    father, tpl = problem.father, m.tpl
    for T in (10., 0.15):
        x, p = ftc.random_plans(ft, tpl, np.array([T]))
        father._var_result = dict((key, x[0, lo:lo + r * c].reshape(c, r).T.copy()) for key, (lo, r, c) in tpl.var_layout.items())
        problem.start_time = 0.
        problem.init_step(1.0, UT)
        free_t_advance_numpy(x, p, None, UT, ft)
        for key, (lo, r, c) in tpl.var_layout.items():
            got, want = x[0, lo:lo + r * c].reshape(c, r).T, np.asarray(father._var_result[key]).reshape(r, c)
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), key


def test_twin_replays_the_reference_run():
    """With the tables the reference itself used at every update (its collocation points, the inverse of its collocation matrix), the
    twin's x after advance is the x0 the reference's solver was called with, its p the state0 / input0 / t of that call, and its log
    the reference's `vehicle.signals` -- both branches of `init_step` and the shortened last update included."""
    from omgtools.batch import free_t_advance_numpy, free_t_append_numpy
    g = ftc.reference_run()
    problem, P = ftc.batch()
    ft, m = ftc.tables(problem, P)
    tpl = m.tpl
    assert sorted((int(o), int(r), int(c)) for _, o, r, c in g['var_layout']) == sorted(tpl.var_layout.values())
    assert sorted((int(o), int(r), int(c)) for _, o, r, c in g['par_layout']) == sorted(tpl.par_layout.values())
    ut, st = float(g['update_time']), float(g['sample_time'])
    assert (ut, st) == (UT, ST)
    N = len(g['plans'])
    log, count, over = np.zeros((1, 3, 2, 80)), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    branches = set()
    for u in range(N):
        x = g['plans'][u][None, :].copy()
        free_t_append_numpy(x, None, log, count, over, ft, 10, st)      # (`Problem.simulate` of the plan just returned)
        if u + 1 == N:
            break
        T = x[0, ft['o_T']]
        branches.add(bool(T < 2 * ut))
        s = (T - ut) / T if T < 2 * ut else ut / (T - ut)
        assert abs(s - float(g['s_%d' % (u + 1)])) < 1e-12
        p = g['p'][u][None, :].copy()
        free_t_advance_numpy(x, p, None, ut, ftc.reference_tables(g, ft, u + 1))
        ftc.check_against_reference_x0(ft, g['plans'][u], x[0], g['x0'][u + 1])
        p_ref = g['p'][u + 1]
        for o in (m.o_state0, m.o_input0):
            assert np.abs(p[0, o:o + 2] - p_ref[o:o + 2]).max() <= 1e-12 * max(1.0, np.abs(p_ref[o:o + 2]).max()), (u, o)
        assert p[0, m.o_t] == 0. and p_ref[m.o_t] == 0.
    assert branches == {False, True}
    n = g['state'].shape[1]
    assert count[0] == n == 1 + 6 * 10 + 5 and not over[0]           # (the last plan has T = 0.055: five samples)
    for o, nm in enumerate(('state', 'input')):
        assert np.abs(log[0, o, :, :n] - g[nm]).max() <= 1e-12 * max(1.0, np.abs(g[nm]).max()), nm
    assert np.abs(g['time'][0] - np.arange(n) * st).max() < 1e-9


def test_branches_of_one_advance_call():
    """T in {10, 0.25, 0.15, 0.1, 0.05, NaN, 0.2} and a masked agent: flags, the rows that stay untouched, the prediction, T."""
    from omgtools.batch import free_t_advance_numpy
    problem, P = ftc.batch()
    ft, m = ftc.tables(problem, P)
    x0, p0 = ftc.random_plans(ft, m.tpl, ftc.BRANCH_T)
    x, p = x0.copy(), p0.copy()
    flags = np.ones(8, dtype=np.int32)
    flags[ftc.MASKED] = 0
    free_t_advance_numpy(x, p, flags, UT, ft)
    assert list(flags) == [1, 1, 1, 1, 0, 0, 0, 1]
    for b in (4, 5, 6):                                      # (stopped by the clause, masked, NaN: nothing is touched)
        assert np.array_equal(x[b], x0[b], equal_nan=True) and np.array_equal(p[b], p0[b])
    T_after = x[:, ft['o_T']]
    assert T_after[0] == 10. - UT and T_after[1] == 0.25 - UT and T_after[2] == 0.15 and T_after[3] == 0.1 and T_after[7] == 0.2 - UT
    rest = np.setdiff1d(np.arange(m.tpl.n_var), ftc.written_columns(ft))
    assert np.array_equal(x[:, rest], x0[:, rest], equal_nan=True)      # (this template has none: its variables are the five entries and T)
    L = m.L
    for b in (0, 1, 2, 3, 7):
        c = x0[b, m.o_spl:m.o_spl + 2 * L].reshape(2, L)
        T = ftc.BRANCH_T[b]
        assert np.allclose(p[b, m.o_state0:m.o_state0 + 2], m.basis.eval_basis([UT / T])[0] @ c.T, rtol=0, atol=1e-12 * max(1, np.abs(c).max()))
        db, Pm = m.basis.derivative(1)
        want = db.eval_basis([UT / T])[0] @ Pm @ c.T / T
        assert np.allclose(p[b, m.o_input0:m.o_input0 + 2], want, rtol=0, atol=1e-12 * max(1, np.abs(want).max()))
        assert p[b, m.o_t] == 0.
        others = np.setdiff1d(np.arange(m.tpl.n_par), [m.o_state0, m.o_state0 + 1, m.o_input0, m.o_input0 + 1, m.o_t])
        assert np.array_equal(p[b, others], p0[b, others])
    # T = 0.1: dt = 0, the plan is projected onto its own basis -- unchanged to rounding; T = 0.2: s = 1, every sample is the end value
    for off, rows, cols, _ in ft['entries']:
        assert np.abs(x[3, off:off + rows * cols] - x0[3, off:off + rows * cols]).max() < 1e-12 * np.abs(x0[3]).max()
        blk, old = x[7, off:off + rows * cols].reshape(cols, rows), x0[7, off:off + rows * cols].reshape(cols, rows)
        assert np.abs(blk - old[:, -1:]).max() < 1e-12 * np.abs(old).max()
    # without flags: every agent, and the stop clause touches nothing
    x, p = x0.copy(), p0.copy()
    free_t_advance_numpy(x, p, None, UT, ft)
    assert np.array_equal(x[4], x0[4]) and x[5, ft['o_T']] == 10. - UT


def test_append_partial_zero_and_overflowing():
    """n_b of `omgx_batch_free_t_append`: a whole update, what is left of the plan (floor(T / sample_time + 5e-7)), nothing; an
    append that does not fit writes nothing but the overflow flag; a masked agent is skipped."""
    from omgtools.batch import free_t_append_numpy, spline_der_numpy
    problem, P = ftc.batch()
    ft, m = ftc.tables(problem, P)
    T = np.array([10., 0.1, 0.0999, 0.0349999999, 0.01, 0.00999, np.nan, 3.0])
    x, _ = ftc.random_plans(ft, m.tpl, T)
    cap = 25
    log, count, over = np.full((8, 3, 2, cap), 7.0), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    flags = np.ones(8, dtype=np.int32)
    flags[7] = 0
    free_t_append_numpy(x, flags, log, count, over, ft, 10, ST)
    assert list(count) == [11, 11, 10, 4, 2, 0, 0, 0] and not over.any()
    L = m.L
    for b in range(5):
        c = x[b, m.o_spl:m.o_spl + 2 * L].reshape(2, L)
        n = count[b]
        u = np.arange(n) * ST / T[b]
        for o in range(3):
            want = spline_der_numpy(c, m.basis.knots, 3, u, o) / T[b] ** o
            assert np.allclose(log[b, o, :, :n], want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))
        assert (log[b, :, :, n:] == 7.0).all()
    assert (log[5:] == 7.0).all()
    before = log.copy()
    free_t_append_numpy(x, flags, log, count, over, ft, 10, ST)      # (the second append: no column 0)
    assert list(count) == [21, 21, 19, 7, 3, 0, 0, 0] and not over.any()
    assert np.array_equal(log[0, :, :, :11], before[0, :, :, :11])
    free_t_append_numpy(x, flags, log, count, over, ft, 10, ST)      # (agents 0 and 1 do not fit: 21 + 10 > 25)
    assert list(count) == [21, 21, 19, 10, 4, 0, 0, 0] and list(over) == [1, 1, 1, 0, 0, 0, 0, 0]


def test_whole_manoeuvre_on_the_host_executor():
    """`HostP2P` with the oracle port on `holonomic_free_t_p2p(8, knot_intervals=5)` (seed 20240814, the builder's default), with the
    stop rule and the log: every agent arrives; the motion time is the elapsed time, bounded below by the velocity limit."""
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = ftc.batch()
    m = BatchP2P(problem, P, ops=port_binding, options=dict(tol=1e-3, max_iter=300), update_time=UT)
    m.stop_at_arrival()
    m.record_signals(sample_time=ST)
    m.solve_cold()
    assert (m.status == 0).all()
    steps, T_prev = 0, m.horizon()
    while m.under_way.any() and steps < 150:
        run = m.under_way.copy()
        assert m.step() is False
        steps += 1
        assert (m.status[m.under_way] == 0).all()
        T_now = m.horizon()
        assert (T_now[run] <= T_prev[run] + 1e-9).all()
        T_prev = T_now
    assert not m.under_way.any(), (steps, m.under_way)
    assert abs(m.time - steps * UT) < 1e-9
    sig = m.signals()
    assert not sig['overflow'].any()
    ftc.check_manoeuvre(m.summary(), P['p'], m.p, m.o_state0, m._o_pose('test'), sig['count'])
    assert np.abs(sig['input'][0, :, :sig['count'][0]]).max() <= 0.5 + 1e-3


def test_refusals():
    from omgtools.batch import BatchP2P, free_t_basis_tables
    from omgtools.splines import BSplineBasis
    from omgtools import workloads as wl
    problem, P = ftc.batch()
    m = BatchP2P(problem, P, ops=object(), update_time=UT)
    for call in (lambda: m.rollout(3), lambda: m.plant(), lambda: m.feedback(), lambda: m.mission(np.zeros((8, 1, 2))),
                 lambda: m.step(states=np.zeros((8, 2)))):
        with pytest.raises(NotImplementedError, match='inv_T'):
            call()
    with pytest.raises(RuntimeError):
        BatchP2P(*ftc.batch(), ops=object()).summary()
    # a basis whose knots are not equidistant has no constant table
    uneven = BSplineBasis(np.r_[np.zeros(3), [0., 0.1, 0.3, 0.6, 1.0], np.ones(3)], 3)
    with pytest.raises(NotImplementedError, match='equidistant'):
        free_t_basis_tables(uneven)
    father = problem.father
    real = father.shifted_entries
    father.shifted_entries = lambda *a, **kw: [(lbl, nm, dict(spl, basis=uneven if spl['basis'].degree == 3 else spl['basis'])) for lbl, nm, spl in real(*a, **kw)]
    try:
        with pytest.raises(NotImplementedError, match='equidistant'):
            BatchP2P(problem, P, ops=object())
    finally:
        del father.shifted_entries
    # a problem loaded from a bundle brings no bases for the shift
    veh = problem.vehicles[0]
    meta = dict(problem_label=problem.label, horizon_time=10., knot_time=1., obstacle_labels=[o.label for o in problem.environment.obstacles],
                vehicle=dict(label=veh.label, knots=list(veh.basis.knots), degree=3, n_dim=2, n_spl=2), shifted=dict(seg=[], every=[]),
                dual_perm=list(range(father.template.n_con)))
    with pytest.raises(NotImplementedError, match='bundle'):
        BatchP2P(wl.ProblemView(meta, father.template), P, ops=object())
