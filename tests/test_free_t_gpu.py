"""Free end time in the device-resident loop: `omgx_batch_free_t_advance` / `_append` against their numpy twins on random plans and
every branch of a call, the refusals of `omgx_batch_set_free_t`, the device loop against the host executor with the oracle port, and
the whole manoeuvre on the device -- as one batch and through the streamed product path."""
import ctypes as C

import numpy as np
import pytest

import free_t_cases as ftc
from free_t_cases import UPDATE_TIME as UT, SAMPLE_TIME as ST

pytestmark = pytest.mark.gpu


def _solver(problem, P, ft):
    import omgtools.backend as be
    solver = be.BatchSolver(problem.father.template, P['p'].shape[0], options=dict(tol=1e-3, max_iter=50))
    solver.set_free_t(ft)
    return solver


def _close(a, b, what):
    """|a - b| <= 1e-12 max(1, |value|) entry by entry; returns the largest deviation in that unit."""
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(a)
    rel = np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok]))
    worst = float(rel.max()) if rel.size else 0.0
    assert worst <= 1e-12, (what, worst)
    return worst


@pytest.mark.parametrize('knot_intervals', [5, 10, 15])      # (n_fit of the vehicle's basis 25, 50 and 75: within a wave, and across one)
def test_advance_and_append_equal_their_twins(knot_intervals):
    import torch
    from omgtools.batch import free_t_advance_numpy, free_t_append_numpy
    problem, P = ftc.batch(8, knot_intervals)
    ft, m = ftc.tables(problem, P)
    assert len(ft['bases'][0]['fit']) == 5 * knot_intervals
    tpl, dev = m.tpl, torch.device('cuda', 0)
    solver = _solver(problem, P, ft)
    try:
        x0, p0 = ftc.random_plans(ft, tpl, ftc.BRANCH_T, seed=knot_intervals)
        flags0 = np.ones(8, dtype=np.int32)
        flags0[ftc.MASKED] = 0
        xr, pr, fr = x0.copy(), p0.copy(), flags0.copy()
        free_t_advance_numpy(xr, pr, fr, UT, ft)
        runs = []
        for _ in range(2):
            x, p = torch.as_tensor(x0, device=dev), torch.as_tensor(p0, device=dev)
            flags = torch.as_tensor(flags0, device=dev)
            solver.free_t_advance(x, p, UT, under_way=flags)
            runs.append((x.cpu().numpy(), p.cpu().numpy(), flags.cpu().numpy()))
        (xg, pg, fg), again = runs
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(runs[0], again)), 'two runs must give the same bits'
        assert np.array_equal(fg, fr) and list(fg) == [1, 1, 1, 1, 0, 0, 0, 1]
        worst = max(_close(xg, xr, 'x'), _close(pg, pr, 'p'))
        for b in (4, 5, 6):                                  # (the stop clause, the masked agent, the NaN: their bits stay)
            assert np.array_equal(xg[b], x0[b], equal_nan=True) and np.array_equal(pg[b], p0[b])
        rest_x = np.setdiff1d(np.arange(tpl.n_var), ftc.written_columns(ft))
        rest_p = np.setdiff1d(np.arange(tpl.n_par), [m.o_state0, m.o_state0 + 1, m.o_input0, m.o_input0 + 1, m.o_t])
        assert np.array_equal(xg[:, rest_x], x0[:, rest_x], equal_nan=True) and np.array_equal(pg[:, rest_p], p0[:, rest_p])
        # without flags: every agent
        x, p = torch.as_tensor(x0, device=dev), torch.as_tensor(p0, device=dev)
        solver.free_t_advance(x, p, UT)
        xr2, pr2 = x0.copy(), p0.copy()
        free_t_advance_numpy(xr2, pr2, None, UT, ft)
        worst = max(worst, _close(x.cpu().numpy(), xr2, 'x, no flags'), _close(p.cpu().numpy(), pr2, 'p, no flags'))
        # the append: a whole update, partial, none, overflowing, masked
        T = np.array([10., 0.1, 0.0999, 0.0349999999, 0.01, 0.00999, np.nan, 3.0])
        xa, _ = ftc.random_plans(ft, tpl, T, seed=11)
        flags0 = np.ones(8, dtype=np.int32)
        flags0[7] = 0
        cap = 25
        lr, cr, orr = np.full((8, 3, 2, cap), 7.0), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
        lg, cg, og = (torch.as_tensor(a.copy(), device=dev) for a in (lr, cr, orr))
        xd, fd = torch.as_tensor(xa, device=dev), torch.as_tensor(flags0, device=dev)
        plan = dict(coeff_off=m.o_spl, n_spl=2, degree=3, knots=m.basis.knots, n_samp=10, sample_time=ST)
        for k in range(3):
            free_t_append_numpy(xa, flags0, lr, cr, orr, ft, 10, ST)
            solver.free_t_append(xd, lg, cg, og, under_way=fd, **plan)
            assert np.array_equal(cg.cpu().numpy(), cr) and np.array_equal(og.cpu().numpy(), orr), k
            worst = max(worst, _close(lg.cpu().numpy(), lr, 'log'))
        assert list(cr) == [21, 21, 19, 10, 4, 0, 0, 0] and list(orr) == [1, 1, 1, 0, 0, 0, 0, 0]
        print('device against twin, knot_intervals %d: largest deviation %.2e (unit: max(1, |value|))' % (knot_intervals, worst))
    finally:
        solver.close()


def test_advance_takes_the_callers_own_tables():
    """The library applies whatever (fit, proj) a basis is registered with: here square collocation tables in the shape of the
    reference's own `BSplineBasis.transform` (`basics/spline.py:283-306`: as many points as coefficients, the inverse of the collocation
    matrix) at the Greville points, registered over the least-squares tables of the same handle."""
    import torch
    from omgtools.batch import free_t_advance_numpy
    from omgtools.splines import BSplineBasis
    problem, P = ftc.batch()
    ft, m = ftc.tables(problem, P)
    bases = []
    for bs in ft['bases']:
        basis = BSplineBasis(bs['knots'], bs['degree'])
        fit = np.asarray(basis.greville(), dtype=float)
        bases.append(dict(bs, fit=fit, proj=np.ascontiguousarray(np.linalg.inv(basis.eval_basis(fit)))))
    ft2 = dict(ft, bases=bases)
    solver = _solver(problem, P, ft)
    try:
        solver.set_free_t(ft2)
        x0, p0 = ftc.random_plans(ft, m.tpl, ftc.BRANCH_T, seed=21)
        xr, pr = x0.copy(), p0.copy()
        free_t_advance_numpy(xr, pr, None, UT, ft2)
        x, p = torch.as_tensor(x0, device='cuda'), torch.as_tensor(p0, device='cuda')
        solver.free_t_advance(x, p, UT)
        _close(x.cpu().numpy(), xr, 'x')
        _close(p.cpu().numpy(), pr, 'p')
        # (collocation interpolates: at T = update_time, dt = 0, the plan comes back to rounding)
        assert np.abs(xr[3] - x0[3]).max() < 1e-12 * np.abs(x0[3]).max()
    finally:
        solver.close()


def test_advance_with_the_reference_tables_hands_the_solver_the_reference_x0():
    """The tables the reference itself used (tests/golden/free_t_holonomic.npz), registered with the handle: the device's x after
    advance is the twin's to 1e-12 and the x0 the reference's solver was called with, on both branches of `init_step`."""
    import torch
    from omgtools.batch import free_t_advance_numpy
    g = ftc.reference_run()
    problem, P = ftc.batch()
    ft, m = ftc.tables(problem, P)
    solver = _solver(problem, P, ft)
    try:
        for u in (1, 5, 6):                                  # (T = 10; 0.25; 0.15 < 2 update_time)
            ft_u = ftc.reference_tables(g, ft, u)
            solver.set_free_t(ft_u)
            x0, p0 = np.tile(g['plans'][u - 1], (8, 1)), np.tile(g['p'][u - 1], (8, 1))
            xr, pr = x0.copy(), p0.copy()
            free_t_advance_numpy(xr, pr, None, UT, ft_u)
            x, p = torch.as_tensor(x0, device='cuda'), torch.as_tensor(p0, device='cuda')
            solver.free_t_advance(x, p, UT)
            xg, pg = x.cpu().numpy(), p.cpu().numpy()
            _close(xg, xr, 'x')
            _close(pg, pr, 'p')
            assert (xg == xg[0]).all()
            ftc.check_against_reference_x0(ft, g['plans'][u - 1], xg[0], g['x0'][u])
            for o in (m.o_state0, m.o_input0):
                assert np.abs(pg[0, o:o + 2] - g['p'][u][o:o + 2]).max() <= 1e-12 * max(1.0, np.abs(g['p'][u][o:o + 2]).max())
    finally:
        solver.close()


def test_set_free_t_refuses_what_it_cannot_carry():
    import omgtools.backend as be
    problem, P = ftc.batch()
    ft, m = ftc.tables(problem, P)
    tpl = m.tpl
    solver = be.BatchSolver(tpl, 8, options=dict(tol=1e-3, max_iter=50))

    def refused(match, **change):
        spec = dict(ft, **change)
        with pytest.raises(be.OmgxError, match=match) as e:
            solver.set_free_t(spec)
        assert '(-1)' in str(e.value)                        # OMGX_E_INVALID

    def basis0(**change):
        return [dict(ft['bases'][0], **change)] + ft['bases'][1:]
    try:
        import torch
        x, p = torch.zeros((8, tpl.n_var), dtype=torch.float64, device='cuda'), torch.zeros((8, tpl.n_par), dtype=torch.float64, device='cuda')
        with pytest.raises(be.OmgxError, match='no free-end-time glue is set'):
            solver.free_t_advance(x, p, UT)
        refused('o_T = %d outside x' % tpl.n_var, o_T=tpl.n_var)
        refused('o_T = -1', o_T=-1)
        refused(r'entries\[1\]: offset', entries=[ft['entries'][0], (tpl.n_var - 3, 6, 2, 1)])
        refused('n_ent = 33', entries=[ft['entries'][0]] * 33)
        refused('n_basis = 5', bases=ft['bases'] + [ft['bases'][1]] * 3)
        refused(r'basis\[0\]: n_fit = 257', bases=basis0(fit=np.linspace(0., 1., 257), proj=np.zeros((8, 257))))
        big = np.r_[np.zeros(1), np.linspace(0., 1., 38), np.ones(1)]            # (degree 1, 40 knots: 38 rows -- allowed)
        solver.set_free_t(dict(ft, bases=ft['bases'] + [dict(degree=1, knots=big, fit=np.linspace(0., 1., 4), proj=np.zeros((38, 4)))]))
        refused(r'entries\[0\]: rows = 65', entries=[(0, 65, 1, 0)])
        refused(r'entries\[0\]: rows = 7, its basis has 8', entries=[(0, 7, 2, 0)])
        refused(r'basis\[0\]: n_knots = 41', bases=basis0(knots=np.r_[np.zeros(3), np.linspace(0., 1., 35), np.ones(3)], proj=np.zeros((37, 25))))
        refused('update_time = 0 must be positive', update_time=0.0)
        refused('update_time = -0.1 must be positive', update_time=-0.1)
        refused(r'p_off\[1\] = %d outside p' % (tpl.n_par - 1), p_off=[m.o_state0, tpl.n_par - 1])
        # null tables, through the C interface itself
        sp = be.CFreeTSpec()
        assert solver.lib.omgx_batch_set_free_t(solver._h, C.byref(sp)) == -1 and b'null p_off / entries / basis' in solver.lib.omgx_last_error()
        kn = np.ascontiguousarray(m.basis.knots, dtype=np.float64)
        off, ent = np.array([m.o_state0, m.o_input0], dtype=np.int32), np.array([[0, 8, 2, 0]], dtype=np.int32)
        bs = (be.CFreeTBasis * 1)(be.CFreeTBasis(3, len(kn), 25, kn.ctypes.data, None, None))
        sp = be.CFreeTSpec(kn.ctypes.data, 0, 2, 3, len(kn), ft['o_T'], 2, off.ctypes.data, m.o_t, UT, 1, ent.ctypes.data, 1, C.addressof(bs))
        assert solver.lib.omgx_batch_set_free_t(solver._h, C.byref(sp)) == -1 and b'basis[0]: null knots / fit / proj' in solver.lib.omgx_last_error()
        # a registration refused for its arguments changes nothing (the one before it stands); NULL switches the glue off
        solver.set_free_t(ft)
        with pytest.raises(be.OmgxError, match='update_time = 0 must be positive'):
            solver.free_t_advance(x, p, 0.0)
        solver.set_free_t(None)
        with pytest.raises(be.OmgxError, match='no free-end-time glue is set'):
            solver.free_t_advance(x, p, UT)
    finally:
        solver.close()


def test_device_loop_replays_the_host_executor():
    """Cold solve and 12 steps at tol 1e-5 on the device and on the host executor with the oracle port (the pattern and the
    tolerances of tests/test_gpu_batch_mpc.py::test_mpc_replay_matches_port)."""
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    from oracle.nlp_numpy import NumpyNLP
    problem, P = ftc.batch()
    tpl = problem.father.template
    nlp = NumpyNLP(tpl)
    opts = dict(tol=1e-5, max_iter=300)
    gpu = BatchP2P(problem, P, ops='hip', options=opts, max_iter_step=300, update_time=UT)
    cpu = BatchP2P(problem, P, ops=port_binding, options=opts, max_iter_step=300, update_time=UT)
    try:
        for m in (gpu, cpu):
            m.stop_at_arrival()
            m.solve_cold()
        o_T = gpu._ft['o_T']
        ok = (gpu.host('status') == 0) & (cpu.status == 0)
        assert ok.sum() >= 4
        for k in range(13):
            if k:
                assert gpu.step() is False and cpu.step() is False
            sg, sc = gpu.host('status'), cpu.status
            assert np.array_equal(sg, sc), k
            ok = ok & (sg == 0)
            assert ok.sum() >= 3
            assert np.array_equal(gpu.host('under_way') != 0, cpu.under_way) and cpu.under_way.all()
            pg, pc, xg = gpu.host('p'), cpu.p, gpu.host('x')
            s0, i0 = gpu.o_state0, gpu.o_input0
            assert np.abs(pg[ok, s0:s0 + 2] - pc[ok, s0:s0 + 2]).max() < 2e-4
            assert np.abs(pg[ok, i0:i0 + 2] - pc[ok, i0:i0 + 2]).max() < 2e-3
            assert (np.abs(xg[ok, o_T] - cpu.x[ok, o_T]) < 1e-4 * (1 + np.abs(cpu.x[ok, o_T]))).all()      # (the objective is T)
            for b in np.nonzero(ok)[0][:3]:
                fg_, gg_ = nlp.fg(xg[b], nlp.term_coefs(pg[b]))
                fc_, gc_ = nlp.fg(cpu.x[b], nlp.term_coefs(pc[b]))
                assert abs(fg_ - fc_) < 1e-4 * (1 + abs(fc_))
                assert (gg_ - tpl.ub).max() < 1e-5 and (tpl.lb - gg_).max() < 1e-5
                assert (gc_ - tpl.ub).max() < 1e-5 and (tpl.lb - gc_).max() < 1e-5
        assert abs(gpu.time - 12 * UT) < 1e-9
    finally:
        gpu.solver.close()


def test_whole_manoeuvre_on_the_device():
    """The batch of the CPU run at tol 1e-3, stop rule and log on: every agent arrives and meets the conditions of the host run, its
    flag clears within two updates of the host run's, its horizon never grows; through `StreamedP2P` the same bits."""
    from omgtools.batch import BatchP2P, StreamedP2P
    from oracle import port_binding
    problem, P = ftc.batch()
    opts = dict(tol=1e-3, max_iter=300)

    def run(m, dev):
        m.stop_at_arrival()
        m.record_signals(sample_time=ST)
        m.solve_cold()
        ended = np.full(8, -1)
        T_prev = np.asarray(m.horizon().cpu() if dev else m.horizon())
        for k in range(1, 151):
            m.step()
            uw = (m.under_way.cpu().numpy() if dev else m.under_way) != 0
            st = m.status.cpu().numpy() if dev else m.status
            assert (st[uw] == 0).all(), k
            T_now = np.asarray(m.horizon().cpu() if dev else m.horizon())
            assert (T_now <= T_prev + 1e-9).all(), k
            T_prev = T_now
            ended[(ended < 0) & ~uw] = k
            if not uw.any():
                break
        assert (ended > 0).all(), ended
        return ended

    host = BatchP2P(problem, P, ops=port_binding, options=opts, update_time=UT)
    ended_host = run(host, False)
    one = BatchP2P(problem, P, ops='hip', options=opts, update_time=UT)
    parts = StreamedP2P(problem, P, n_streams=2, options=opts, update_time=UT)
    try:
        ended = run(one, True)
        assert np.abs(ended - ended_host).max() <= 2, (ended, ended_host)
        sig = one.signals()
        count = sig['count'].cpu().numpy()
        assert not sig['overflow'].cpu().numpy().any()
        ftc.check_manoeuvre(one.summary().cpu().numpy(), P['p'], one.host('p'), one.o_state0, one._o_pose('test'), count)
        assert np.array_equal(run(parts, True), ended)
        for name in ('x', 'p', 'lam', 'status'):
            assert np.array_equal(getattr(parts, name).cpu().numpy(), one.host(name)), name
        sp = parts.signals()
        assert np.array_equal(sp['count'].cpu().numpy(), count)
        for b in range(8):
            assert np.array_equal(sp['splines'][b, :, :, :count[b]].cpu().numpy(), sig['splines'][b, :, :, :count[b]].cpu().numpy())
    finally:
        one.solver.close()
        parts.close()
