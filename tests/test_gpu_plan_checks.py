"""The part of the plan rule (include/omgx.h, above omgx_store_spec) that needs a handle: every plan-taking glue entry refuses a plan
that reaches outside x, and the three entries that used to let a knot vector shorter than 2 * degree + 2 through refuse it -- all
ahead of any launch --, and the handle that refused them works on as a fresh one does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 4


def _loop():
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = workloads.holonomic_p2p(B)
    return BatchP2P(problem, P, ops='hip', device=torch.device('cuda', 0), options=dict(tol=1e-3, max_iter=300))


def _plan(m):
    return dict(coeff_off=m.o_spl, n_spl=m.n_spl, degree=m.basis.degree, knots=np.asarray(m.basis.knots), inv_T=1.0 / m.T)


def _cold_predict_rollout(m):
    import torch
    m.solve_cold(bends=())
    m.solver.predict_ex(m.x, m.p, tau=0.01, p_off=m.p_offs, p_t=m.o_t, t_value=0.1, **_plan(m))
    m.rollout(1)
    torch.cuda.synchronize()
    return dict((k, getattr(m, k).cpu().numpy()) for k in ('x', 'lam', 'p', 'status', 'iters'))


def test_a_plan_outside_x_or_on_too_few_knots_is_refused_before_any_launch():
    import torch
    from omgtools.backend import OmgxError
    m = _loop()
    s, tpl, n_spl, deg = m.solver, m.tpl, m.n_spl, m.basis.degree
    f64, i32 = dict(dtype=torch.float64, device=m.dev), dict(dtype=torch.int32, device=m.dev)
    n_samp, cap = 10, 21
    out, t0 = torch.zeros((B, 2, n_spl, 5), **f64), torch.zeros(B, **f64)
    log, count = torch.zeros((B, 3, n_spl, cap), **f64), torch.zeros(B, **i32)
    vec = dict((nm, torch.zeros((B, n_spl), **f64)) for nm in ('state', 'state_prev', 'input_last'))
    state5, summary, n_upd = torch.zeros((B, 5), **f64), torch.zeros((B, 8), **f64), torch.zeros(B, **i32)
    o_pose = tpl.entry_range(m.veh.label, 'poseT', 'par')[0]
    clock = ([0.01], [0.1], [0])                             # tau, t_rel, crossed of one rollout step

    def entries(plan):
        """name -> call of every plan-taking entry with that plan"""
        sig = dict(plan, n_samp=n_samp, p_t=m.o_t, sample_time=0.01)
        plant = dict(plan, dist=None, n_upd=n_upd, overflow=None, under_way=None, n_samp=n_samp, max_updates=2, p_t=m.o_t, p_state0=m.o_state0,
                     p_input0=m.o_input0, p_poseT=o_pose, sample_time=0.01, stop_tol=1e-3, **vec)
        flat = (plan['coeff_off'], plan['n_spl'], plan['degree'], plan['knots'])
        return {
            'sample': lambda: s.sample(m.x, *flat, 2, t0, 0.01, 5, out=out, device=True),
            'store': lambda: s.store(m.x, out, None, t0, *flat, 2, 5, 0.01, plan['inv_T']),
            'set_store': lambda: s.set_store(out, None, t0, *flat, 2, 5, 0.01, plan['inv_T']),
            'set_signals': lambda: s.set_signals(log, count, None, **sig),
            'signals_append': lambda: s.signals_append(m.x, m.p, log, count, None, **sig),
            'signals_reduce': lambda: s.signals_reduce(log, count, vec['state'], summary, **sig),
            'set_plant': lambda: s.set_plant(plant),
            'plant_simulate': lambda: s.plant_simulate(m.x, m.p, plant),
            'plant_predict': lambda: s.plant_predict(m.x, m.p, 0.01, 0.1, plant),
            'predict': lambda: s.predict(m.x, m.p, *flat, 0.01, plan['inv_T'], m.o_state0, m.o_input0, m.o_t, 0.1),
            'predict_ex': lambda: s.predict_ex(m.x, m.p, *flat, 0.01, plan['inv_T'], m.p_offs, m.o_t, 0.1),
            'predict_quadrotor': lambda: s.predict_quadrotor(m.x, m.p, plan['coeff_off'], plan['degree'], plan['knots'], 0.01, plan['inv_T'], m.p_offs, m.o_t,
                                                             0.1, state5, None, 1, 0.01),
            'rollout': lambda: s.rollout(m.p, m.x, m.lb, m.ub, m.lam, m.status, m.iters, *clock, *flat, plan['inv_T'], m.p_offs, m.o_t),
        }
    try:
        assert n_spl == 2 and deg >= 3                       # (what omgx_batch_predict_quadrotor reads: two splines of degree >= 3)
        outside = entries(dict(_plan(m), coeff_off=tpl.n_var - 1))
        assert len(outside) == 13
        for name, call in outside.items():
            with pytest.raises(OmgxError, match='outside x'):
                call()
        short = entries(dict(_plan(m), knots=_plan(m)['knots'][:2 * deg + 1]))
        for name in ('predict_ex', 'predict_quadrotor', 'rollout'):
            with pytest.raises(OmgxError, match='n_knots'):
                short[name]()
        got = _cold_predict_rollout(m)
    finally:
        s.close()
    fresh = _loop()
    try:
        ref = _cold_predict_rollout(fresh)
    finally:
        fresh.solver.close()
    assert (ref['iters'] > 0).all()
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
