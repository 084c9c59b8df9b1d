"""The instances of the wave-level factorisation (wave_ldl / wave_bwd, omg-tools_amd/csrc/omgx_wave.h) and the rule that picks
them per leaf (wave_leaf_small, used by kkt_factor_wave and kkt_solve_wave in omgx_core.h):

    banded leaf of order <= 36 and half bandwidth <= 5   ->  wave_ldl<36, 5, true, 2>, wave_bwd<36, true>
    other banded leaf of half bandwidth <= 8              ->  wave_ldl<40, 8, true, 2>, wave_bwd<40, true>
    the root (one vector row)                             ->  wave_ldl<40, 40, false, 1>

An instance that drops a live column, a band entry or the right-hand-side row, or a pivot test that lets a pivot of the wrong sign
pass (the cold solves start with such pivots: the inertia correction answers them, so a missed flag changes the iteration counts),
derails every iteration.  The device loop is therefore held against the host build of the same solver (oracle/port_binding), in the
pattern of tests/test_gpu_descriptor_image.py: a cold solve and three receding-horizon steps of 0.4 knot intervals, the third of
which crosses a knot.  Statuses and iteration counts are integers and must be equal; the plans agree to TOL_X_PORT = 1e-4 (kernel
and host build sum their reductions in different orders: rounding apart, not the same bits -- the bound of
tests/test_gpu_descriptor_image.py and tests/test_gpu_table_sharing.py).

Every case states from the plan (describe_plan: leaf_sizes, leaf_bw) which instance the rule above selects for its hyperplane
leaves, so that no case can silently run another path than the one it is there for."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)
N = 8
TOL_X_PORT = 1e-4
LDS_PER_CU = 160 * 1024            # MI355X: 160 KiB of LDS per compute unit

# (knot intervals, obstacles): order of the hyperplane leaves, the instance the rule selects (None: the plan leaves the wave path)
CASES = [
    pytest.param(11, 3, 36, 'small', id='k11_o3_headline_leaf36'),
    pytest.param(10, 3, 33, 'small', id='k10_o3_leaf33_not_multiple_of_four'),
    pytest.param(7, 1, 24, 'small', id='k7_o1_one_small_leaf'),
    pytest.param(11, 5, 36, 'small', id='k11_o5_more_leaves_than_waves'),
    pytest.param(12, 1, 39, 'wide', id='k12_o1_leaf39_falls_back'),
]


def _template_only(fn, *a, **kw):
    """A front-end builder called for its template (`Point2point.init` would create a solver object of its own)."""
    import omgtools.backend as be
    saved = be.create_nlp
    be.create_nlp = lambda tpl, opt, name='': (None, 0.)
    try:
        return fn(*a, **kw)
    finally:
        be.create_nlp = saved


def _instance(n, bw):
    """The documented rule (wave_leaf_small, omgx_wave.h)."""
    return 'small' if n <= 36 and bw <= 5 else ('wide' if bw <= 8 else 'dense')


def _loop(mpc, steps):
    host = (lambda n: getattr(mpc, n)) if mpc.kind == 'host' else mpc.host
    mpc.solve_cold(bends=())
    out, crossed = [(host('x').copy(), host('status').copy(), host('iters').copy())], 0
    for _ in range(steps):
        crossed += int(bool(mpc.step()))
        out.append((host('x').copy(), host('status').copy(), host('iters').copy()))
    return out, crossed


@pytest.mark.parametrize('knots, n_obs, leaf_order, instance', CASES)
def test_device_loop_matches_the_host_build(knots, n_obs, leaf_order, instance):
    import torch
    from omgtools import scenarios
    from omgtools.backend import describe_plan
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = _template_only(scenarios.holonomic_p2p, N, knot_intervals=knots, n_obs=n_obs)
    plan = describe_plan(problem.father.template)
    # the hyperplane leaves (one per obstacle, banded) come first, the sparse diagonal leaf of the terminal slacks last
    assert plan['n_leaf'] == n_obs + 1
    assert plan['leaf_sizes'][:n_obs] == [leaf_order] * n_obs, plan['leaf_sizes']
    assert plan['leaf_bw'][:n_obs] == [5] * n_obs and plan['leaf_bw'][n_obs] == 0, plan['leaf_bw']
    on_wave_path = bool(plan['wave_path'])
    if instance == 'small':
        assert on_wave_path, plan                           # (a case that is here for the small instances must run them)
    else:
        # leaf order 39: on the wave path it takes the <40, 8> instances; where its root (n_root + n_eq) has more than 40
        # columns the plan leaves the wave path altogether -- whichever the plan says, the loop below must match the host build
        assert on_wave_path == (plan['n_root'] + plan['n_eq'] <= 40), plan
    if on_wave_path:
        assert [_instance(n, bw) for n, bw in zip(plan['leaf_sizes'][:n_obs], plan['leaf_bw'][:n_obs])] == [instance] * n_obs
    if n_obs > 4:
        assert plan['n_leaf'] > 4                           # more leaves than the four waves of a half-CU workgroup: a second round
    update_time = 0.4 * float(problem.knot_time)            # steps at 0.4, 0.8, 1.2 knot intervals: the third crosses a knot
    ref = BatchP2P(problem, P, ops=port_binding, options=OPTS, update_time=update_time)
    ref.n_threads = 8
    want, crossed_ref = _loop(ref, 3)
    problem_g, P_g = _template_only(scenarios.holonomic_p2p, N, knot_intervals=knots, n_obs=n_obs)
    gpu = BatchP2P(problem_g, P_g, ops='hip', device=torch.device('cuda', 0), options=OPTS, update_time=update_time)
    try:
        info = gpu.solver.workspace()
        print('k %d, %d obstacles: leaves %s (bw %s), root %d + %d, wave path %d, mode %d, %d B of LDS'
              % (knots, n_obs, plan['leaf_sizes'], plan['leaf_bw'], plan['n_root'], plan['n_eq'], plan['wave_path'], info['mode'], info['lds_bytes']))
        assert info['mode'] == plan['ws_mode'] and info['lds_bytes'] == plan['lds_bytes'], (info, plan['ws_mode'], plan['lds_bytes'])
        if on_wave_path:
            assert info['mode'] in (0, 4, 5)
        if (knots, n_obs) == (11, 3):
            assert info['mode'] == 5 and 2 * info['lds_bytes'] <= LDS_PER_CU, info      # the headline class: two agents per CU
        got, crossed = _loop(gpu, 3)
    finally:
        gpu.solver.close()
    assert crossed == crossed_ref == 1
    lo, hi = gpu.tpl.entry_range(gpu.veh.label, 'splines_seg0', 'var')
    for k, ((x, st, it), (xr, st_r, it_r)) in enumerate(zip(got, want)):
        worst = float(np.abs(x[:, lo:hi] - xr[:, lo:hi]).max())
        print('%s: iters %s, max |coefficient diff| %.2e' % ('cold' if k == 0 else 'step %d' % k, it.tolist(), worst))
        assert np.array_equal(st, st_r), (k, st, st_r)
        assert np.array_equal(it, it_r), (k, it, it_r)
        assert worst < TOL_X_PORT, (k, worst)
