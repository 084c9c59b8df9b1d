"""The two forms of the Schur phase of the wave-path factorisation (kkt_factor_wave, omg-tools_amd/csrc/omgx_core.h) and the rule
that picks one per plan (HostPlan::schur_rule, omg-tools_amd/csrc/omgx_plan.h; reported by omgx_plan_schur_tiles):

    tile owners   wave 0, 1, 2 owns tile (0,0), (1,0), (1,1) of every banded leaf's S_l = W D^-1 W', subtracts them in leaf order
                  from a register copy of its root entries and stores once; the index tables come from LDS
    rounds        one leaf per barrier-separated round, index tables from global memory

Tile owners iff the plan is on the wave path, every banded leaf precedes the (one) diagonal leaf, all banded leaves have the identical
coupling row, coupling rows + the right-hand-side row fit two 16-row blocks (nc + 1 <= 32) and the workgroup has at least three waves
(256 or 512 threads: always, for the plans the library builds); the library adds that the tables must fit the free descriptor slots,
which a case notices as a report that contradicts the rule recomputed here.

A tile owner that drops a leaf, a row block, the right-hand-side row or the order of the subtractions derails every iteration, so the
device is held against the host build of the same solver (oracle/port_binding) in the pattern of tests/test_gpu_factor_instances.py:
a cold solve and three receding-horizon steps of 0.4 knot intervals, the third of which crosses a knot; statuses and iteration counts
equal, spline coefficients within that file's TOL_X_PORT = 1e-4.  The two ADMM bundles are held the same way over one x-update.

Every case first asserts which form its plan reports and that the report agrees with the rule recomputed from
oracle.plan_numpy.SolverPlan(tpl).cpl_ptr / cpl_idx: no case can silently run the other form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)
N = 8
TOL_X_PORT = 1e-4

# (knot intervals, obstacles): banded leaves formed by tile owners (0: rounds), coupling rows + the right-hand-side row
P2P_CASES = [
    pytest.param(11, 3, 3, 30, id='k11_o3_headline_second_row_block_partial'),
    pytest.param(11, 5, 5, 30, id='k11_o5_five_leaves_on_three_tile_waves'),
    pytest.param(7, 1, 1, 22, id='k7_o1_single_leaf'),
    pytest.param(4, 1, 1, 16, id='k4_o1_one_tile_waves_1_and_2_idle'),
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


def _rule(tpl, plan):
    """The rule recomputed: number of banded leaves formed by tile owners, 0 = rounds.  Leaf kinds from describe_plan (a diagonal leaf
    has half bandwidth 0), coupling rows from the numpy plan."""
    from oracle.plan_numpy import SolverPlan
    sp = SolverPlan(tpl)
    rows = [tuple(int(i) for i in sp.cpl_idx[sp.cpl_ptr[l]:sp.cpl_ptr[l + 1]]) for l in range(sp.n_leaf)]
    assert sp.n_leaf == plan['n_leaf'] and [len(r) for r in rows] == plan['leaf_cpl']
    banded = [bw > 0 for bw in plan['leaf_bw']]
    nb = sum(banded)
    if not plan['wave_path'] or nb == 0 or banded != [True] * nb + [False] * (plan['n_leaf'] - nb) or plan['n_leaf'] - nb > 1:
        return 0, rows
    if len(set(rows[:nb])) != 1 or len(rows[0]) + 1 > 32:
        return 0, rows
    return nb, rows


def _selected(tpl, want_tiles):
    """(plan, rule) after the two assertions every case starts with."""
    from omgtools.backend import describe_plan, plan_schur_tiles
    plan = describe_plan(tpl)
    reported = plan_schur_tiles(tpl)
    rule, rows = _rule(tpl, plan)
    print('leaves %s (bw %s), coupling rows %s, root %d + %d, wave path %d: reported %d, rule %d'
          % (plan['leaf_sizes'], plan['leaf_bw'], plan['leaf_cpl'], plan['n_root'], plan['n_eq'], plan['wave_path'], reported, rule))
    assert reported == want_tiles, (reported, want_tiles)
    assert reported == rule, (reported, rule, rows)
    return plan, rows


def _loop(mpc, steps):
    host = (lambda n: getattr(mpc, n)) if mpc.kind == 'host' else mpc.host
    mpc.solve_cold(bends=())
    out, crossed = [(host('x').copy(), host('status').copy(), host('iters').copy())], 0
    for _ in range(steps):
        crossed += int(bool(mpc.step()))
        out.append((host('x').copy(), host('status').copy(), host('iters').copy()))
    return out, crossed


@pytest.mark.parametrize('knots, n_obs, tiles, nc1', P2P_CASES)
def test_device_loop_matches_the_host_build(knots, n_obs, tiles, nc1):
    import torch
    from omgtools import scenarios
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = _template_only(scenarios.holonomic_p2p, N, knot_intervals=knots, n_obs=n_obs)
    plan, rows = _selected(problem.father.template, tiles)
    assert plan['n_leaf'] == n_obs + 1 and plan['leaf_cpl'][0] + 1 == nc1 == plan['n_root'] + 1, plan
    if nc1 <= 16:
        assert nc1 == 16                                    # the largest root that is one tile: one more knot interval adds two rows
    if n_obs > 3:
        assert tiles > 3                                    # more banded leaves than tile owners keep in flight: a second group
    update_time = 0.4 * float(problem.knot_time)            # steps at 0.4, 0.8, 1.2 knot intervals: the third crosses a knot
    ref = BatchP2P(problem, P, ops=port_binding, options=OPTS, update_time=update_time)
    ref.n_threads = 8
    want, crossed_ref = _loop(ref, 3)
    problem_g, P_g = _template_only(scenarios.holonomic_p2p, N, knot_intervals=knots, n_obs=n_obs)
    gpu = BatchP2P(problem_g, P_g, ops='hip', device=torch.device('cuda', 0), options=OPTS, update_time=update_time)
    try:
        info = gpu.solver.workspace()
        assert info['mode'] == plan['ws_mode'] and info['lds_bytes'] == plan['lds_bytes'], (info, plan['ws_mode'], plan['lds_bytes'])
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


# the ADMM bundles at 64 agents: banded leaves formed by tile owners, workspace mode, distinct coupling rows among the banded leaves
ADMM_CASES = [
    pytest.param('formation', 3, 4, 1, id='formation_64_tiles_mode_4'),
    pytest.param('rendezvous', 0, 0, 2, id='rendezvous_64_distinct_rows_rounds'),
]


@pytest.mark.parametrize('kind, tiles, mode, distinct', ADMM_CASES)
def test_x_update_matches_the_host_build(kind, tiles, mode, distinct):
    """The first x-update of the ADMM iteration (parameters as `BatchADMM.initialize` leaves them, the options of the existing ADMM
    tests) solved by the device and by the host build."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from admm_numpy_ops import NumpyAdmmOps
    from omgtools import workloads
    from omgtools.admm import BatchADMM
    from omgtools.backend import BatchSolver
    from oracle import port_binding
    n = 64
    rendezvous = kind == 'rendezvous'
    problem, updater, father, lay, P = (workloads.rendezvous_holonomic if rendezvous else workloads.formation_holonomic)(n)
    tpl = father.template
    plan, rows = _selected(tpl, tiles)
    nb = sum(bw > 0 for bw in plan['leaf_bw'])
    assert len(set(rows[:nb])) == distinct and plan['ws_mode'] == mode, (rows, plan['ws_mode'])
    ops = NumpyAdmmOps(tpl, lay, P['p'], P['x0'])
    admm = BatchADMM(lay, P['nbr'], ops, rho=2.0 if rendezvous else 1.0)
    admm.initialize()
    ops.set_time(lay, 0.0, admm.rho)
    p, x0 = ops.p.copy(), ops.x.copy()
    opts = dict(tol=1e-6, max_iter=300, warm_z_cap=0.0, max_soc=0)
    want = port_binding.solve(tpl, p, x0, n_threads=8, **opts)
    solver = BatchSolver(tpl, n, options=opts)
    try:
        assert solver.workspace()['mode'] == mode
        got = solver.solve(p, x0)
    finally:
        solver.close()
    lo = lay.x_spl
    worst = float(np.abs(got['x'][:, lo:lo + lay.ns] - want['x'][:, lo:lo + lay.ns]).max())
    print('%s: status %s, iters %s, max |coefficient diff| %.2e' % (kind, got['status'].tolist(), got['iters'].tolist(), worst))
    assert np.array_equal(got['status'], want['status']), (got['status'], want['status'])
    assert np.array_equal(got['iters'], want['iters']), (got['iters'], want['iters'])
    assert worst < TOL_X_PORT, worst
