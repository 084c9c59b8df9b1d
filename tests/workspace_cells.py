"""The workspace cells of the wave path and the class that stands for each (tests/test_workspace_cells_cpu.py,
tests/test_gpu_workspace_cells.py).

A template class on the wave path gets its workspace mode when the handle is created (`plan_for_mode`, omgx.hip): 0 (everything in
LDS), 5 or 4 (the compact store with Jacobian values in a slab: include/omgx.h), tried in this order, first for two agents per CU --
workgroups of 256 threads, the LDS part within `kLdsHalf` = 160 KiB / 2 - 512 B -- then for one agent per CU, 512 threads.  Every
(mode, per CU) cell has kernel instances of its own (the selectors of omgx_device.h, the units omgx_inst_*.hip): full / lean / refine
solve, six rollout instances, eval.  The headline fleet (`workloads.holonomic_p2p`, k11 / 3 obstacles) sits in ONE cell, mode 5 with
two per CU; the classes below are what a user gets with other knot counts and obstacle numbers.

The table is what `describe_plan` / `plan_schur_tiles` report for `scenarios.holonomic_p2p(n, knot_intervals=k, n_obs=o)` (host
only).  The sweep behind it: k = 4 .. 12, o = 1 .. 10, built with zero agents (the plan needs the template, not the parameter
rows).  The cells and every class of the sweep in them:

    mode 0, two per CU: k4 o1-8, k5 o1-6, k6 o1-5, k7 o1-4, k8 o1-3, k9 o1-2, k10 o1-2, k11 o1-2;
    mode 5, two per CU: k4 o9-10, k5 o7-8, k6 o6-7, k7 o5, k8 o4, k9 o3-4, k10 o3, k11 o3;
    mode 4, two per CU: k5 o9, k7 o6, k8 o5;
    mode 0, one per CU: k5 o10, k6 o8-10, k7 o7-9, k8 o6-8, k9 o5-7, k10 o4-6, k11 o4-5 -- k10 o4 is the smallest (114192 B);
    mode 5, one per CU: k7 o10, k8 o9-10, k9 o8-9, k10 o7-8, k11 o6-7;
    mode 4, one per CU: k9 o10 (159416 B) and k10 o9 (162760 B) -- k9 o10 is the smaller;
    k10 o10 and k11 o8-10 fit a whole CU in none of the three modes (the blocked routines with a spill mode); k12 and beyond leave
    the wave path (root wider than 40 columns).

Parameter rows.  The builder places the obstacles by rejection sampling -- discs in a box of 1.6 m with `gap` between any two --
which at the default gap of 0.25 m does not return for 8 and more obstacles; its own `gap` argument is what a user with so many
obstacles sets.  k9 o10 is built with gap = 0: discs may touch, and from the straight-line guess some agents then end in a local
infeasibility (status 2, on the host build and the device alike).  The refine case asks for status 0 (the bound of
`test_refined_steps_match_port`), so the case takes the first seed after the default one at which the HOST BUILD converges for all
eight agents, plain and refined, over the cold solve and three steps (default + 6; tried in order, the device not consulted).

`build_class` is the one way a test gets a class: it asserts the cell from the plan, so no case can silently run another instance
than the one it is there for."""
import collections

LDS_PER_CU = 160 * 1024            # MI355X: 160 KiB of LDS per compute unit
LDS_HALF = LDS_PER_CU // 2 - 512   # `kLdsHalf` (omgx.hip): the LDS part of a two-per-CU workgroup

Cell = collections.namedtuple('Cell', 'id knots n_obs wave_path mode per_cu schur_tiles why gap seed', defaults=(0.25, None))
DEFAULT_SEED = 20240807 + 2        # (of `scenarios.holonomic_p2p`)

CASES = [
    Cell('k7_o3_mode0_two_per_cu', 7, 3, 1, 0, 2, 3, 'mode 0 with 256 threads: everything in LDS, four waves'),
    Cell('k7_o6_mode4_two_per_cu', 7, 6, 1, 4, 2, 6, 'mode 4 with 256 threads: next to it in the cell k5 o9 and k8 o5; six tiles on three owner waves'),
    Cell('k11_o6_mode5_one_per_cu', 11, 6, 1, 5, 1, 6, 'mode 5 with 512 threads: eight waves, eight scratch blocks, tile owners three of eight'),
    Cell('k11_o3_mode5_two_per_cu_headline', 11, 3, 1, 5, 2, 3, 'the headline class (every other GPU test): the control'),
    Cell('k10_o4_mode0_one_per_cu', 10, 4, 1, 0, 1, 4, 'mode 0 with 512 threads: the smallest class of the sweep in this cell; leaf order 33'),
    Cell('k9_o10_mode4_one_per_cu', 9, 10, 1, 4, 1, 10, 'mode 4 with 512 threads: the smaller of the two classes of the sweep in this cell; ten tiles, '
         'eleven leaves on eight waves', gap=0.0, seed=DEFAULT_SEED + 6),
    Cell('k13_o1_off_the_wave_path', 13, 1, 0, 0, 1, 0, 'off the wave path, all in LDS: ipm_solve_kernel<WS_LDS, false, ...>, no rollout instance'),
]
WAVE_CASES = [c for c in CASES if c.wave_path]


def threads(case):
    """Workgroup size of the cell's launches."""
    return 256 if case.per_cu == 2 else 512


def cell_of(plan, tiles):
    """(wave path, mode, agents per CU, Schur-tile leaves) as the plan report states them."""
    per_cu = 2 if plan['wave_path'] and plan['lds_bytes'] <= LDS_HALF else 1
    return int(plan['wave_path']), int(plan['ws_mode']), per_cu, int(tiles)


_BUILT = {}


def build_class(case, n):
    """(problem, P, plan) of `n` agents of the case's class, its cell asserted from the plan report.  The front end builds a class
    once per process (its labels count up with every object built, and the parameter generator draws agent after agent from one
    seeded stream: the first n rows are the batch of n agents); every caller gets the shared problem and rows of its own."""
    if case.id not in _BUILT or len(_BUILT[case.id][1]['p']) < n:
        _BUILT[case.id] = _build_class(case, max(n, 8))
    problem, P, plan = _BUILT[case.id]
    return problem, dict((k, v[:n].copy()) for k, v in P.items()), plan


def _build_class(case, n):
    from omgtools import scenarios
    from omgtools.backend import describe_plan, plan_schur_tiles
    from test_gpu_factor_instances import _template_only
    kw = dict(gap=case.gap) if case.seed is None else dict(gap=case.gap, seed=case.seed)
    problem, P = _template_only(scenarios.holonomic_p2p, n, knot_intervals=case.knots, n_obs=case.n_obs, **kw)
    tpl = problem.father.template
    plan = describe_plan(tpl)
    got, want = cell_of(plan, plan_schur_tiles(tpl)), (case.wave_path, case.mode, case.per_cu, case.schur_tiles)
    assert got == want, ('%s: the plan puts k%d o%d into cell (wave path, mode, per CU, tiles) = %s, the table says %s (%d B of LDS): a change '
                         'to the work split moved the class -- the GPU cases of that cell need a new representative (sweep in the docstring '
                         'of tests/workspace_cells.py)' % (case.id, case.knots, case.n_obs, got, want, plan['lds_bytes']))
    if case.wave_path:
        assert (plan['lds_bytes'] <= LDS_HALF) == (case.per_cu == 2) and plan['lds_bytes'] <= LDS_PER_CU, (case.id, plan['lds_bytes'])
    return problem, P, plan
