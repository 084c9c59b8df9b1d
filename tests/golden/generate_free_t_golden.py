#!/usr/bin/env python
"""Generate tests/golden/free_t_holonomic.npz: what the REFERENCE's own `Holonomic` + `Point2point(freeT=True)` + `Deployer` hand to their
solver from update to update of a free-end-time run, with `ideal_prediction = ideal_update = True`.  No solver is involved: the solver
call is replaced, ON THE INSTANCE, by a recorder that keeps x0 and p and returns a stored plan -- seeded smooth coefficient sets whose T
walks through both branches of `FreeTPoint2point.init_step`: several updates at T about 10 falling by the update time, then 0.25, then
0.15 (below two update times), then 0.055 (below one: `Problem.simulate` travels a shortened span).  Run in the build container only:

    python tests/golden/generate_free_t_golden.py

Per update and basis the tables the reference actually used in `shift_spline` -> `BSplineBasis.transform` are recorded too: the
collocation matrix it solved with (the call of its linear solver is watched) and the points of its own grid at which that matrix was
evaluated (found again on the grid by their rows), mapped back from [s, 1] to [0, 1]; `proj` is the inverse of the matrix.

The file holds data only: x0 [N, n_var] and p [N, n_par] as the solver was called, the plans returned `plans` [N, n_var], per update
u >= 1 and basis j `s_u`, `fit_u_j`, `proj_u_j`, `degree_j`, `knots_j`; the logged signals `state`, `input` [2, columns] and `time`; the
layouts of x and p (name, offset, rows, columns); update and sample time."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UPDATE_TIME, SAMPLE_TIME = 0.1, 0.01
T_PLANS = [10.0, 9.9, 9.8, 9.7, 0.25, 0.15, 0.055]


def main():
    sys.path.insert(0, HERE)
    import generate_golden                                   # (installs the shim's casadi; the reference comes in below)
    m = generate_golden.install_reference()
    sys.modules['omgtools.execution'].__path__ = [os.path.join(generate_golden.REF, 'execution')]
    dep = importlib.import_module('omgtools.execution.deployer')
    sh, spl_mod, p2p_mod = m['basics.shape'], m['basics.spline'], m['problems.point2point']
    veh = m['vehicles.holonomic'].Holonomic()
    veh.define_knots(knot_intervals=5)
    veh.set_options({'ideal_prediction': True, 'ideal_update': True})
    veh.set_initial_conditions([-1.5, -1.5])
    veh.set_terminal_conditions([2., 2.])
    env = m['environment.environment'].Environment(room={'shape': sh.Square(5.)})
    Obstacle = m['environment.obstacle'].Obstacle
    env.add_obstacle(Obstacle({'position': [0.2, -0.4]}, shape=sh.Circle(0.4)))
    env.add_obstacle(Obstacle({'position': [1.0, 1.2], 'velocity': [-0.1, 0.05]}, shape=sh.Circle(0.3)))
    problem = p2p_mod.Point2point(veh, env, options={'verbose': 0}, freeT=True)
    problem.init()
    father = problem.father
    var_layout, par_layout = generate_golden.layout_of(father._var_struct), generate_golden.layout_of(father._par_struct)
    n_var = sum(r * c for _, _, r, c in var_layout)
    o_T = dict((nm, off) for nm, off, _, _ in var_layout)[problem.label + '/T']
    rng = np.random.default_rng(20240807 + 8)
    plans = np.cumsum(rng.normal(0., 0.3, (len(T_PLANS), n_var)), axis=1)
    plans[:, o_T] = T_PLANS
    calls = []

    class Recorder(object):
        def __call__(self, x0, p, lbg, ubg):
            calls.append((np.asarray(x0.cat, dtype=float).reshape(-1).copy(), np.asarray(p.cat, dtype=float).reshape(-1).copy()))
            return {'x': plans[len(calls) - 1].reshape(-1, 1).copy(), 'lam_g': np.zeros((np.asarray(lbg.cat).size, 1))}

        def stats(self):
            return {'return_status': 'Solve_Succeeded'}
    problem.problem = Recorder()

    # the tables of every `shift_spline`: watch the linear solve inside `BSplineBasis.transform`
    tables, update = {}, [0]
    real_transform, real_la = spl_mod.BSplineBasis.transform, spl_mod.la

    class WatchedLa(object):
        def __init__(self):
            self.seen = None

        def solve(self, a, b, *args, **kw):
            self.seen = np.array(a, dtype=float)
            return real_la.solve(a, b, *args, **kw)

        def __getattr__(self, name):
            return getattr(real_la, name)

    def transform(self, other, *args, **kw):
        watch = WatchedLa()
        spl_mod.la = watch
        try:
            out = real_transform(self, other, *args, **kw)
        finally:
            spl_mod.la = real_la
        key = (update[0], other.degree)
        if isinstance(other, spl_mod.BSplineBasis) and watch.seen is not None and key not in tables:
            grid = np.asarray(self._x, dtype=float)
            on_grid = np.asarray(self(grid).toarray(), dtype=float)
            rows = [int(np.argmin(np.abs(on_grid - row[None, :]).max(axis=1))) for row in watch.seen]
            assert all(np.array_equal(on_grid[i], row) for i, row in zip(rows, watch.seen))
            s = float(self.knots[0])
            tables[key] = (s, (grid[rows] - s) / (float(self.knots[-1]) - s), np.linalg.inv(watch.seen),
                           np.asarray(other.knots, dtype=float))
        return out
    spl_mod.BSplineBasis.transform = transform
    try:
        deployer = dep.Deployer(problem, SAMPLE_TIME, UPDATE_TIME)
        deployer.reset()
        t = 0.0
        for k in range(len(T_PLANS)):
            update[0] = k
            deployer.update(t)
            problem.simulate(t, UPDATE_TIME, SAMPLE_TIME)
            t += UPDATE_TIME
    finally:
        spl_mod.BSplineBasis.transform = real_transform
    assert len(calls) == len(T_PLANS)
    data = dict(x0=np.array([c[0] for c in calls]), p=np.array([c[1] for c in calls]), plans=plans)
    degrees = sorted(set(d for _, d in tables))
    for j, d in enumerate(degrees):
        data['degree_%d' % j] = d
    for (u, d), (s, fit, proj, knots) in tables.items():
        j = degrees.index(d)
        data['s_%d' % u] = s
        data['fit_%d_%d' % (u, j)], data['proj_%d_%d' % (u, j)], data['knots_%d' % j] = fit, proj, knots
    for nm in ('state', 'input', 'time'):
        data[nm] = np.asarray(veh.signals[nm], dtype=float)
    np.savez_compressed(os.path.join(HERE, 'free_t_holonomic.npz'), var_layout=np.array(var_layout, dtype=object),
                        par_layout=np.array(par_layout, dtype=object), update_time=UPDATE_TIME, sample_time=SAMPLE_TIME, n_bases=len(degrees),
                        **data)
    print('free_t_holonomic.npz written: %d calls, tables %s, T handed to the solver %s, %d logged columns'
          % (len(calls), sorted(tables), np.round(data['x0'][:, o_T], 6), data['state'].shape[1]))


if __name__ == '__main__':
    main()
