#!/usr/bin/env python
"""Generate tests/golden/mission_holonomic.npz: what the REFERENCE's own `Holonomic` + `Point2point` + `Deployer` hand to their solver
when a vehicle is given a second goal -- the sequence of `examples/p2p_holonomic_multiproblem.py`: a run, `set_terminal_conditions`,
`Deployer.reset()` (`Problem.reinitialize`), then the first update of the new run with `enforce_states` and the ordinary second one.
No solver is involved: the solver call is replaced, ON THE INSTANCE, by a recorder that keeps x0 and p and returns a stored plan (the
plans of tests/golden/signals_holonomic.npz will do).  Run in the build container only:

    python tests/golden/generate_mission_golden.py

The replay: N_RUN updates of the first run (agent 0's plans 0 .. N_RUN - 1 of the fixture, no knot crossing), every one followed by
`Problem.simulate` as `Simulator.update` does; then the goal change; then two updates of the new run (agent 1's plans 0 and 1).  Once
with the ideal options (`ideal_prediction = ideal_update = True`) and once with the vehicle's defaults (the plant: `Vehicle.simulate`
by odeint, `Vehicle.predict` from the state one update ago).

The file holds data only, per run `ideal` / `plant`: x0 [N_RUN + 2, n_var] and p [N_RUN + 2, n_par] as the solver was called, the plans
returned `coeffs` [N_RUN + 2, 2, L], the logged signals `state`, `input` [2, columns] and `time`; and once: the layouts of x and p
(name, offset, rows, columns), the new goal, N_RUN, update and sample time."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_RUN = 6
GOAL_NEW = [-1.0, 1.5]


def replay(m, dep, g, ideal):
    sh = m['basics.shape']
    Holonomic = m['vehicles.holonomic'].Holonomic
    Environment = m['environment.environment'].Environment
    Obstacle = m['environment.obstacle'].Obstacle
    Point2point = m['problems.point2point'].Point2point
    upd, st = float(g['update_time']), float(g['sample_time'])
    veh = Holonomic()
    veh.define_knots(knot_intervals=len(g['knots']) - 2 * 3 - 1)
    assert np.array_equal(np.asarray(veh.basis.knots, dtype=float), g['knots'])
    if ideal:
        veh.set_options({'ideal_prediction': True, 'ideal_update': True})
    else:
        assert not veh.options['ideal_prediction'] and not veh.options['ideal_update'] and not veh.options['1storder_delay']
    start = g['state'][0, :, 0]
    veh.set_initial_conditions(list(start))
    veh.set_terminal_conditions([1.4, 1.7])
    env = Environment(room={'shape': sh.Square(5.)})
    for pos, r in (([0.1, -0.3], 0.3), ([-0.5, 0.4], 0.25), ([0.6, 0.5], 0.35)):
        env.add_obstacle(Obstacle({'position': pos}, shape=sh.Circle(r)))
    problem = Point2point(veh, env, options={'verbose': 0}, freeT=False)
    problem.init()
    father = problem.father
    import generate_golden
    lay = dict((nm, (off, r, c)) for nm, off, r, c in generate_golden.layout_of(father._var_struct))
    off, L, n = lay[veh.label + '/splines_seg0']
    assert (L, n) == g['coeffs'].shape[3:1:-1]
    calls, plans = [], []

    class Recorder(object):
        def __call__(self, x0, p, lbg, ubg):
            x = np.asarray(x0.cat, dtype=float).reshape(-1).copy()
            calls.append((x.copy(), np.asarray(p.cat, dtype=float).reshape(-1).copy()))
            x[off:off + n * L] = plans[len(calls) - 1].reshape(-1)      # (the struct is column-major: spline after spline)
            return {'x': x.reshape(-1, 1), 'lam_g': np.zeros((np.asarray(lbg.cat).size, 1))}

        def stats(self):
            return {'return_status': 'Solve_Succeeded'}
    problem.problem = Recorder()
    deployer = dep.Deployer(problem, st, upd)
    plans += [g['coeffs'][k, 0] for k in range(N_RUN)] + [g['coeffs'][k, 1] for k in range(2)]
    t = 0.0
    deployer.reset()                                         # (`Simulator.run`)
    for k in range(N_RUN + 2):
        if k == N_RUN:                                       # the goal change of examples/p2p_holonomic_multiproblem.py, and the new run
            veh.set_terminal_conditions(GOAL_NEW)
            deployer.reset()
        deployer.update(t)
        problem.simulate(t, upd, st)
        t += upd
    assert len(calls) == N_RUN + 2
    out = dict(x0=np.array([c[0] for c in calls]), p=np.array([c[1] for c in calls]), coeffs=np.array(plans))
    for nm in ('state', 'input', 'time'):
        out[nm] = np.asarray(veh.signals[nm], dtype=float)
    return out, generate_golden.layout_of(father._var_struct), generate_golden.layout_of(father._par_struct)


def main():
    g = np.load(os.path.join(HERE, 'signals_holonomic.npz'))
    sys.path.insert(0, HERE)
    import generate_golden                                   # (installs the shim's casadi; the reference comes in below)
    m = generate_golden.install_reference()
    sys.modules['omgtools.execution'].__path__ = [os.path.join(generate_golden.REF, 'execution')]
    dep = importlib.import_module('omgtools.execution.deployer')
    data, var_layout, par_layout = {}, None, None
    for tag, ideal in (('ideal', True), ('plant', False)):
        out, vl, pl = replay(m, dep, g, ideal)
        if var_layout is None:                               # (the first problem's labels: vehicle0, obstacle0 .. 2, p2p0)
            var_layout, par_layout = vl, pl
        data.update(('%s_%s' % (tag, k), v) for k, v in out.items())
        print(tag, 'leg start p', out['p'][N_RUN][:6], 't', out['p'][N_RUN][-1], 'columns', out['state'].shape[1])
    np.savez_compressed(os.path.join(HERE, 'mission_holonomic.npz'), var_layout=np.array(var_layout, dtype=object),
                        par_layout=np.array(par_layout, dtype=object), goal_new=np.array(GOAL_NEW), n_run=N_RUN,
                        update_time=float(g['update_time']), sample_time=float(g['sample_time']), horizon_time=float(g['horizon_time']), **data)
    print('mission_holonomic.npz written')


if __name__ == '__main__':
    main()
