#!/usr/bin/env python
"""Generate tests/golden/obstacle_script.npz: what the REFERENCE's own `Obstacle` makes of `simulation={'trajectories': {...}}`
(`environment/obstacle.py:172-264`: `prepare_simulation`, `_ode`, `simulate`) -- 4 circular 2-D obstacles, 60 updates of 0.1 s,
`sample_time` 0.01, as `Simulator.run` calls `environment.simulate(update_time, sample_time)`.  No solver is involved.  Run in the
build container only:

    python tests/golden/generate_obstacle_script_golden.py

The reference comes in through the shim exactly as in generate_golden.py.  The scripts:
  obstacle 0   the one of `examples/p2p_holonomic_multiproblem.py:35-38`: at rest until its first event, velocity jumps on the update
               grid, at 3.0 and 4.0
  obstacle 1   drifting from the start; a velocity jump off the update grid (1.25), a position jump on it (2.0), an acceleration
               jump off the SAMPLE grid (3.333)
  obstacle 2   two kinds at one time (velocity and acceleration at 2.5), a velocity jump at the end of the run's first update (0.1)
  obstacle 3   two events inside one update (velocity at 4.52 and 4.57), an acceleration jump on the grid (1.5) and its reversal
               off the grid (5.05)
The on-grid times are chosen where the reference's own time axis (`signals['time']`, accumulated `linspace` ends) reaches the
nominal time: at some boundaries (0.8 .. 1.1, 4.7 .. 6.0 with these settings) it ends one ulp short of it, the zero-order
interpolation of the increments then shows a jump at that time only in the NEXT update's samples -- the same trajectory, but a
boundary state without the jump.  The generator asserts that no on-grid event sits on such a boundary.

The file holds data only: the events (ev_time, ev_obstacle, ev_kind [E], ev_value [E, 2], ascending in time), the initial states
(initial [3, 4, 2]: position, velocity, acceleration), the reference's position / velocity / acceleration at every update boundary
([61, 4, 2]: `signals[...][:, -1]` after every `simulate`, row 0 the initial state), update_time, sample_time, and two numbers:
  ode_dev    largest deviation (position, velocity or acceleration) of the reference's state at the end of an update from the exact
             piecewise motion -- constant acceleration between the jumps, closed form below -- started from the reference's own
             state at the start of that update: the error of LSODA at a discontinuity, the reference's and not a property of the
             statement
  late_dev   the smallest, over the events, of the position deviation an event applied one `sample_time` late would cause: the
             larger of the deviations at the end of the update that holds the event and at the end of the update after it (an event
             ON the update grid moves into the next update when it is late, and a velocity jump shows in the position only there),
             both from the reference's state at the start of the update that holds the event
and the generator asserts late_dev >= 10 * ode_dev: a bound of 10 * ode_dev separates the integrator's error from any indexing
mistake.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
UPDATE_TIME, SAMPLE_TIME, N_UPD = 0.1, 0.01, 60
KINDS = ('position', 'velocity', 'acceleration')

INITIAL = [{'position': [1.0, 0.5]},
           {'position': [-0.5, 0.25], 'velocity': [0.1, -0.05]},
           {'position': [0.0, -1.0], 'velocity': [0.0, 0.2], 'acceleration': [0.01, 0.0]},
           {'position': [2.0, 2.0]}]
SCRIPTS = [{'velocity': {'time': [3., 4.], 'values': [[-0.15, 0.0], [0., 0.15]]}},
           {'velocity': {'time': [1.25], 'values': [[0.2, 0.1]]},
            'position': {'time': [2.0], 'values': [[0.3, -0.2]]},
            'acceleration': {'time': [3.333], 'values': [[-0.2, 0.25]]}},
           {'velocity': {'time': [0.1, 2.5], 'values': [[0.12, 0.0], [-0.1, -0.3]]},
            'acceleration': {'time': [2.5], 'values': [[0.0, 0.15]]}},
           {'velocity': {'time': [4.52, 4.57], 'values': [[0.3, 0.0], [-0.1, 0.2]]},
            'acceleration': {'time': [1.5, 5.05], 'values': [[0.2, -0.2], [-0.2, 0.2]]}}]


def exact(state, events, t0, t1):
    """(x, v, a) [each [2]] carried from t0 to t1 with constant acceleration between the jumps events = [(time, kind, value)] with
    t0 < time <= t1 (ascending)."""
    x, v, a = (np.array(s, dtype=float) for s in state)
    cur = [x, v, a]
    t = t0
    for tau, kind, val in events:
        h = tau - t
        cur[0] = cur[0] + h * cur[1] + 0.5 * h * h * cur[2]
        cur[1] = cur[1] + h * cur[2]
        cur[kind] = cur[kind] + val
        t = tau
    h = t1 - t
    cur[0] = cur[0] + h * cur[1] + 0.5 * h * h * cur[2]
    cur[1] = cur[1] + h * cur[2]
    return cur


def within(events, t0, t1):
    return [e for e in events if t0 + 1e-9 < e[0] <= t1 + 1e-9]


def main():
    sys.path.insert(0, HERE)
    import generate_golden                                   # (installs the shim's casadi; the reference comes in below)
    m = generate_golden.install_reference()
    Obstacle = m['environment.obstacle'].Obstacle
    Circle = m['basics.shape'].Circle
    n_obs = len(INITIAL)
    table = sorted([(float(tau), q, KINDS.index(kind), np.asarray(val, dtype=float)) for q, sc in enumerate(SCRIPTS)
                    for kind, traj in sc.items() for tau, val in zip(traj['time'], traj['values'])], key=lambda r: r[0])
    bounds = np.round(np.arange(N_UPD + 1) * UPDATE_TIME, 9)
    sig = np.zeros((3, N_UPD + 1, n_obs, 2))
    ode_dev, late_dev = 0.0, np.inf
    for q in range(n_obs):
        obs = Obstacle(dict((k, list(v)) for k, v in INITIAL[q].items()), shape=Circle(0.3),
                       simulation={'trajectories': dict((k, dict(time=list(t['time']), values=[list(v) for v in t['values']])) for k, t in SCRIPTS[q].items())})
        assert not obs.options['bounce']
        for o, key in enumerate(KINDS):
            sig[o, 0, q] = np.asarray(obs.signals[key], dtype=float)[:, -1]
            assert np.array_equal(sig[o, 0, q], np.asarray(INITIAL[q].get(key, [0., 0.]), dtype=float))
        for k in range(N_UPD):
            obs.simulate(UPDATE_TIME, SAMPLE_TIME)
            assert abs(float(obs.signals['time'][-1]) - bounds[k + 1]) < 1e-9
            for tau, qq, _, _ in table:
                assert qq != q or abs(tau - bounds[k + 1]) > 1e-9 or float(obs.signals['time'][-1]) >= tau, (q, tau)
            for o, key in enumerate(KINDS):
                sig[o, k + 1, q] = np.asarray(obs.signals[key], dtype=float)[:, -1]
        mine = [(tau, kind, val) for tau, qq, kind, val in table if qq == q]
        for k in range(N_UPD):
            ev = within(mine, bounds[k], bounds[k + 1])
            got = exact(sig[:, k, q], [(min(tau, bounds[k + 1]), kind, val) for tau, kind, val in ev], bounds[k], bounds[k + 1])
            ode_dev = max(ode_dev, max(np.abs(got[o] - sig[o, k + 1, q]).max() for o in range(3)))
            for j, late in enumerate(ev):
                # this event one sample late, every other one in its place: the two boundaries after the start of this update
                moved = sorted([(tau + (SAMPLE_TIME if (tau, kind) == (late[0], late[1]) else 0.0), kind, val) for tau, kind, val in mine],
                               key=lambda r: r[0])
                t0, t1, t2 = bounds[k], bounds[k + 1], bounds[min(k + 2, N_UPD)]
                dev = 0.0
                for end in (t1, t2):
                    right = exact(sig[:, k, q], [e for e in mine if t0 + 1e-9 < e[0] <= end + 1e-9], t0, end)
                    wrong = exact(sig[:, k, q], [e for e in moved if t0 + 1e-9 < e[0] <= end + 1e-9], t0, end)
                    dev = max(dev, np.abs(right[0] - wrong[0]).max())
                late_dev = min(late_dev, dev)
    print('ode_dev %.3e, late_dev %.3e' % (ode_dev, late_dev))
    assert late_dev >= 10 * ode_dev, (late_dev, ode_dev)
    np.savez_compressed(os.path.join(HERE, 'obstacle_script.npz'),
                        ev_time=np.array([r[0] for r in table]), ev_obstacle=np.array([r[1] for r in table], dtype=np.int32),
                        ev_kind=np.array([r[2] for r in table], dtype=np.int32), ev_value=np.array([r[3] for r in table]),
                        initial=sig[:, 0], position=sig[0], velocity=sig[1], acceleration=sig[2],
                        update_time=UPDATE_TIME, sample_time=SAMPLE_TIME, ode_dev=ode_dev, late_dev=late_dev)
    print('obstacle_script.npz: %d obstacles, %d updates, %d events' % (n_obs, N_UPD, len(table)))


if __name__ == '__main__':
    main()
