#!/usr/bin/env python
"""Generate tests/golden/plant_quadrotor.npz: what the REFERENCE's own `Quadrotor` with its default options
(`ideal_prediction=False, ideal_update=False`) makes of 8 updates of solved plans of the Quadrotor class (4 agents, update 4 crosses a
knot: the class's knot_time is 0.3846 s) when an input disturbance acts on the vehicle: `Vehicle.predict` from the second update on,
`Vehicle.store`, `Vehicle.simulate` (`vehicles/vehicle.py:326-337, 370-390`) with the model's own `ode`
(`vehicles/quadrotor.py:149-152`).  Run in the build container only:

    python tests/golden/generate_plant_quadrotor_golden.py

Two stages, because this repository's package and the reference's share the name `omgtools`:
  --plans FILE   (a child process) this repository's host loop -- `workloads.quadrotor_p2p(4)`, `oracle.port_binding`, tol 1e-6 -- with
                 `plant(model='quadrotor')` and the disturbance `input_disturbance(4, 2, 8, 10, ..., fc=0.1, stdev=0.05, seed=3)`: the
                 cold solve and 7 steps.  Recorded: the plan coefficients and t_rel of every update, the disturbance.
  (main)         imports the reference through the shim exactly as generate_golden.py does.  `add_disturbance` is replaced, ON THE
                 INSTANCE, by a function that adds the recorded realisation of the update (held at its last value beyond the samples
                 the update travels).  It replays predict / store / simulate over the recorded plans; no solver is involved.

The file holds data only: knots, coeffs [8, 4, 2, L], t_rel [8], dist [4, 2, 8, 11], the signals state [4, 5, 81], input [4, 2, 81], dspl
[4, 2, 81], the predicted spl0 / dspl0 / ddspl0 per update [8, 4, 2] (row 0: not predicted, NaN), the state at the start of every
update state_start [8, 4, 5], and three numbers:
  ode_dev           largest deviation of the reference's odeint state samples (simulate, all five entries, and the predicted position)
                    from classical Runge-Kutta on its linearly interpolated input -- the statements of include/omgx.h
                    OMGX_HAS_PLANT_QUADROTOR, written out below --, started from the reference's own state at the start of each update
  ode_dev_chained   the same with the Runge-Kutta chain's own state carried through all 8 updates
  sample_shift_dev  the smallest deviation (over agents and updates; largest over entries and samples) that taking the disturbance one
                    sample late -- every update -- or the nominal inputs one sample late -- THE ACCELERATING UPDATES ONLY, see below --
                    would cause on these plans
and the generator asserts sample_shift_dev >= 100 * ode_dev (ode_dev over ALL updates): a bound of 10 * ode_dev sits a factor ten below
any indexing mistake.

Restricted to the accelerating updates.  On the solved plans the vehicles leave rest during the updates 0 .. 3 (`accelerating` in the
file: 1 1 1 1 0 0 0 0); from update 4 on the thrust sits at its bound u1max and the pitch rate is nearly steady, so the nominal inputs
are constant over an update and taking them one sample late moves the state by 4e-7 .. 7e-5 only (1e-3 in the last update of two
agents): a shift of a constant is invisible by construction, whatever the code does.  The nominal-input shift is therefore counted over
the updates 0 .. 3 (3e-3 or more), the disturbance shift over all eight (1.3e-4 or more).  The factor 100 is not loosened, all eight
updates stay in the file, and the tests hold every update, the steady ones and the knot crossing included, to 10 * ode_dev.
"""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FC, STDEV, SEED = 0.1, 0.05, 3
N_AGENTS, N_UPD, SAMPLE_TIME, GRAVITY = 4, 8, 0.01, 9.81
ACCELERATING = (1, 1, 1, 1, 0, 0, 0, 0)      # (the updates in which the nominal inputs move: the docstring)


def write_plans(path):
    sys.path.insert(0, os.path.join(ROOT, 'omg-tools_amd'))
    sys.path.insert(0, ROOT)
    from omgtools import workloads
    from omgtools.batch import BatchP2P, input_disturbance
    from oracle import port_binding
    problem, P = workloads.quadrotor_p2p(N_AGENTS)
    m = BatchP2P(problem, P, ops=port_binding, options=dict(tol=1e-6, max_iter=500))
    n_samp = int(round(m.update_time / SAMPLE_TIME, 6))
    n_horizon = int(round(m.T / SAMPLE_TIME, 6)) + 1
    dist = input_disturbance(N_AGENTS, 2, N_UPD, n_samp, n_horizon, fc=FC, stdev=STDEV, seed=SEED)
    m.plant(sample_time=SAMPLE_TIME, max_updates=N_UPD, disturbance=dist, model='quadrotor', gravity=GRAVITY)
    coeffs, t_rel, crossed = [], [], []
    for k in range(N_UPD):
        crossed.append(bool(m.step()) if k else (m.solve_cold() and False))
        assert (m.status == 0).all(), (k, m.status)
        coeffs.append(m.x[:, m.o_spl:m.o_spl + 2 * m.L].reshape(N_AGENTS, 2, m.L).copy())
        t_rel.append(float(m.p[0, m.o_t]))
    assert crossed == [False] * 4 + [True] + [False] * 3, crossed      # (update 4, the fifth solve, is the first behind the knot)
    np.savez(path, coeffs=np.array(coeffs), t_rel=np.array(t_rel), dist=dist, knots=np.asarray(m.basis.knots, dtype=float),
             horizon_time=m.T, update_time=m.update_time, knot_time=m.knot_time)


def quad_ode(s, u1, u2, g):
    return np.array([s[2], s[3], u1 * math.sin(s[4]), u1 * math.cos(s[4]) - g, u2])


def rk4(s0, a, h, g):
    """State samples 0 .. n [5, n + 1] from s0 under the linearly interpolated input samples a [2, n + 1]: per interval k1 at a_i, k2
    and k3 at (a_i + a_{i+1}) / 2, k4 at a_{i+1}."""
    n = a.shape[1] - 1
    out = np.empty((5, n + 1))
    s = np.array(s0, dtype=float)
    out[:, 0] = s
    for i in range(n):
        ua, ub = a[:, i], a[:, i + 1]
        um = 0.5 * (ua + ub)
        k1 = quad_ode(s, ua[0], ua[1], g)
        k2 = quad_ode(s + 0.5 * h * k1, um[0], um[1], g)
        k3 = quad_ode(s + 0.5 * h * k2, um[0], um[1], g)
        k4 = quad_ode(s + h * k3, ub[0], ub[1], g)
        s = s + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        out[:, i + 1] = s
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'plans.npz')
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--plans', path])
        g = dict(np.load(path))
    dist = g['dist']
    sys.path.insert(0, HERE)
    import generate_golden                                   # (installs the shim's casadi; the reference comes in below)
    m = generate_golden.install_reference()
    Quadrotor = m['vehicles.quadrotor'].Quadrotor
    BSpline = m['basics.spline'].BSpline
    T, upd, st = float(g['horizon_time']), float(g['update_time']), SAMPLE_TIME
    n_upd, n_samp, A = N_UPD, int(round(upd / st, 6)), N_AGENTS
    assert dist.shape == (A, 2, n_upd, n_samp + 1)
    knot_intervals = len(g['knots']) - 2 * 4 - 1
    sig = {k: [] for k in ('state', 'input', 'dspl')}
    pred = {k: np.full((n_upd, A, 2), np.nan) for k in ('spl0', 'dspl0', 'ddspl0')}
    state_start = np.zeros((n_upd, A, 5))
    ode_dev = ode_dev_chained = 0.0
    shift_dev = np.inf
    for a in range(A):
        veh = Quadrotor()
        veh.define_knots(knot_intervals=knot_intervals)
        assert np.array_equal(np.asarray(veh.basis.knots, dtype=float), g['knots']) and veh.g == GRAVITY
        assert not veh.options['ideal_prediction'] and not veh.options['ideal_update'] and not veh.options['1storder_delay']
        veh.set_options({'input_disturbance': {'fc': FC, 'stdev': STDEV * np.ones(2)}})      # (truthy: `simulate` then calls add_disturbance)
        update = [0]

        def recorded(inp, a=a, update=update):
            d = np.repeat(dist[a, :, update[0], -1:], inp.shape[1], axis=1)
            d[:, :n_samp + 1] = dist[a, :, update[0], :]
            return inp + d
        veh.add_disturbance = recorded
        current_time, chained = 0., None
        for k in range(n_upd):
            update[0] = k
            if k:
                # (`Vehicle.predict`: the old plan's inputs, from the state one update ago)
                prev_start, nominal_prev = state_start[k - 1, a], np.asarray(veh.trajectories['input'], dtype=float)[:, :n_samp + 1]
                veh.predict(current_time, upd, st)
                pred['spl0'][k, a] = np.asarray(veh.prediction['state'], dtype=float)[:2]
                pred['dspl0'][k, a], pred['ddspl0'][k, a] = veh.prediction['dspl'], veh.prediction['ddspl']
                ode_dev = max(ode_dev, np.abs(rk4(prev_start, nominal_prev, st, GRAVITY)[:2, -1] - pred['spl0'][k, a]).max())
            rel = float(g['t_rel'][k])
            segs = [[BSpline(veh.basis, g['coeffs'][k, a, s]) for s in range(2)]]
            n_col = int(round((T - rel) / st, 6)) + 1            # (`Point2point.store`)
            veh.store(current_time, st, segs, T, np.linspace(rel, rel + (n_col - 1) * st, n_col))
            nominal = np.asarray(veh.trajectories['input'], dtype=float)
            start = np.asarray(veh.signals['state'][:, -1] if hasattr(veh, 'signals') else veh.trajectories['state'][:, 0], dtype=float).copy()
            state_start[k, a] = start
            veh.simulate(upd, st)
            got = np.asarray(veh.signals['state'], dtype=float)[:, -n_samp:]
            applied = nominal[:, :n_samp + 1] + dist[a, :, k, :]
            assert np.abs(np.asarray(veh.signals['input'], dtype=float)[:, -n_samp:] - applied[:, 1:]).max() == 0.
            exact = rk4(start, applied, st, GRAVITY)[:, 1:]
            ode_dev = max(ode_dev, np.abs(exact - got).max())
            chained = rk4(start if chained is None else chained, applied, st, GRAVITY)[:, 1:]
            ode_dev_chained = max(ode_dev_chained, np.abs(chained - got).max())
            chained = chained[:, -1]
            # an off-by-one choice of samples: the nominal inputs one sample late, or the disturbance one sample late
            late = rk4(start, nominal[:, 1:n_samp + 2] + dist[a, :, k, :], st, GRAVITY)[:, 1:]
            dlate = rk4(start, nominal[:, :n_samp + 1] + np.c_[dist[a, :, k, 1:], dist[a, :, k, -1:]], st, GRAVITY)[:, 1:]
            shift_dev = min(shift_dev, np.abs(dlate - exact).max())
            if ACCELERATING[k]:
                shift_dev = min(shift_dev, np.abs(late - exact).max())
            current_time += upd
        for key in sig:
            sig[key].append(np.asarray(veh.signals[key], dtype=float))
    sig = {k: np.array(v) for k, v in sig.items()}
    n_col = 1 + n_samp * n_upd
    assert sig['state'].shape == (A, 5, n_col) and sig['input'].shape == (A, 2, n_col) and sig['dspl'].shape == (A, 2, n_col), sig['state'].shape
    print('ode_dev %.3e, chained %.3e, sample_shift_dev %.3e (ratio %.0f)' % (ode_dev, ode_dev_chained, shift_dev, shift_dev / ode_dev))
    assert shift_dev >= 100 * ode_dev, (shift_dev, ode_dev)
    np.savez_compressed(os.path.join(HERE, 'plant_quadrotor.npz'), knots=g['knots'], coeffs=g['coeffs'], t_rel=g['t_rel'], dist=dist,
                        horizon_time=T, update_time=upd, sample_time=st, knot_time=float(g['knot_time']), gravity=GRAVITY,
                        state_start=state_start, ode_dev=ode_dev, ode_dev_chained=ode_dev_chained, sample_shift_dev=shift_dev,
                        accelerating=np.array(ACCELERATING, dtype=np.int32), fc=FC, stdev=STDEV, seed=SEED, **dict(sig, **pred))
    print('plant_quadrotor.npz: %d agents, %d updates, %d columns' % (A, n_upd, n_col))


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--plans':
        write_plans(sys.argv[2])
    else:
        main()
