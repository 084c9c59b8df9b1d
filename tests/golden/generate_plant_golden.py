#!/usr/bin/env python
"""Generate tests/golden/plant_holonomic.npz: what the REFERENCE's own `Holonomic` with its default options
(`ideal_prediction=False, ideal_update=False`) makes of the plans stored in tests/golden/signals_holonomic.npz (4 agents, 12
updates, one knot crossing) when an input disturbance acts on the vehicle: `Vehicle.predict` from the second update on,
`Holonomic.store`, `Vehicle.simulate` (`vehicles/vehicle.py:326-337, 370-390`).  No solver is involved.  Run in the build
container only:

    python tests/golden/generate_plant_golden.py

Two stages, because this repository's package and the reference's share the name `omgtools`:
  --dist FILE    (a child process) the disturbance realisation, from this repository's `omgtools.batch.input_disturbance(...,
                 fc=0.1, stdev=0.05, seed=3)`: [4, 2, 12, 11].
  (main)         imports the reference through the shim exactly as generate_golden.py does.  `add_disturbance` is replaced, ON THE
                 INSTANCE, by a function that adds the recorded realisation of the update (held at its last value beyond the
                 samples the update travels: the reference's odeint may look a little past the end of the interval).

The file holds data only: the disturbance, the signals state / input / dinput [4, 2, 121], the predicted state0 / input0 per
update [12, 4, 2] (row 0: not predicted, NaN), the state at the start of every update state_start [12, 4, 2], and three numbers:
  ode_dev           largest deviation of the reference's odeint state samples (simulate and predict) from the exact integral of
                    its linearly interpolated input -- the trapezoid sum --, started from the reference's own state at the start of
                    each update: the error of LSODA on a kinked input, the reference's and not a property of the statements
  ode_dev_chained   the same with the trapezoid's own state carried through all 12 updates
  sample_shift_dev  the smallest deviation (over agents and updates; largest over axes and samples) an off-by-one choice of the
                    input samples would cause on these plans
and the generator asserts sample_shift_dev >= 10 * ode_dev: a bound of 10 * ode_dev separates the integrator's error from any
indexing mistake.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FC, STDEV, SEED = 0.1, 0.05, 3


def write_disturbance(path):
    sys.path.insert(0, os.path.join(ROOT, 'omg-tools_amd'))
    from omgtools.batch import input_disturbance
    g = np.load(os.path.join(HERE, 'signals_holonomic.npz'))
    n_upd = len(g['t_rel'])
    n_samp = int(round(float(g['update_time']) / float(g['sample_time']), 6))
    n_horizon = int(round(float(g['horizon_time']) / float(g['sample_time']), 6)) + 1
    np.save(path, input_disturbance(4, 2, n_upd, n_samp, n_horizon, fc=FC, stdev=STDEV, seed=SEED))


def trapezoid(s0, a, h):
    """State samples 1 .. n of an integrator from s0 under the linearly interpolated input samples a [n_in, n + 1]."""
    return s0[:, None] + h * np.cumsum((a[:, :-1] + a[:, 1:]) / 2.0, axis=1)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'dist.npy')
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--dist', path])
        dist = np.load(path)
    g = np.load(os.path.join(HERE, 'signals_holonomic.npz'))
    sys.path.insert(0, HERE)
    import generate_golden                                   # (installs the shim's casadi; the reference comes in below)
    m = generate_golden.install_reference()
    Holonomic = m['vehicles.holonomic'].Holonomic
    BSpline = m['basics.spline'].BSpline
    T, upd, st = float(g['horizon_time']), float(g['update_time']), float(g['sample_time'])
    n_upd, n_samp = len(g['t_rel']), int(round(upd / st, 6))
    assert dist.shape == (4, 2, n_upd, n_samp + 1)
    knot_intervals = len(g['knots']) - 2 * 3 - 1
    sig = {k: [] for k in ('state', 'input', 'dinput')}
    state0 = np.full((n_upd, 4, 2), np.nan)
    input0 = np.full((n_upd, 4, 2), np.nan)
    state_start = np.zeros((n_upd, 4, 2))
    ode_dev = ode_dev_chained = 0.0
    shift_dev = np.inf
    for a in range(4):
        veh = Holonomic()
        veh.define_knots(knot_intervals=knot_intervals)
        assert np.array_equal(np.asarray(veh.basis.knots, dtype=float), g['knots'])
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
                state0[k, a], input0[k, a] = veh.prediction['state'], veh.prediction['input']
                ode_dev = max(ode_dev, np.abs(trapezoid(prev_start, nominal_prev, st)[:, -1] - state0[k, a]).max())
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
            exact = trapezoid(start, applied, st)
            ode_dev = max(ode_dev, np.abs(exact - got).max())
            chained = trapezoid(start if chained is None else chained, applied, st)
            ode_dev_chained = max(ode_dev_chained, np.abs(chained - got).max())
            chained = chained[:, -1]
            # an off-by-one choice of samples: the nominal inputs one sample late, or the disturbance one sample late
            late = trapezoid(start, nominal[:, 1:n_samp + 2] + dist[a, :, k, :], st)
            dlate = trapezoid(start, nominal[:, :n_samp + 1] + np.c_[dist[a, :, k, 1:], dist[a, :, k, -1:]], st)
            shift_dev = min(shift_dev, np.abs(late - exact).max(), np.abs(dlate - exact).max())
            current_time += upd
        for key in sig:
            sig[key].append(np.asarray(veh.signals[key], dtype=float))
    sig = {k: np.array(v) for k, v in sig.items()}
    n_col = 1 + n_samp * n_upd
    assert sig['state'].shape == (4, 2, n_col), sig['state'].shape
    print('ode_dev %.3e, chained %.3e, sample_shift_dev %.3e' % (ode_dev, ode_dev_chained, shift_dev))
    assert shift_dev >= 10 * ode_dev, (shift_dev, ode_dev)
    np.savez_compressed(os.path.join(HERE, 'plant_holonomic.npz'), dist=dist, state0=state0, input0=input0, state_start=state_start,
                        ode_dev=ode_dev, ode_dev_chained=ode_dev_chained, sample_shift_dev=shift_dev, fc=FC, stdev=STDEV, seed=SEED, **sig)
    print('plant_holonomic.npz: %d agents, %d updates, %d columns' % (4, n_upd, n_col))


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--dist':
        write_disturbance(sys.argv[2])
    else:
        main()
