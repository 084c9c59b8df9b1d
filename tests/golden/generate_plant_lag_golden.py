#!/usr/bin/env python
"""Generate tests/golden/plant_lag_holonomic.npz: what the REFERENCE's own `Holonomic` with `{'1storder_delay': True,
'time_constant': 0.1}` (the options of its `examples/p2p_holonomic_disturbances.py`) and its default `ideal_prediction=False,
ideal_update=False` makes of the plans stored in tests/golden/signals_holonomic.npz (4 agents, 12 updates, one knot crossing) under
the disturbance recorded in tests/golden/plant_holonomic.npz: `Vehicle.predict` from the second update on, `Holonomic.store`,
`Vehicle.simulate` with `_ode_1storder` (`vehicles/vehicle.py:326-337, 370-390, 429-431`).  No solver is involved.  Run in the build
container only:

    python tests/golden/generate_plant_lag_golden.py

The reference comes in through the shim exactly as in generate_plant_golden.py; `add_disturbance` is replaced, ON THE INSTANCE, by a
function that adds the recorded realisation of the update (held at its last value beyond the samples the update travels).

The file holds data only: the time constant, the signals state / input / dinput [4, 2, 121], the predicted state0 / input0 per update
[12, 4, 2] (row 0: not predicted, NaN), the state and the last applied input at the start of every update state_start / input_start
[12, 4, 2], and four numbers:
  lag_dev           largest deviation of the reference's odeint input samples from the recursion of include/omgx.h
                    (OMGX_HAS_PLANT_LAG: the exact solution of the lag equation under the linearly interpolated command), restarted
                    from the reference's own v_0 at each update: the error of LSODA on a kinked right-hand side
  ode_dev           the same for the state samples (simulate: the trapezoid sum of the recursion's samples from the reference's own
                    start state; predict: the trapezoid sum of the nominal inputs)
  ode_dev_chained   the same with the recursion's own input and state carried through all 12 updates
  sample_shift_dev  the smallest deviation (over agents and updates; largest over axes and samples) of the lagged input that taking
                    the commanded samples -- the nominal inputs, or the disturbance -- one sample late would cause on these plans
and the generator asserts sample_shift_dev >= 10 * max(lag_dev, ode_dev): bounds of 10 x the recorded deviations separate the
integrator's error from any indexing mistake.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TIME_CONSTANT = 0.1


def lag(v0, a, h, tc):
    """Lagged samples 0 .. n of the commanded samples a [n_in, n + 1] from v0: the statements of include/omgx.h, in their order."""
    E = np.exp(-h / tc)
    v = np.empty_like(a)
    v[:, 0] = v0
    for i in range(a.shape[1] - 1):
        s = (a[:, i + 1] - a[:, i]) / h
        r = tc * s
        v[:, i + 1] = (a[:, i + 1] - r) + ((v[:, i] - a[:, i]) + r) * E
    return v


def trapezoid(s0, a, h):
    """State samples 1 .. n of an integrator from s0 under the linearly interpolated input samples a [n_in, n + 1]."""
    return s0[:, None] + h * np.cumsum((a[:, :-1] + a[:, 1:]) / 2.0, axis=1)


def main():
    g = np.load(os.path.join(HERE, 'signals_holonomic.npz'))
    dist = np.load(os.path.join(HERE, 'plant_holonomic.npz'))['dist']
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
    state_start, input_start = np.zeros((n_upd, 4, 2)), np.zeros((n_upd, 4, 2))
    lag_dev = ode_dev = ode_dev_chained = 0.0
    shift_dev = np.inf
    for a in range(4):
        veh = Holonomic()
        veh.define_knots(knot_intervals=knot_intervals)
        assert np.array_equal(np.asarray(veh.basis.knots, dtype=float), g['knots'])
        veh.set_options({'input_disturbance': {'fc': 0.1, 'stdev': 0.05 * np.ones(2)},      # (truthy: `simulate` then calls add_disturbance)
                         '1storder_delay': True, 'time_constant': TIME_CONSTANT})
        assert not veh.options['ideal_prediction'] and not veh.options['ideal_update'] and veh.options['1storder_delay']
        update = [0]

        def recorded(inp, a=a, update=update):
            d = np.repeat(dist[a, :, update[0], -1:], inp.shape[1], axis=1)
            d[:, :n_samp + 1] = dist[a, :, update[0], :]
            return inp + d
        veh.add_disturbance = recorded
        current_time, ch_state, ch_input = 0., None, None
        for k in range(n_upd):
            update[0] = k
            if k:
                # (`Vehicle.predict`: the old plan's nominal inputs, from the state one update ago -- no lag in it)
                prev_start, nominal_prev = state_start[k - 1, a], np.asarray(veh.trajectories['input'], dtype=float)[:, :n_samp + 1]
                veh.predict(current_time, upd, st)
                state0[k, a], input0[k, a] = veh.prediction['state'], veh.prediction['input']
                ode_dev = max(ode_dev, np.abs(trapezoid(prev_start, nominal_prev, st)[:, -1] - state0[k, a]).max())
            rel = float(g['t_rel'][k])
            segs = [[BSpline(veh.basis, g['coeffs'][k, a, s]) for s in range(2)]]
            n_col = int(round((T - rel) / st, 6)) + 1            # (`Point2point.store`)
            veh.store(current_time, st, segs, T, np.linspace(rel, rel + (n_col - 1) * st, n_col))
            nominal = np.asarray(veh.trajectories['input'], dtype=float)
            have = hasattr(veh, 'signals')
            start = np.asarray(veh.signals['state'][:, -1] if have else veh.trajectories['state'][:, 0], dtype=float).copy()
            v0 = np.asarray(veh.signals['input'][:, -1] if have else veh.trajectories['input'][:, 0], dtype=float).copy()
            state_start[k, a], input_start[k, a] = start, v0
            veh.simulate(upd, st)
            got_in = np.asarray(veh.signals['input'], dtype=float)[:, -n_samp:]
            got_st = np.asarray(veh.signals['state'], dtype=float)[:, -n_samp:]
            commanded = nominal[:, :n_samp + 1] + dist[a, :, k, :]
            v = lag(v0, commanded, st, TIME_CONSTANT)
            lag_dev = max(lag_dev, np.abs(v[:, 1:] - got_in).max())
            ode_dev = max(ode_dev, np.abs(trapezoid(start, v, st) - got_st).max())
            ch_v = lag(v0 if ch_input is None else ch_input, commanded, st, TIME_CONSTANT)
            ch_s = trapezoid(start if ch_state is None else ch_state, ch_v, st)
            ode_dev_chained = max(ode_dev_chained, np.abs(ch_s - got_st).max())
            ch_state, ch_input = ch_s[:, -1], ch_v[:, -1]
            # an off-by-one choice of samples: the nominal inputs one sample late, or the disturbance one sample late
            late = lag(v0, nominal[:, 1:n_samp + 2] + dist[a, :, k, :], st, TIME_CONSTANT)
            dlate = lag(v0, nominal[:, :n_samp + 1] + np.c_[dist[a, :, k, 1:], dist[a, :, k, -1:]], st, TIME_CONSTANT)
            shift_dev = min(shift_dev, np.abs(late - v).max(), np.abs(dlate - v).max())
            current_time += upd
        for key in sig:
            sig[key].append(np.asarray(veh.signals[key], dtype=float))
    sig = {k: np.array(v) for k, v in sig.items()}
    n_col = 1 + n_samp * n_upd
    assert sig['state'].shape == (4, 2, n_col), sig['state'].shape
    print('lag_dev %.3e, ode_dev %.3e, chained %.3e, sample_shift_dev %.3e' % (lag_dev, ode_dev, ode_dev_chained, shift_dev))
    assert shift_dev >= 10 * max(lag_dev, ode_dev), (shift_dev, lag_dev, ode_dev)
    np.savez_compressed(os.path.join(HERE, 'plant_lag_holonomic.npz'), time_constant=TIME_CONSTANT, state0=state0, input0=input0,
                        state_start=state_start, input_start=input_start, lag_dev=lag_dev, ode_dev=ode_dev,
                        ode_dev_chained=ode_dev_chained, sample_shift_dev=shift_dev, **sig)
    print('plant_lag_holonomic.npz: %d agents, %d updates, %d columns' % (4, n_upd, n_col))


if __name__ == '__main__':
    main()
