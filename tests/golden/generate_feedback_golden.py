#!/usr/bin/env python
"""Generate tests/golden/feedback_holonomic.npz: what the REFERENCE's own `Holonomic.predict(..., state0=measured)` makes of the
plans stored in tests/golden/signals_holonomic.npz (4 agents, 12 updates, one knot crossing) when the state the prediction starts
from is measured outside the loop (`Deployer.update(current_time, states, ...)`, `execution/deployer.py:43-79` ->
`Vehicle.predict`, `vehicles/vehicle.py:302-337`), and of its `enforce_states` / `enforce_states + enforce_inputs` forms
(`vehicle.py:303-321`, `vehicles/holonomic.py:107-113`).  No solver and no simulated vehicle are involved.  Run in the build
container only:

    python tests/golden/generate_feedback_golden.py

The reference is imported through the shim exactly as generate_golden.py does.  Per update k >= 1 and agent the plan of update
k - 1 is stored (`Holonomic.store`) and `predict` is called with
  measured[k]   the plan's own state at the start of update k - 1 plus a seeded offset of up to 5 cm per axis,
  given_in[k]   (the enforce_inputs form only) a seeded input of up to 0.5 m/s per axis.

The file holds data only: measured, given_in [12, 4, 2]; state0 / input0 [12, 4, 2] (`prediction['state']`, `prediction['input']`
of the plain form; row 0: not predicted, NaN); enf_state0 / enf_input0 (enforce_states) and enfi_state0 / enfi_input0
(enforce_states + enforce_inputs); and two numbers:
  ode_dev           largest deviation of the reference's odeint end state from the exact integral of its linearly interpolated
                    input -- measured + the trapezoid sum --: the error of LSODA on a kinked input, the reference's and not a
                    property of the statements
  sample_shift_dev  the smallest deviation (over agents and updates; largest over axes and the state samples of the update) an
                    off-by-one choice of the input samples would cause on these plans
and the generator asserts sample_shift_dev >= 10 * ode_dev: a bound of 10 * ode_dev separates the integrator's error from any
indexing mistake.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, OFFSET, INPUT = 11, 0.05, 0.5


def trapezoid(s0, a, h):
    """State samples 1 .. n of an integrator from s0 under the linearly interpolated input samples a [n_in, n + 1]."""
    return s0[:, None] + h * np.cumsum((a[:, :-1] + a[:, 1:]) / 2.0, axis=1)


def main():
    g = np.load(os.path.join(HERE, 'signals_holonomic.npz'))
    sys.path.insert(0, HERE)
    import generate_golden                                   # (installs the shim's casadi; the reference comes in below)
    m = generate_golden.install_reference()
    Holonomic = m['vehicles.holonomic'].Holonomic
    BSpline = m['basics.spline'].BSpline
    T, upd, st = float(g['horizon_time']), float(g['update_time']), float(g['sample_time'])
    n_upd, n_samp = len(g['t_rel']), int(round(upd / st, 6))
    knot_intervals = len(g['knots']) - 2 * 3 - 1
    rng = np.random.default_rng(SEED)
    offset = rng.uniform(-OFFSET, OFFSET, size=(n_upd, 4, 2))
    given_in = rng.uniform(-INPUT, INPUT, size=(n_upd, 4, 2))
    out = {k: np.full((n_upd, 4, 2), np.nan) for k in ('measured', 'state0', 'input0', 'enf_state0', 'enf_input0', 'enfi_state0', 'enfi_input0')}
    ode_dev, shift_dev = 0.0, np.inf
    for a in range(4):
        veh = Holonomic()
        veh.define_knots(knot_intervals=knot_intervals)
        assert np.array_equal(np.asarray(veh.basis.knots, dtype=float), g['knots'])
        assert not veh.options['ideal_prediction'] and not veh.options['1storder_delay']
        current_time = 0.
        for k in range(1, n_upd):
            # the plan of update k - 1, as `Point2point.store` hands it to the vehicle
            rel = float(g['t_rel'][k - 1])
            segs = [[BSpline(veh.basis, g['coeffs'][k - 1, a, s]) for s in range(2)]]
            n_col = int(round((T - rel) / st, 6)) + 1
            veh.store(current_time, st, segs, T, np.linspace(rel, rel + (n_col - 1) * st, n_col))
            nominal = np.asarray(veh.trajectories['input'], dtype=float)
            measured = np.asarray(veh.trajectories['state'], dtype=float)[:, 0] + offset[k, a]
            out['measured'][k, a] = measured
            veh.predict(current_time, upd, st, state0=measured.copy())
            out['state0'][k, a], out['input0'][k, a] = veh.prediction['state'], veh.prediction['input']
            exact = trapezoid(measured, nominal[:, :n_samp + 1], st)
            ode_dev = max(ode_dev, np.abs(exact[:, -1] - out['state0'][k, a]).max())
            late = trapezoid(measured, nominal[:, 1:n_samp + 2], st)      # (an off-by-one choice of samples: one sample late)
            shift_dev = min(shift_dev, np.abs(late - exact).max())
            veh.predict(current_time, upd, st, state0=measured.copy(), enforce_states=True)
            out['enf_state0'][k, a], out['enf_input0'][k, a] = veh.prediction['state'], veh.prediction['input']
            veh.predict(current_time, upd, st, state0=measured.copy(), input0=given_in[k, a].copy(), enforce_states=True, enforce_inputs=True)
            out['enfi_state0'][k, a], out['enfi_input0'][k, a] = veh.prediction['state'], veh.prediction['input']
            current_time += upd
    assert np.array_equal(out['enf_state0'][1:], out['measured'][1:]) and not out['enf_input0'][1:].any()
    assert np.array_equal(out['enfi_state0'][1:], out['measured'][1:]) and np.array_equal(out['enfi_input0'][1:], given_in[1:])
    print('ode_dev %.3e, sample_shift_dev %.3e' % (ode_dev, shift_dev))
    assert shift_dev >= 10 * ode_dev, (shift_dev, ode_dev)
    np.savez_compressed(os.path.join(HERE, 'feedback_holonomic.npz'), given_in=given_in, ode_dev=ode_dev, sample_shift_dev=shift_dev,
                        seed=SEED, offset=OFFSET, **out)
    print('feedback_holonomic.npz: %d agents, %d updates' % (4, n_upd))


if __name__ == '__main__':
    main()
