#!/usr/bin/env python
"""Generate tests/golden/signals_holonomic.npz: the travelled trajectories (`vehicle.signals`) the REFERENCE's own
`Holonomic.store` + `Vehicle.simulate` (with `ideal_update`) build from a sequence of plans.  No solver is involved on the
reference's side: it is pure spline evaluation.  Run in the build container only:

    python tests/golden/generate_signals_golden.py

Two stages, because this repository's package and the reference's share the name `omgtools`:
  --plans FILE   (a child process) the host loop of this repository (`BatchP2P` over the oracle port) on the 8 agents of the
                 config-2 workload, update_time 0.1: the cold solve and 11 steps -- 12 updates, one knot crossing inside
                 (t = 1.0 passes the knot at 0.909).  Writes the spline coefficients and t (time since the last knot) of
                 four agents whose cold solve succeeded, per update.
  (main)         imports the reference through the shim exactly as generate_golden.py does and feeds those plans, update by
                 update, through `Holonomic.store` (time axis of `Point2point.store`, `problems/point2point.py:213-229`) and
                 `Vehicle.simulate` (`vehicles/vehicle.py:359-369`), sample_time 0.01.

The file holds data only: coeffs [12, 4, 2, L], t_rel [12], agents [4], knots, horizon_time, update_time, sample_time and the
signals state / input / dinput [4, 2, 121], time [121].
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
N_UPDATES, UPDATE_TIME, SAMPLE_TIME = 12, 0.1, 0.01


def write_plans(path):
    sys.path.insert(0, os.path.join(ROOT, 'omg-tools_amd'))
    sys.path.insert(0, ROOT)
    import omgtools.backend as be
    from omgtools.scenarios import holonomic_p2p
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    saved = be.create_nlp
    be.create_nlp = lambda tpl, opt, name='': (None, 0.)
    try:
        problem, P = holonomic_p2p(8)
    finally:
        be.create_nlp = saved
    mpc = BatchP2P(problem, P, ops=port_binding, options=dict(tol=1e-3, max_iter=300), update_time=UPDATE_TIME)
    mpc.solve_cold()
    agents = np.flatnonzero(mpc.status == 0)[:4]
    assert len(agents) == 4
    lo, n = mpc.o_spl, mpc.n_spl * mpc.L
    coeffs, t_rel, crossings = [], [], 0
    for k in range(N_UPDATES):
        if k:
            crossings += int(mpc.step())
        coeffs.append(mpc.x[agents, lo:lo + n].reshape(4, mpc.n_spl, mpc.L).copy())
        t_rel.append(float(mpc.p[0, mpc.o_t]))
    assert crossings == 1
    np.savez(path, coeffs=np.array(coeffs), t_rel=np.array(t_rel), agents=agents, knots=np.asarray(mpc.basis.knots),
             horizon_time=mpc.T, knot_intervals=problem.vehicles[0].knot_intervals)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        plans = os.path.join(tmp, 'plans.npz')
        subprocess.check_call([sys.executable, os.path.abspath(__file__), '--plans', plans])
        d = dict(np.load(plans))
    sys.path.insert(0, HERE)
    import generate_golden                                   # (installs the shim's casadi; the reference comes in below)
    m = generate_golden.install_reference()
    Holonomic = m['vehicles.holonomic'].Holonomic
    BSpline = m['basics.spline'].BSpline
    T, kt = float(d['horizon_time']), None
    out = {}
    for a in range(4):
        veh = Holonomic()
        veh.define_knots(knot_intervals=int(d['knot_intervals']))
        veh.set_options({'ideal_update': True})
        assert np.array_equal(np.asarray(veh.basis.knots, dtype=float), d['knots'])
        current_time = 0.
        for k in range(N_UPDATES):
            rel = float(d['t_rel'][k])
            segs = [[BSpline(veh.basis, d['coeffs'][k, a, s]) for s in range(2)]]
            n_samp = int(round((T - rel) / SAMPLE_TIME, 6)) + 1       # (`Point2point.store`)
            time_axis = np.linspace(rel, rel + (n_samp - 1) * SAMPLE_TIME, n_samp)
            veh.store(current_time, SAMPLE_TIME, segs, T, time_axis)
            veh.simulate(UPDATE_TIME, SAMPLE_TIME)
            current_time += UPDATE_TIME
        for key in ('state', 'input', 'dinput', 'time'):
            out.setdefault(key, []).append(np.asarray(veh.signals[key], dtype=float))
    sig = {k: np.array(v) for k, v in out.items()}
    n_col = 1 + int(round(UPDATE_TIME / SAMPLE_TIME, 6)) * N_UPDATES
    assert sig['state'].shape == (4, 2, n_col), sig['state'].shape
    time = sig.pop('time')
    assert np.abs(time - time[0]).max() == 0.
    np.savez_compressed(os.path.join(HERE, 'signals_holonomic.npz'), coeffs=d['coeffs'], t_rel=d['t_rel'], agents=d['agents'],
                        knots=d['knots'], horizon_time=T, update_time=UPDATE_TIME, sample_time=SAMPLE_TIME,
                        time=time[0].reshape(-1), **sig)
    print('signals_holonomic.npz: %d agents, %d updates, %d columns' % (4, N_UPDATES, n_col))


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--plans':
        write_plans(sys.argv[2])
    else:
        main()
