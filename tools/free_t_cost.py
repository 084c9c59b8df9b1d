#!/usr/bin/env python
"""What the free-end-time loop costs: one MI355X, the batch of `scenarios.holonomic_free_t_p2p` (Holonomic, a standing and a moving
circle, T a variable of every agent).

    python tools/free_t_cost.py [--agents 1024] [--knot-intervals 10] [--reps 3] [--max-steps 150] [--phase-steps 40] [--out FILE]

Two legs per repetition, each from a fresh cold solve with the stop rule and the log on, after one dropped repetition:
`manoeuvre` -- `step()` until no agent is under way (looked at every tenth step: one synchronise) or `max-steps`, host clock around
the loop that ends in a device synchronise; reported: solves (agents solved, counted on the device from `iters > 0`) per second,
iterations per solve, steps, agents arrived.  `phases` -- the first `phase-steps` steps with device events around the three launches of
a step (advance, solve with its launch-order kernel, append): p50 per launch.  Nothing like it was measured before: report only."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'omg-tools_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1024)
    ap.add_argument('--knot-intervals', type=int, default=10)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--max-steps', type=int, default=150)
    ap.add_argument('--phase-steps', type=int, default=40)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from omgtools.batch import BatchP2P
    from omgtools.scenarios import holonomic_free_t_p2p
    dev = torch.device('cuda', 0)
    problem, P = holonomic_free_t_p2p(a.agents, knot_intervals=a.knot_intervals)
    tpl = problem.father.template

    def fresh():
        m = BatchP2P(problem, P, ops='hip', device=dev, options=dict(tol=1e-3, max_iter=300))
        m.stop_at_arrival()
        m.record_signals(max_updates=a.max_steps + 1)
        m.solve_cold()
        return m

    runs, phases, cold = [], [], []
    for rep in range(a.reps + 1):
        m = fresh()
        cold.append((int((m.status == 0).sum()), float(m.iters.float().mean())))
        solves = torch.zeros((), dtype=torch.int64, device=dev)
        iters = torch.zeros((), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = 0
        while steps < a.max_steps:
            m.step()
            steps += 1
            solves += (m.iters > 0).sum()
            iters += m.iters.sum()
            if steps % 10 == 0 and not bool((m.under_way != 0).any()):
                break
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        summ = m.summary()
        arrived = int(((m.under_way == 0) & (summ[:, 5] < 1e-2)).sum())
        if rep:
            runs.append((dt, int(solves), int(iters), steps, arrived, float(summ[:, 1].median())))
        m.solver.close()
        m = fresh()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.phase_steps)]
        for k in range(a.phase_steps):                      # (the statements of `BatchP2P._step_free_t`, an event between its launches)
            ev[k][0].record()
            m._free_t_advance()
            m._advance_obstacles(m.time, m.time + m.update_time)
            m.time += m.update_time
            ev[k][1].record()
            m._solve(True)
            ev[k][2].record()
            m._signals_append_now()
            ev[k][3].record()
        torch.cuda.synchronize()
        if rep:
            phases.append([[e[i].elapsed_time(e[i + 1]) for i in range(3)] for e in ev])
        m.solver.close()
    ph = np.array(phases).reshape(-1, 3)
    rate = np.array([r[1] / r[0] for r in runs])
    lines = ['Free end time: %d agents of holonomic_free_t_p2p, knot_intervals %d (n_var %d, n_con %d), tol 1e-3, %d repetitions after one dropped, %s'
             % (a.agents, a.knot_intervals, tpl.n_var, tpl.n_con, a.reps, torch.cuda.get_device_name(0)),
             '  cold solve: %d of %d agents succeeded, %.1f iterations on average' % (cold[-1][0], a.agents, cold[-1][1]),
             '  manoeuvre (step() until no agent is under way, stop rule and log on): raw runs (k solves/s): %s' % ' '.join('%.1f' % (v / 1e3) for v in rate),
             '            p50 %.1f k solves/s (min %.1f, max %.1f); %d solves, %.2f iterations per solve, %d steps in %.1f ms (%.3f ms per step); '
             '%d of %d agents arrived within 1e-2, median motion time %.2f s'
             % (np.median(rate) / 1e3, rate.min() / 1e3, rate.max() / 1e3, runs[0][1], runs[0][2] / max(1, runs[0][1]), runs[0][3],
                1e3 * np.median([r[0] for r in runs]), 1e3 * np.median([r[0] / r[3] for r in runs]), runs[0][4], a.agents, runs[0][5]),
             '  per launch of a step, device events, first %d steps, p50 (min .. max) in microseconds:' % a.phase_steps]
    for i, nm in enumerate(('advance (+ obstacle motion)', 'solve (+ launch order)', 'append')):
        lines.append('            %-28s %7.1f (%.1f .. %.1f)' % (nm, 1e3 * np.median(ph[:, i]), 1e3 * ph[:, i].min(), 1e3 * ph[:, i].max()))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
