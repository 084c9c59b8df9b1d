#!/usr/bin/env python
"""Developer tool: what the travelled-trajectory log (`BatchP2P.record_signals`) costs on the 1024-agent benchmark batch.

    python tools/signals_cost.py [--agents 1024] [--steps 130] [--reps 3] > profiles/signals_on_ab.txt

Times the whole manoeuvre with the stop rule (cold solve outside the clock) (a) as ONE `rollout(steps)` launch and (b) as `steps`
`step()` calls, each with the log off and on, `reps` times each, interleaved; prints per variant the best and the median wall time,
solves (the iteration-carrying updates: agents under way), solves/s and the time per solve, and the difference the log makes.
Wall time between two device synchronisations around the loop (host launches included: this is what a caller sees)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'omg-tools_amd'))


def run(n, steps, mode, log):
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = workloads.holonomic_p2p(n)
    m = BatchP2P(problem, P, ops='hip', device=torch.device('cuda', 0), options=dict(tol=1e-3, max_iter=300))
    m.stop_at_arrival()
    if log:
        m.record_signals(sample_time=0.01, max_updates=steps + 1)
    m.solve_cold()
    it_log = torch.zeros((steps, n), dtype=torch.int32, device=m.dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if mode == 'rollout':
        m.rollout(steps, iters_log=it_log)
    else:
        for k in range(steps):
            m.step()
            it_log[k].copy_(m.iters)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    solves = int((it_log > 0).sum().item())
    left = int(m.under_way.sum().item())
    cols = int(m.signals()['count'].sum().item()) if log else 0
    m.solver.close()
    return dt, solves, left, cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=130)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    print('# %d agents, %d updates, stop rule on, tol 1e-3; wall time of the loop, %d runs per variant (interleaved)' % (a.agents, a.steps, a.reps))
    res = {}
    run(a.agents, 5, 'rollout', True)                       # (warm-up: library load, first launches)
    for r in range(a.reps):
        for mode in ('rollout', 'step'):
            for log in (False, True):
                res.setdefault((mode, log), []).append(run(a.agents, a.steps, mode, log))
    for mode in ('rollout', 'step'):
        med = {}
        for log in (False, True):
            ts = np.array([q[0] for q in res[(mode, log)]])
            solves, left, cols = res[(mode, log)][0][1:]
            med[log] = (np.median(ts), solves)
            print('%-8s log %-3s  best %8.2f ms  median %8.2f ms  solves %7d  %6.3f M solves/s  %7.3f us/solve  under way at the end %d  columns logged %d  runs(ms) %s'
                  % (mode, 'on' if log else 'off', ts.min() * 1e3, np.median(ts) * 1e3, solves, solves / np.median(ts) / 1e6,
                     np.median(ts) / max(solves, 1) * 1e6, left, cols, ' '.join('%.2f' % (t * 1e3) for t in ts)))
        d = med[True][0] - med[False][0]
        print('%-8s log on - off: %+.2f ms (%+.1f %%), %+.3f us per solve' % (mode, d * 1e3, 100. * d / med[False][0], d / max(med[True][1], 1) * 1e6))


if __name__ == '__main__':
    main()
