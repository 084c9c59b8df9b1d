#!/usr/bin/env python
"""What the plant in the loop costs: throughput of the receding-horizon loop of the benchmark batch (config 2, 1024 agents) with
`BatchP2P.plant` against the ideal loop -- in one launch (`rollout`) and per step (`receding_horizon_batch`: three sub-batch launches
per step) --, same process, the arms alternating, every leg from a fresh cold solve.

    python tools/plant_cost.py [--agents 1024] [--steps 60] [--reps 5] [--out profiles/plant_cost.txt]

Arms: ideal (no plant), plant (no disturbance), plant+noise (the reference's input disturbance, stdev 0.02), plant+noise+log (and the
travelled trajectories logged), plant+noise cap 20 (`max_iter_step=20`: a step's solve gives up after 20 iterations instead of 300).  A leg = `steps` updates of every agent after `warmup` untimed ones, host clock around work that ends
in a device synchronise; solves/s = agents * steps / time.  The arms do not solve the same problems after the first update (the
disturbed vehicles leave their plans), so the figure is the cost of the loop as a user runs it, iterations included.  Printed next to
the rollout legs: the mean iteration count per solve, the share of solves that did not end in Solve_Succeeded, and the longest loop
of one agent (sum of its iteration counts over the timed updates) against the mean one -- a launch lasts as long as its longest
loop, and a vehicle that a disturbance has pushed across a constraint is solved to the iteration cap at every update."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'omg-tools_amd'))

ARMS = ('ideal', 'plant', 'plant+noise', 'plant+noise+log', 'plant+noise cap 20')


def make(form, arm, problem, P, dist, max_updates, dev):
    from omgtools.batch import BatchP2P, receding_horizon_batch
    kw = dict(options=dict(tol=1e-3, max_iter=300), max_iter_step=20 if arm.endswith('cap 20') else None)
    m = BatchP2P(problem, P, ops='hip', device=dev, **kw) if form == 'rollout' else receding_horizon_batch(problem, P, device=dev, **kw)
    if arm != 'ideal':
        m.plant(sample_time=0.01, max_updates=max_updates, disturbance=dist if 'noise' in arm else None)
    if 'log' in arm:
        m.record_signals(sample_time=0.01, max_updates=max_updates)
    m.solve_cold()
    return m


def leg(form, m, steps, warmup, stats, status):
    import torch
    if form == 'rollout':
        m.rollout(warmup)
    else:
        for _ in range(warmup):
            m.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if form == 'rollout':
        m.rollout(steps, iters_log=stats, status_log=status)
    else:
        for _ in range(steps):
            m.step()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from omgtools import workloads
    from omgtools.batch import input_disturbance
    dev = torch.device('cuda', 0)
    problem, P = workloads.holonomic_p2p(a.agents)
    max_updates = a.steps + a.warmup + 1
    dist = input_disturbance(a.agents, 2, max_updates, 10, 128, fc=0.1, stdev=0.02, seed=11)
    lines = ['plant in the loop: cost on the config-2 batch, %d agents, %d timed updates after %d, %d repetitions (arms alternating), %s'
             % (a.agents, a.steps, a.warmup, a.reps, torch.cuda.get_device_name(0))]
    for form in ('rollout', 'per step'):
        rate = dict((arm, []) for arm in ARMS)
        iters = dict((arm, []) for arm in ARMS)
        for rep in range(a.reps + 1):                       # (repetition 0 warms every arm up -- code objects, allocator -- and is dropped)
            for arm in ARMS:
                m = make(form, arm, problem, P, dist, max_updates, dev)
                stats = torch.zeros((a.steps, a.agents), dtype=torch.int32, device=dev)
                status = torch.zeros((a.steps, a.agents), dtype=torch.int32, device=dev)
                dt = leg(form, m, a.steps, a.warmup, stats, status)
                if rep:
                    rate[arm].append(a.agents * a.steps / dt)
                    if form == 'rollout':
                        loops = stats.double().sum(dim=0)
                        iters[arm].append((float(stats.double().mean()), float((status != 0).double().mean()), float(loops.max()), float(loops.mean())))
                m.close() if hasattr(m, 'close') else m.solver.close()
        lines.append('%s:' % form)
        base = np.median(rate['ideal'])
        for arm in ARMS:
            r = np.array(rate[arm])
            it = ''
            if iters[arm]:
                q = np.mean(np.array(iters[arm]), axis=0)
                it = '  %.2f iterations / solve, %.2f %% of the solves not succeeded, longest loop %.0f iterations (mean %.0f)' % (q[0], 100. * q[1], q[2], q[3])
            lines.append('  %-19s median %.3f M solves/s (min %.3f, max %.3f)  %+.1f %% against ideal%s'
                         % (arm, np.median(r) / 1e6, r.min() / 1e6, r.max() / 1e6, 100. * (np.median(r) / base - 1.), it))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
