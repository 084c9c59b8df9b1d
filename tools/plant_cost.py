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
loop, and a vehicle that a disturbance has pushed across a constraint is solved to the iteration cap at every update.

    python tools/plant_cost.py --lag [--parent DIR] [--agents 1024] [--steps 20] [--warmup 5] [--reps 3] [--rounds 3] [--time-constant 0.1] [--tiny 1e-4]

The lag leg: what the first-order actuator lag (`plant(time_constant=...)`) costs, and whether the plant WITHOUT it costs what it did on
the parent commit.  Arms: step_plant / rollout_plant (the plant on, no lag: the per-step loop of `receding_horizon_batch`, and one
`rollout(steps)` launch) on this tree and on the parent (--parent DIR: a checkout of the parent commit with its built library), step_lag /
rollout_lag (time constant --time-constant) and step_lag_tiny / rollout_lag_tiny (--tiny, 1e-4 s: the lag routine runs, the vehicles
stay within some 1e-4 m/s of their commands, so the problems stay those of the plain arms up to that -- the cost of the mechanism) on
this tree.  No disturbance: the lag-off arms of the two trees solve the same problems; the lag arms solve others (the vehicles fall
behind their plans, and one that the mismatch has pushed across a constraint is solved to the iteration cap at every update and sets
the pace of the batch), iterations per solve are printed.  Every tree in child processes of its own (two versions of the
package cannot share a process), `rounds` rounds with the trees alternating, each child `reps` repetitions of its arms, alternating,
after one dropped repetition, every leg from a fresh cold solve.  Per arm: the p50 over all repetitions of the time per step with
the smallest and the largest; two arms separate when these ranges do not overlap."""
import argparse
import json
import os
import subprocess
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


LAG_ARMS = ('step_plant', 'step_lag_tiny', 'step_lag', 'rollout_plant', 'rollout_lag_tiny', 'rollout_lag')


def lag_child(a):
    """One tree, one process: prints {arm: [[seconds, iterations per solve, share not succeeded], ...]} as one JSON line."""
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), 'omg-tools_amd'))
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P, receding_horizon_batch
    dev = torch.device('cuda', 0)
    arms = [s for s in a.arms.split(',') if s]
    problem, P = workloads.holonomic_p2p(a.agents)
    out = dict((arm, []) for arm in arms)
    for rep in range(a.reps + 1):                           # (repetition 0 warms every arm up -- code objects, allocator -- and is dropped)
        for arm in arms:
            form = 'rollout' if arm.startswith('rollout') else 'per step'
            kw = dict(options=dict(tol=1e-3, max_iter=300))
            m = BatchP2P(problem, P, ops='hip', device=dev, **kw) if form == 'rollout' else receding_horizon_batch(problem, P, device=dev, **kw)
            lag = dict(time_constant=a.tiny) if arm.endswith('_tiny') else (dict(time_constant=a.time_constant) if arm.endswith('_lag') else {})
            m.plant(sample_time=0.01, max_updates=a.steps + a.warmup + 1, **lag)
            m.solve_cold()
            stats = torch.zeros((a.steps, a.agents), dtype=torch.int32, device=dev)
            status = torch.zeros((a.steps, a.agents), dtype=torch.int32, device=dev)
            dt = leg(form, m, a.steps, a.warmup, stats, status)
            if rep:
                out[arm].append((dt, float(stats.double().mean()), float((status != 0).double().mean())) if form == 'rollout' else (dt, -1.0, -1.0))
            m.close() if hasattr(m, 'close') else m.solver.close()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), arms=out)))


def lag_main(a):
    trees = [('this tree', ROOT, ','.join(LAG_ARMS))] + ([('parent', a.parent, 'step_plant,rollout_plant')] if a.parent else [])
    res, device = {}, '?'
    for rnd in range(a.rounds):
        for tag, tree, arms in trees:
            cmd = [sys.executable, os.path.abspath(__file__), '--lag', '--tree', tree, '--arms', arms, '--agents', str(a.agents), '--steps', str(a.steps),
                   '--warmup', str(a.warmup), '--reps', str(a.reps), '--time-constant', str(a.time_constant), '--tiny', str(a.tiny)]
            got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
            got = json.loads([ln for ln in got.splitlines() if ln.startswith('RESULT ')][-1][7:])
            device = got['device']
            for arm, rows in got['arms'].items():
                res.setdefault((tag, arm), []).extend(rows)
    lines = ['plant lag: cost on the config-2 batch, %d agents, %d timed updates after %d, %d rounds x %d repetitions per tree (trees and arms '
             'alternating), no disturbance, time constant %g s (tiny: %g s), %s' % (a.agents, a.steps, a.warmup, a.rounds, a.reps, a.time_constant, a.tiny, device)]
    rng = {}
    for (tag, arm), rows in res.items():
        ms = 1e3 * np.array([r[0] for r in rows]) / a.steps
        rng[(tag, arm)] = (ms.min(), ms.max(), np.median(ms))
        it = '' if rows[0][1] < 0 else ';  %.2f iterations / solve, %.2f %% of the solves not succeeded' % (
            np.mean([r[1] for r in rows]), 100. * np.mean([r[2] for r in rows]))
        lines.append('  %-9s %-14s p50 %.4f ms / step (min %.4f, max %.4f; spread %.1f %% of p50; %d runs)   %.3f M solves/s%s'
                     % (tag, arm, np.median(ms), ms.min(), ms.max(), 100. * (ms.max() - ms.min()) / np.median(ms), len(ms), a.agents / np.median(ms) / 1e3, it))

    def compare(u, v):
        (lo0, hi0, m0), (lo1, hi1, m1) = rng[u], rng[v]
        lines.append('  %s %s against %s %s: %+.1f %% time at p50; the ranges %s' % (v[0], v[1], u[0], u[1], 100. * (m1 / m0 - 1.),
                     'overlap -- the two do not separate' if lo1 <= hi0 and lo0 <= hi1 else 'do not overlap -- the two separate'))
    if a.parent:
        compare(('parent', 'step_plant'), ('this tree', 'step_plant'))
        compare(('parent', 'rollout_plant'), ('this tree', 'rollout_plant'))
    for form in ('step', 'rollout'):
        compare(('this tree', form + '_plant'), ('this tree', form + '_lag_tiny'))
        compare(('this tree', form + '_plant'), ('this tree', form + '_lag'))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=None)
    ap.add_argument('--warmup', type=int, default=None)
    ap.add_argument('--reps', type=int, default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--lag', action='store_true', help='the lag leg (see the docstring)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--time-constant', type=float, default=0.1)
    ap.add_argument('--tiny', type=float, default=1e-4, help='time constant of the *_lag_tiny arms')
    ap.add_argument('--parent', default=None)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)      # (a child of the lag leg: measure this tree)
    ap.add_argument('--arms', default=','.join(LAG_ARMS), help=argparse.SUPPRESS)
    a = ap.parse_args()
    for nm, plain, lag in (('steps', 60, 20), ('warmup', 10, 5), ('reps', 5, 3)):
        if getattr(a, nm) is None:
            setattr(a, nm, lag if a.lag else plain)
    if a.lag:
        return lag_child(a) if a.tree is not None else lag_main(a)
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
