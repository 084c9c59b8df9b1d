#!/usr/bin/env python
"""What the Quadrotor's plant costs a step: the per-step loop (`receding_horizon_batch`) of a Quadrotor batch with
`plant(model='quadrotor')` on and off on this tree, and with the plant off on the parent commit.

    python tools/plant_quadrotor_cost.py [--parent DIR] [--agents 4096] [--steps 20] [--warmup 5] [--reps 3] [--rounds 3] [--tail 5] [--out FILE]

Arms: off (the ideal loop) and on (the plant, no disturbance, no log: two launches more per step and sub-batch) on this tree, off on the
parent (--parent DIR: a checkout of the parent commit with its built library).  Every tree in child processes of its own (two versions
of the package cannot share a process), `rounds` rounds with the trees alternating, each child `reps` repetitions of its arms,
alternating, after one dropped repetition, every leg from a fresh cold solve: `warmup` untimed updates, then `steps` timed ones, host
clock around work that ends in a device synchronise.  Without a disturbance the plant's prediction is the plan's own state at the next
update only up to the error of the linearly interpolated inputs, and -- as in the reference -- only the position of the prediction
enters the solver, so the vehicle's own velocity and pitch drift from the plan: the arms do NOT solve the same problems.  A step lasts as
long as its slowest solve, so behind every leg `tail` untimed updates record the mean iteration count, the count of the slowest solve
and the share of solves that did not succeed; and the two launches of the plant are timed on their own on the idle device.  Per arm: the
p50 over all repetitions of the time per step with the smallest and the largest; two arms separate when these ranges do not overlap."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    """One tree, one process: prints {arm: [[seconds, iterations per solve, share not succeeded, iterations of the slowest solve, seconds of the two launches], ...]} as one JSON line."""
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), 'omg-tools_amd'))
    import torch
    from omgtools import workloads
    from omgtools.batch import receding_horizon_batch
    dev = torch.device('cuda', 0)
    arms = [s for s in a.arms.split(',') if s]
    problem, P = workloads.quadrotor_p2p(a.agents)
    out = dict((arm, []) for arm in arms)
    for rep in range(a.reps + 1):                           # (repetition 0 warms every arm up -- code objects, allocator -- and is dropped)
        for arm in arms:
            m = receding_horizon_batch(problem, P, device=dev, options=dict(tol=1e-3, max_iter=300))
            if arm == 'on':
                m.plant(sample_time=0.01, max_updates=a.steps + a.warmup + 2 * a.tail + 1, model='quadrotor')
            m.solve_cold()
            for _ in range(a.warmup):
                m.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                m.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            # untimed: who sets the pace of a step (a launch lasts as long as its slowest solve), and the two launches on their own
            it_mean, it_max, bad = [], [], []
            for _ in range(a.tail):
                m.step()
                it = m.iters
                it_mean.append(float(it.double().mean())), it_max.append(float(it.max())), bad.append(float((m.status != 0).double().mean()))
            launch = -1.0
            if arm == 'on':
                parts = getattr(m, 'parts', [m])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.tail):                         # (on the idle device: predict + simulate of every sub-batch, back to back)
                    for q in parts:
                        q._plant_predict(0.02, 0.1)
                        q._plant_simulate()
                torch.cuda.synchronize()
                launch = (time.perf_counter() - t0) / a.tail
                assert not any(bool(q.plant_state()['overflow'].any()) for q in parts)
            if rep:
                out[arm].append((dt, float(np.mean(it_mean)), float(np.mean(bad)), float(np.mean(it_max)), launch))
            m.close() if hasattr(m, 'close') else m.solver.close()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), parts=len(getattr(m, 'parts', [m])), arms=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--tail', type=int, default=5, help='untimed updates behind a leg: iteration counts, the two launches on their own')
    ap.add_argument('--parent', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)      # (a child: measure this tree)
    ap.add_argument('--arms', default='off,on', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.tree is not None:
        return child(a)
    trees = [('this tree', ROOT, 'off,on')] + ([('parent', a.parent, 'off')] if a.parent else [])
    res, device, parts = {}, '?', 0
    for rnd in range(a.rounds):
        for tag, tree, arms in trees:
            cmd = [sys.executable, os.path.abspath(__file__), '--tree', tree, '--arms', arms, '--agents', str(a.agents), '--steps', str(a.steps),
                   '--warmup', str(a.warmup), '--reps', str(a.reps), '--tail', str(a.tail)]
            got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
            got = json.loads([ln for ln in got.splitlines() if ln.startswith('RESULT ')][-1][7:])
            device, parts = got['device'], got['parts']
            for arm, rows in got['arms'].items():
                res.setdefault((tag, arm), []).extend(rows)
    lines = ["Quadrotor's plant: cost of a step of the config-3 batch (Quadrotor, 5 moving obstacles), %d agents in %d sub-batches, %d timed updates "
             'after %d, %d rounds x %d repetitions per tree (trees and arms alternating), no disturbance, no log, %s'
             % (a.agents, parts, a.steps, a.warmup, a.rounds, a.reps, device)]
    rng = {}
    for (tag, arm), rows in res.items():
        ms = 1e3 * np.array([r[0] for r in rows]) / a.steps
        rng[(tag, arm)] = (ms.min(), ms.max(), np.median(ms))
        lines.append('  %-9s plant %-3s p50 %.3f ms / step (min %.3f, max %.3f; spread %.1f %% of p50; %d runs)   %.1f k solves/s;  the %d updates behind: '
                     '%.2f iterations / solve, the slowest solve of an update %.0f iterations on average, %.3f %% of the solves not succeeded'
                     % (tag, arm, np.median(ms), ms.min(), ms.max(), 100. * (ms.max() - ms.min()) / np.median(ms), len(ms), a.agents / np.median(ms), a.tail,
                        np.mean([r[1] for r in rows]), np.mean([r[3] for r in rows]), 100. * np.mean([r[2] for r in rows])))
        if arm == 'on':
            lm = 1e3 * np.array([r[4] for r in rows])
            lines.append('            the two launches of the plant on their own (predict + simulate of every sub-batch, idle device, host clock over %d '
                         'repetitions ending in a synchronise): p50 %.3f ms per update of the batch (min %.3f, max %.3f)' % (a.tail, np.median(lm), lm.min(), lm.max()))

    def compare(u, v):
        (lo0, hi0, m0), (lo1, hi1, m1) = rng[u], rng[v]
        lines.append('  %s plant %s against %s plant %s: %+.1f %% time at p50 (%+.3f ms); the ranges %s'
                     % (v[0], v[1], u[0], u[1], 100. * (m1 / m0 - 1.), m1 - m0,
                        'overlap -- the two do not separate' if lo1 <= hi0 and lo0 <= hi1 else 'do not overlap -- the two separate'))
    compare(('this tree', 'off'), ('this tree', 'on'))
    if a.parent:
        compare(('parent', 'off'), ('this tree', 'off'))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
