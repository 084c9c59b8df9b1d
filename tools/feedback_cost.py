#!/usr/bin/env python
"""What feeding measured states back costs: the per-step loop of the benchmark batch (config 2, 1024 agents, `receding_horizon_batch`:
three sub-batch launches per step) stepped with `step()` against `step(states=...)` -- same process, the arms alternating, every leg
from a fresh cold solve.

    python tools/feedback_cost.py [--agents 1024] [--steps 60] [--reps 7] [--arms ideal,feedback,plant] [--tree DIR] [--out FILE]

Arms: ideal (`step()`: predict_kernel + solve), feedback (`step(states=S)`: feedback_predict_kernel + solve -- one small launch in
the place of another), plant (`plant()` without a disturbance: plant_predict_kernel + solve + plant_simulate_kernel, for scale).  The
states fed are those of the undisturbed plant, recorded in an untimed pass (`plant_state()['state_prev']` ahead of every step): the
feedback arm then solves the plant arm's problems bit for bit, and those differ from the ideal arm's by the error of the trapezoid
rule only (printed per arm: iterations per solve and solves not succeeded at the last timed update).  A leg = `steps` updates of
every agent after `warmup` untimed ones, host clock around work that ends in a device synchronise.  Per arm: the p50 over the
repetitions of the time per step and of the rate, with the smallest and the largest repetition; two arms separate when their
[min, max] ranges do not overlap.

--tree DIR: import the package from another checkout (DIR/omg-tools_amd, with its built library) -- the parent commit's `step()` on the
same box is `--tree <parent checkout> --arms ideal`, run alternately with this tree's."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ('ideal', 'feedback', 'plant')


def make(arm, problem, P, max_updates, dev):
    from omgtools.batch import receding_horizon_batch
    m = receding_horizon_batch(problem, P, device=dev, options=dict(tol=1e-3, max_iter=300))
    if arm == 'plant':
        m.plant(sample_time=0.01, max_updates=max_updates)
    if arm == 'feedback':
        m.feedback(sample_time=0.01)
    m.solve_cold()
    return m


def record_states(problem, P, n, max_updates, dev):
    """[n, B, n_spl]: `state_prev` of the undisturbed plant ahead of each of n steps."""
    import torch
    m = make('plant', problem, P, max_updates, dev)
    rec = []
    for _ in range(n):
        rec.append(m.plant_state()['state_prev'].clone())
        torch.cuda.synchronize()                            # (the sub-batch streams of the next step do not wait for this copy)
        m.step()
    torch.cuda.synchronize()
    m.close() if hasattr(m, 'close') else m.solver.close()
    return torch.stack(rec).contiguous()


def leg(arm, m, steps, warmup, rec):
    import torch
    step = (lambda k: m.step(states=rec[k])) if arm == 'feedback' else (lambda k: m.step())
    for k in range(warmup):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(warmup, warmup + steps):
        step(k)
    t_issue = time.perf_counter() - t0                      # (the host is done issuing; the device is not)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, t_issue, float(m.iters.double().mean()), int((m.status != 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--arms', default=','.join(ARMS))
    ap.add_argument('--tree', default=ROOT)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    arms = [s for s in a.arms.split(',') if s]
    if any(s not in ARMS for s in arms):
        ap.error('arms are %s' % ', '.join(ARMS))
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), 'omg-tools_amd'))
    import torch
    from omgtools import workloads
    dev = torch.device('cuda', 0)
    problem, P = workloads.holonomic_p2p(a.agents)
    max_updates = a.steps + a.warmup + 1
    rec = record_states(problem, P, a.steps + a.warmup, max_updates, dev) if 'feedback' in arms else None
    lines = ['measured states in the loop: cost on the config-2 batch, %d agents, per-step path, %d timed updates after %d, %d repetitions '
             '(arms alternating), %s, tree %s' % (a.agents, a.steps, a.warmup, a.reps, torch.cuda.get_device_name(0), os.path.relpath(os.path.abspath(a.tree), ROOT))]
    secs = dict((arm, []) for arm in arms)
    last = dict((arm, []) for arm in arms)                  # (iterations per solve and solves not succeeded at the last timed update)
    for rep in range(a.reps + 1):                           # (repetition 0 warms every arm up -- code objects, allocator -- and is dropped)
        for arm in arms:
            m = make(arm, problem, P, max_updates, dev)
            dt, t_issue, it, bad = leg(arm, m, a.steps, a.warmup, rec)
            if rep:
                secs[arm].append(dt)
                last[arm].append((it, bad, t_issue))
            m.close() if hasattr(m, 'close') else m.solver.close()
    base = np.median(secs[arms[0]])
    for arm in arms:
        t = np.array(secs[arm])
        ms, rate = 1e3 * t / a.steps, a.agents * a.steps / t / 1e6
        lines.append('  %-9s p50 %.4f ms / step (min %.4f, max %.4f)   p50 %.3f M solves/s (min %.3f, max %.3f)   %+.1f %% time against %s;  '
                     'host issuing a step p50 %.4f ms;  last update: %.2f iterations / solve, %d of %d not succeeded'
                     % (arm, np.median(ms), ms.min(), ms.max(), np.median(rate), rate.min(), rate.max(), 100. * (np.median(t) / base - 1.), arms[0],
                        1e3 * np.median([q[2] for q in last[arm]]) / a.steps, np.mean([q[0] for q in last[arm]]), max(q[1] for q in last[arm]), a.agents))
    for arm in arms[1:]:
        lo0, hi0, lo1, hi1 = min(secs[arms[0]]), max(secs[arms[0]]), min(secs[arm]), max(secs[arm])
        lines.append('  %s against %s: the ranges %s' % (arm, arms[0], 'overlap -- the two do not separate' if lo1 <= hi0 and lo0 <= hi1 else 'do not overlap -- the two separate'))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
