#!/usr/bin/env python
"""What a mission costs, and that the plain rollout is what it was: one MI355X, a batch of the headline class (config 2, Holonomic with
three obstacles).

    python tools/mission_cost.py [--parent DIR] [--agents 1024] [--steps 150] [--plain-steps 120] [--reps 3] [--rounds 3] [--out FILE]

Arms: `mission` (this tree: `stop_at_arrival(1.5)`, three further goals per agent -- back to its start, to its first goal again, back
once more --, the whole mission as ONE `rollout(steps)` launch; reported: solves/s with the cold leg-start solves included, and the share
of the solves that were leg starts) and `plain` (the stop-rule manoeuvre as one `rollout(plain_steps)` launch with `stop_at_arrival(1e-3)`,
no mission: on this tree and, with --parent DIR -- a checkout of the parent commit with its built library --, on the parent; the
existing kernel instances are meant to be the same code).  Every tree in child processes of its own (two versions of the package cannot
share a process), `rounds` rounds with the trees alternating, each child `reps` repetitions of its arms after one dropped repetition,
every leg from a fresh cold solve, host clock around a launch that ends in a device synchronise.  Per arm the p50 over all repetitions
with the smallest and the largest; two arms separate when these ranges do not overlap."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    """One tree, one process: prints {arm: [[seconds, solves, leg starts], ...]} as one JSON line."""
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), 'omg-tools_amd'))
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    dev = torch.device('cuda', 0)
    arms = [s for s in a.arms.split(',') if s]
    problem, P = workloads.holonomic_p2p(a.agents)
    out = dict((arm, []) for arm in arms)
    for rep in range(a.reps + 1):                           # (repetition 0 warms every arm up -- code objects, allocator -- and is dropped)
        for arm in arms:
            m = BatchP2P(problem, P, ops='hip', device=dev, options=dict(tol=1e-3, max_iter=300))
            K = a.steps if arm == 'mission' else a.plain_steps
            m.stop_at_arrival(stop_tol=1.5 if arm == 'mission' else 1e-3)
            m.solve_cold()
            if arm == 'mission':
                n, L = m.n_dim, m.L
                x0 = np.asarray(P['x0'], dtype=float)
                start = np.stack([x0[:, m.o_spl + k * L] for k in range(n)], axis=1)
                o_pose = m._o_pose('mission')
                goal0 = m.host('p')[:, o_pose:o_pose + n]
                m.mission(np.stack([start, goal0, start], axis=1))
            it_log = torch.zeros((K, a.agents), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.rollout(K, iters_log=it_log)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            starts = int((m.mission_state()['arrivals'][:, :-1] >= 0).sum()) if arm == 'mission' else 0
            if rep:
                out[arm].append((dt, int((it_log > 0).sum()), starts, int((m.under_way != 0).sum())))
            m.solver.close()
    print('RESULT ' + json.dumps(dict(device=torch.cuda.get_device_name(0), arms=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=150, help='steps per agent of the mission launch')
    ap.add_argument('--plain-steps', type=int, default=120, help='steps per agent of the plain stop-rule launch')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)      # (a child: measure this tree)
    ap.add_argument('--arms', default='plain,mission', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.tree is not None:
        return child(a)
    trees = [('this tree', ROOT, 'plain,mission')] + ([('parent', a.parent, 'plain')] if a.parent else [])
    res, device = {}, '?'
    for rnd in range(a.rounds):
        for tag, tree, arms in trees:
            cmd = [sys.executable, os.path.abspath(__file__), '--tree', tree, '--arms', arms, '--agents', str(a.agents), '--steps', str(a.steps),
                   '--plain-steps', str(a.plain_steps), '--reps', str(a.reps)]
            got = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
            got = json.loads([ln for ln in got.splitlines() if ln.startswith('RESULT ')][-1][7:])
            device = got['device']
            for arm, rows in got['arms'].items():
                res.setdefault((tag, arm), []).extend(rows)
    lines = ['Missions: %d agents of config 2, one launch per run, %d rounds x %d repetitions per tree (trees alternating), %s' % (a.agents, a.rounds, a.reps, device)]
    rng = {}
    for (tag, arm), rows in res.items():
        rate = np.array([r[1] / r[0] for r in rows]) / 1e6
        rng[(tag, arm)] = (rate.min(), rate.max(), np.median(rate))
        lines.append('  %-9s %-7s raw runs (M solves/s): %s' % (tag, arm, ' '.join('%.3f' % v for v in rate)))
        lines.append('            p50 %.3f M solves/s (min %.3f, max %.3f; spread %.1f %% of p50); %d solves in %.1f ms per run; %d agents still under way at the end'
                     % (np.median(rate), rate.min(), rate.max(), 100. * (rate.max() - rate.min()) / np.median(rate), rows[0][1], 1e3 * np.median([r[0] for r in rows]), rows[0][3]))
        if arm == 'mission':
            lines.append('            leg starts (cold solves inside the launch): %d of %d solves = %.2f %%' % (rows[0][2], rows[0][1], 100. * rows[0][2] / rows[0][1]))
    if a.parent:
        (lo0, hi0, m0), (lo1, hi1, m1) = rng[('parent', 'plain')], rng[('this tree', 'plain')]
        spread = max((hi0 - lo0) / m0, (hi1 - lo1) / m1)
        lines.append('  plain rollout, this tree against parent: %+.1f %% solves/s at p50; run-to-run spread observed in this session %.1f %%: %s'
                     % (100. * (m1 / m0 - 1.), 100. * spread, 'no change' if abs(m1 / m0 - 1.) <= spread else 'THE MEDIANS LIE FURTHER APART THAN THE SPREAD'))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
