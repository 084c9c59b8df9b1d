#!/usr/bin/env python
"""Developer tool: the tile-owner form of the Schur phase against the round form inside one library, through whole solves.

The plan reads OMGX_NO_SCHUR_TILES when it is made, so each form runs in a child process of its own: 8 agents, a cold solve and three
receding-horizon steps of 0.4 knot intervals for each (knot intervals, obstacles) of CASES, and one cold x-update of the formation and
rendez-vous bundles at 64 agents.  Every array of every solve (x, status, iters, and lam_g where the solver returns it) is written
to DIR/{tiles,rounds}/ and compared as bytes; the form each plan reports (omgx_plan_schur_tiles) is printed per case.  Exits non-zero
on a difference.  The record of one run is section 1 of profiles/schur_tiles_ab.txt.

    python tools/schur_forms_ab.py DIR            (on a machine with the GPU)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'omg-tools_amd'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CASES = [(11, 3), (11, 5), (10, 3), (7, 1), (4, 1), (4, 3)]
OPTS = dict(tol=1e-3, max_iter=300)


def _template_only(fn, *a, **kw):
    import omgtools.backend as be
    saved = be.create_nlp
    be.create_nlp = lambda tpl, opt, name='': (None, 0.)
    try:
        return fn(*a, **kw)
    finally:
        be.create_nlp = saved


def child(out):
    import numpy as np
    import torch
    from omgtools import scenarios, workloads
    from omgtools.admm import BatchADMM
    from omgtools.backend import BatchSolver, plan_schur_tiles
    from omgtools.batch import BatchP2P
    from admm_numpy_ops import NumpyAdmmOps
    os.makedirs(out, exist_ok=True)
    label = 'round form (OMGX_NO_SCHUR_TILES=1)' if os.environ.get('OMGX_NO_SCHUR_TILES') else 'tile owners'
    for knots, n_obs in CASES:
        problem, P = _template_only(scenarios.holonomic_p2p, 8, knot_intervals=knots, n_obs=n_obs)
        print('%s: k%d o%d tiles reported %d' % (label, knots, n_obs, plan_schur_tiles(problem.father.template)), flush=True)
        mpc = BatchP2P(problem, P, ops='hip', device=torch.device('cuda', 0), options=OPTS, update_time=0.4 * float(problem.knot_time))
        try:
            mpc.solve_cold(bends=())
            for s in range(4):
                if s:
                    mpc.step()
                for name in ('x', 'status', 'iters'):
                    np.save(os.path.join(out, 'k%d_o%d_s%d_%s.npy' % (knots, n_obs, s, name)), mpc.host(name))
        finally:
            mpc.solver.close()
    for kind in ('formation', 'rendezvous'):
        rendezvous = kind == 'rendezvous'
        problem, updater, father, lay, P = (workloads.rendezvous_holonomic if rendezvous else workloads.formation_holonomic)(64)
        tpl = father.template
        print('%s: %s tiles reported %d' % (label, kind, plan_schur_tiles(tpl)), flush=True)
        ops = NumpyAdmmOps(tpl, lay, P['p'], P['x0'])
        admm = BatchADMM(lay, P['nbr'], ops, rho=2.0 if rendezvous else 1.0)
        admm.initialize()
        ops.set_time(lay, 0.0, admm.rho)
        solver = BatchSolver(tpl, 64, options=dict(tol=1e-6, max_iter=300, warm_z_cap=0.0, max_soc=0))
        try:
            got = solver.solve(ops.p.copy(), ops.x.copy())
        finally:
            solver.close()
        for name in ('x', 'status', 'iters', 'lam_g'):
            if name in got:
                np.save(os.path.join(out, '%s_%s.npy' % (kind, name)), got[name])


def main():
    if len(sys.argv) == 3 and sys.argv[1] == '--child':
        return child(sys.argv[2])
    out = sys.argv[1]
    for form in ('tiles', 'rounds'):
        env = dict(os.environ)
        env.pop('OMGX_NO_SCHUR_TILES', None)
        if form == 'rounds':
            env['OMGX_NO_SCHUR_TILES'] = '1'
        # (a fresh child per form; stop at the first one that fails: nothing more on a device that reported an error)
        subprocess.run([sys.executable, os.path.abspath(__file__), '--child', os.path.join(out, form)], env=env, check=True, timeout=240)
    names = sorted(os.listdir(os.path.join(out, 'tiles')))
    different = 0
    for n in names:
        a = open(os.path.join(out, 'tiles', n), 'rb').read()
        b = open(os.path.join(out, 'rounds', n), 'rb').read()
        different += a != b
        if n.endswith('_x.npy') or a != b:
            print('%-24s %8d bytes  %s' % (n[:-4], len(a), 'byte-equal' if a == b else 'DIFFERENT'))
    print('arrays %d different %d' % (len(names), different))
    return 1 if different or sorted(os.listdir(os.path.join(out, 'rounds'))) != names else 0


if __name__ == '__main__':
    sys.exit(main())
