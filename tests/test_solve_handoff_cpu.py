"""The host build of the solver core shares omg-tools_amd/csrc/omgx_core.h with the kernels.  The wave path's linear solve was
rebuilt there (kkt_root_solve_wave: the factorisation ends in the solution); the host build has no wave path and must compute what it
computed before: 8 agents of k7 o3 (tests/workspace_cells.py), cold solve and three steps of 0.4 knot intervals, against the loop as
the host build of the commit before that change recorded it (tests/golden/solve_handoff_host_k7_o3.npz: x, status, iters after each
of the four launches).  Statuses and iteration counts equal; x to 1e-9 -- the source, the compiler flags and the order of every sum
are the same, so the bits are expected to be the same, and the bound only leaves room for another libm behind exp / log."""
import os

import numpy as np

from workspace_cells import WAVE_CASES, build_class

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'solve_handoff_host_k7_o3.npz')
TOL_X = 1e-9


def test_host_build_compiles_from_the_shared_header(tmp_path):
    """oracle/Makefile's own rule, into a directory of the test's (the library other tests have loaded is left alone)."""
    import subprocess
    oracle_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
    subprocess.check_call(['make', '-C', oracle_dir, '-s', 'BUILD=%s' % tmp_path])
    assert os.path.getsize(os.path.join(str(tmp_path), 'libomgx_port.so')) > 0


def test_host_build_loop_is_unchanged():
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    from test_gpu_factor_instances import _loop
    case = next(c for c in WAVE_CASES if (c.knots, c.n_obs) == (7, 3))
    problem, P, _ = build_class(case, 8)
    ref = BatchP2P(problem, P, ops=port_binding, options=dict(tol=1e-3, max_iter=300), update_time=0.4 * float(problem.knot_time))
    ref.n_threads = 8
    got, crossed = _loop(ref, 3)
    want = np.load(GOLDEN)
    assert crossed == int(want['crossed']) == 1
    assert want['x'].shape == (4, 8, problem.father.template.n_var)
    for k, (x, st, it) in enumerate(got):
        worst = float(np.abs(x - want['x'][k]).max())
        print('launch %d: iters %s, max |x diff| %.2e (bound %.0e)' % (k, it.tolist(), worst, TOL_X))
        assert np.array_equal(st, want['status'][k]), (k, st, want['status'][k])
        assert np.array_equal(it, want['iters'][k]), (k, it, want['iters'][k])
        assert worst < TOL_X, (k, worst)
