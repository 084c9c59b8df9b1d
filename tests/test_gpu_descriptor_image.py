"""The matrix descriptors of the wave path as a plan-time image (HostPlan::bmat_img, omg-tools_amd/csrc/omgx_plan.h): the plan fills
them once per template with the statements a workgroup used to run per solve (kkt_describe_fill, omgx_core.h) and the kernels copy
them (kkt_descriptors).  A wrong descriptor -- an offset, a band width, a leaf taken for the root -- derails the factorisation of
every iteration, so the device loop is held against the host build of the same solver (oracle/port_binding), which writes its
descriptors itself on every solve, in the pattern of tests/test_gpu_batch_mpc.py: a cold solve and receding-horizon steps across a
knot crossing (the step that follows the shift runs on other options and other multipliers, through the same descriptors).

Statuses and iteration counts are integers and must be equal.  The plans are compared to TOL_X_PORT: kernel and host build run the
same statements but sum their reductions in different orders (512 threads against one), so their iterates agree to rounding, not to
the bit -- 1e-4 is the bound tests/test_gpu_table_sharing.py and tests/test_gpu_solver.py hold the two to at equal iteration counts
(measured here: 1.4e-13 after the cold solve, 2.5e-14 .. 1.4e-13 after the steps; never the same bits, before this image or with it).
Bit-equality is what tests/test_gpu_slot_handout.py and `bench.py --dump-outputs` against the parent commit check."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)
N = 12
TOL_X_PORT = 1e-4


def _loop(mpc, steps):
    host = (lambda n: getattr(mpc, n)) if mpc.kind == 'host' else mpc.host
    mpc.solve_cold(bends=())
    out, crossed = [(host('x').copy(), host('status').copy(), host('iters').copy())], 0
    for _ in range(steps):
        crossed += int(bool(mpc.step()))
        out.append((host('x').copy(), host('status').copy(), host('iters').copy()))
    return out, crossed


def test_cold_solve_and_crossing_step_match_the_host_build():
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    problem, P = workloads.holonomic_p2p(N)
    update_time = 0.4 * float(problem.knot_time)            # steps at 0.4, 0.8, 1.2 knot intervals: the third crosses a knot
    ref = BatchP2P(problem, P, ops=port_binding, options=OPTS, update_time=update_time)
    ref.n_threads = 8
    want, crossed_ref = _loop(ref, 3)
    problem_g, P_g = workloads.holonomic_p2p(N)
    gpu = BatchP2P(problem_g, P_g, ops='hip', device=torch.device('cuda', 0), options=OPTS, update_time=update_time)
    try:
        info = gpu.solver.workspace()
        assert info['mode'] in (0, 4, 5)                    # the wave path: the instances that copy the image
        got, crossed = _loop(gpu, 3)
    finally:
        gpu.solver.close()
    assert crossed == crossed_ref == 1
    lo, hi = gpu.tpl.entry_range(gpu.veh.label, 'splines_seg0', 'var')
    for k, ((x, st, it), (xr, st_r, it_r)) in enumerate(zip(got, want)):
        worst = float(np.abs(x[:, lo:hi] - xr[:, lo:hi]).max())
        print('%s: iters %s, max |coefficient diff| %.2e, same bits: %s' % ('cold' if k == 0 else 'step %d' % k, it.tolist(), worst,
                                                                          np.array_equal(x, xr)))
        assert np.array_equal(st, st_r), (k, st, st_r)
        assert np.array_equal(it, it_r), (k, it, it_r)
        assert worst < TOL_X_PORT, (k, worst)
