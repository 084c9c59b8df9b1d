"""The `omgx_batch` handle as one owner of its device memory and of its kernel instances ("Handle: ownership and the
instance table"): a handle that switched on every lazily allocated block and was closed leaves the process as it found it -- a
fresh handle returns the bits of one that never had a feature on --, the instance table holds lean / refine / rollout entries for
the wave-path class only, and a creation that fails half-way leaves nothing behind that a later handle trips over.  Every call
here is one the API defines; the classes and sizes are those of tests/test_gpu_prepare.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)
KEYS = ('x', 'lam_g', 'status', 'iters')


def _plain_cold_and_warm(problem, P, B):
    """A handle with no feature on: a cold solve, then a warm-started one at a moved horizon clock."""
    from omgtools.backend import BatchSolver
    tpl = problem.father.template
    p2 = P['p'].copy()
    p2[:, tpl.entry_range(problem.label, 't', 'par')[0]] += 0.1
    s = BatchSolver(tpl, B, options=OPTS)
    try:
        cold = s.solve(P['p'], P['x0'])
        s.set_options(warm_start=1)
        warm = s.solve(p2, cold['x'], lam_g0=cold['lam_g'], status0=cold['status'])
    finally:
        s.close()
    return cold, warm


@pytest.fixture(scope='module')
def wave_class():
    """holonomic_p2p(16) -- wave path, mode 5, two per CU -- and the plain reference, computed once before any feature is used."""
    from omgtools import workloads
    B = 16
    problem, P = workloads.holonomic_p2p(B)
    return problem, P, B, _plain_cold_and_warm(problem, P, B)


def test_a_handle_with_every_block_switched_on_leaves_nothing_behind(wave_class):
    import torch
    from omgtools.batch import BatchP2P
    problem, P, B, (ref_cold, ref_warm) = wave_class
    assert (ref_cold['status'] == 0).all() and (ref_warm['status'] == 0).all()
    dev = torch.device('cuda', 0)
    mpc = BatchP2P(problem, P, ops='hip', device=dev, options=OPTS)      # update_time 0.1 s, knot_time 1 s: update 10 crosses a knot
    s = mpc.solver
    try:
        assert s.workspace()['mode'] == 5
        f64 = dict(dtype=torch.float64, device=dev)
        out, vt, t0 = torch.zeros((B, 3, mpc.n_dim, 11), **f64), torch.zeros((B, 11), **f64), torch.zeros(B, **f64)
        s.set_prepare(1)                                                   # the setup kernel's records
        s.set_store(out, vt, t0, mpc.o_spl, mpc.n_dim, mpc.basis.degree, mpc.basis.knots, 3, 11, 0.1 / mpc.T, 1.0 / mpc.T)   # the store block
        assert mpc.solve_cold() >= 0                                       # restart guesses inside the launch, prepared setup
        assert s.workspace()['last_instance'] == 0
        mpc.stop_at_arrival(stop_tol=-1.0)                                 # a rule that never holds: every agent solved at every update
        mpc.record_signals(sample_time=0.05, max_updates=16)               # the log, in the same block as the store
        mpc.step()                                                         # update 1
        # a second, different shift-table set through the host-pointer path (which also stages the mask)
        e0 = mpc.shift_entries[:1].copy()
        scratch = mpc.host('x').copy()
        s.shift(scratch, np.ones(B, dtype=np.uint8), e0, mpc.shift_mats[:e0[0, 1] ** 2])
        assert np.isfinite(scratch).all()
        assert mpc.rollout(2) == 0                                         # updates 2-3
        assert mpc.rollout(5) == 0                                         # updates 4-8: a longer step table than before
        assert mpc.rollout(3) == 1                                         # updates 9-11: across the knot, with the loop's own shift set
        torch.cuda.synchronize()
        assert (mpc.host('status') == 0).sum() >= B - 2 and (mpc.host('under_way') == 1).all()
        assert int(mpc._sig['overflow'].sum()) == 0 and int(mpc._sig['count'].min()) > 1
        assert float(out.abs().max()) > 0.1
    finally:
        s.close()
    cold, warm = _plain_cold_and_warm(problem, P, B)
    for k in KEYS:
        assert np.array_equal(cold[k], ref_cold[k]), ('cold', k)
        assert np.array_equal(warm[k], ref_warm[k]), ('warm', k)


@pytest.mark.parametrize('name,B,mode,lean', [('holonomic_p2p', 16, 5, 1), ('quadrotor_p2p', 6, 1, 0), ('holonomic3d_p2p', 5, 3, 0)])
def test_instance_table_of_the_shipped_classes(name, B, mode, lean):
    import torch
    from omgtools import workloads
    from omgtools.backend import BatchSolver, OmgxError
    problem, P = getattr(workloads, name)(B)
    tpl = problem.father.template
    s = BatchSolver(tpl, B, options=dict(tol=1e-3, max_iter=60))
    try:
        assert s.workspace()['mode'] == mode
        s.solve(P['p'], P['x0'])
        assert s.workspace()['last_instance'] == lean
        s.set_options(refine=1)
        s.solve(P['p'], P['x0'])
        assert s.workspace()['last_instance'] == 0
        if not lean:                                                       # the spill classes have no rollout entry: an error, no fallback
            dev = torch.device('cuda', 0)
            f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
            p, x, lam = torch.zeros((B, tpl.n_par), **f64), torch.zeros((B, tpl.n_var), **f64), torch.zeros((B, tpl.n_con), **f64)
            lb, ub = torch.as_tensor(tpl.lb, **f64), torch.as_tensor(tpl.ub, **f64)
            status, iters = torch.zeros(B, **i32), torch.zeros(B, **i32)
            with pytest.raises(OmgxError, match='not available for this template class'):
                s.rollout(p, x, lb, ub, lam, status, iters, [0.05], [0.0], [0], 0, 1, 3, np.r_[np.zeros(4), np.ones(4)], 1.0, [0], 0)
    finally:
        s.close()


@pytest.mark.parametrize('field,words', [('block_off', 'reaches outside'), ('eq_rows', 'equality row')])
def test_a_failed_creation_is_followed_by_a_working_handle(wave_class, monkeypatch, field, words):
    """`block_off`: the template is refused by the argument checks; `eq_rows`: by the plan, after the handle exists -- the one
    failure path of omgx_batch_create, which destroys it.  Both are OMGX_E_INVALID (-1)."""
    import omgtools.backend as be
    problem, P, B, (ref_cold, _) = wave_class
    tpl = problem.father.template
    make = be.make_ctemplate

    def broken(t, plan=None):
        ct, keep = make(t, plan)
        getattr(ct, field)[0] = 10 ** 6                                    # (writes into the array `keep` holds)
        return ct, keep
    monkeypatch.setattr(be, 'make_ctemplate', broken)
    with pytest.raises(be.OmgxError, match=r'\(-1\).*' + words):
        be.BatchSolver(tpl, B, options=OPTS)
    monkeypatch.setattr(be, 'make_ctemplate', make)
    s = be.BatchSolver(tpl, B, options=OPTS)
    try:
        cold = s.solve(P['p'], P['x0'])
    finally:
        s.close()
    for k in KEYS:
        assert np.array_equal(cold[k], ref_cold[k]), k
