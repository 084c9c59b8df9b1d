"""Measured states fed back into the per-step loop on the device (`omgx_batch_predict_measured`, `BatchP2P.step(states=...)`): the
prediction must equal the reference's `Vehicle.predict(state0=...)` and a closed form written here, a loop fed the plant's own
`state_prev` must be the plant's loop bit for bit, agents without a measurement must be predicted as `omgx_batch_predict_ex` predicts
them, and the order workgroup that rides in the launch (block B of a grid of B + 1) must not be taken for an agent."""
import os

import numpy as np
import pytest

from test_feedback_cpu import check_against_feedback_fixture, replay_feedback_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OPTS = dict(tol=1e-3, max_iter=300)
CANARY = 777.0


def _mk(n, workload='holonomic_p2p', cls=None, **kw):
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = getattr(workloads, workload)(n)
    return (cls or BatchP2P)(problem, P, device=torch.device('cuda', 0), options=OPTS, **kw)


def _close(*ms):
    for m in ms:
        if hasattr(m, 'close'):
            m.close()
        else:
            m.solver.close()


def _np(t):
    return t.cpu().numpy()


def test_device_prediction_equals_the_reference():
    """The plans and measurements of tests/golden/feedback_holonomic.npz through `DeviceP2P._feedback_predict` (4 agents): the
    bounds of tests/test_feedback_cpu.py -- inputs 1e-10, states 10 x the reference's own odeint error, both enforce forms exact."""
    import torch
    g, f = np.load(os.path.join(GOLD, 'signals_holonomic.npz')), np.load(os.path.join(GOLD, 'feedback_holonomic.npz'))
    dev = _mk(4)
    assert np.array_equal(np.asarray(dev.basis.knots, dtype=float), g['knots']) and dev.T == float(g['horizon_time'])
    dev.feedback(sample_time=float(g['sample_time']))

    def put(t, a):
        t.copy_(torch.as_tensor(np.ascontiguousarray(a), dtype=t.dtype, device=t.device))

    def feed(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev.dev)
    check_against_feedback_fixture(f, replay_feedback_fixture(dev, g, f, _np, put, feed))
    _close(dev)


@pytest.mark.parametrize('streamed', [False, True])
def test_loop_fed_the_plants_state_is_the_plants_loop(streamed):
    """Loop A: the plant with a disturbance in the loop.  Loop B: feedback, every step fed A's `state_prev` copied before that step.
    The cold solve and 12 steps across the knot crossing, `straggler_first` on (the order workgroup rides in both prediction
    launches): x, p, lam, status, iters hold the same bits after every step.  streamed: B as three sub-batches on their own streams,
    each handed its rows."""
    import torch
    from omgtools.batch import StreamedP2P, input_disturbance
    n = 48 if streamed else 40
    A = _mk(n)
    B = _mk(n, cls=StreamedP2P, n_streams=3) if streamed else _mk(n)
    assert A.straggler_first
    A.plant(sample_time=0.01, max_updates=13, disturbance=input_disturbance(n, 2, 13, 10, 1001, fc=0.1, stdev=0.02, seed=7))
    B.feedback(sample_time=0.01)
    A.solve_cold(bends=())
    B.solve_cold(bends=())
    crossings = 0
    for k in range(12):
        prev = A.plant_state()['state_prev'].clone()
        crossings += int(A.step())
        B.step(states=prev)
        for name in ('x', 'p', 'lam', 'status', 'iters'):
            assert torch.equal(getattr(A, name), getattr(B, name)), (k, name)
    assert crossings == 1
    assert float((A.plant_state()['state'] - A.plant_state()['state_prev']).abs().max()) > 1e-3
    _close(A, B)


def _closed_form(knots, degree, c, t_rel, T, st, n_samp, S, tau):
    """scipy's B-splines, no code shared with the package: measured state + trapezoid sum of the plan's inputs at the samples
    0 .. n_samp; the plan's state and input at tau.  c [B, n_spl, L], t_rel [B]."""
    from scipy.interpolate import BSpline
    s0, ideal, i0 = (np.zeros(S.shape) for _ in range(3))
    for b in range(len(c)):
        spl = BSpline(knots, c[b].T, degree)
        u = spl.derivative()((t_rel[b] + np.arange(n_samp + 1) * st) / T).T / T
        s0[b] = S[b] + st * np.cumsum((u[:, :-1] + u[:, 1:]) / 2.0, axis=1)[:, -1]
        ideal[b], i0[b] = spl(tau), spl.derivative()(tau) / T
    return s0, ideal, i0


def _canary_rows(m):
    """x and p of the loop as the first B rows of tensors with one more row: what a launch that took block B for an agent would read
    and write."""
    import torch
    xf, pf = (torch.cat([t, torch.full_like(t[:1], CANARY)]) for t in (m.x, m.p))
    m.x, m.p = xf[:m.B], pf[:m.B]
    return xf, pf


@pytest.mark.parametrize('n,t_rel,n_samp', [(1, 0.0, 10), (5, 0.0, 10), (5, 0.85, 10), (5, 0.85, 100)])
def test_predict_entry_alone(n, t_rel, n_samp):
    """The entry without a solve, on solved plans of the signals fixture: with a pending launch order (grid B + 1; 1 agent: the second
    block is the order workgroup), t_rel = 0 and a t_rel whose sample grid crosses the knot at T / 11 = 0.909 s inside the update
    (the span is chosen per sample); 100 samples per update: more (spline, sample) pairs than the 64 threads that evaluate them.
    fresh all 1, all 0 and alternating: fresh rows against the closed form (1e-12 state, 1e-10
    input), the others bit for bit what `omgx_batch_predict_ex` writes; the row behind p is untouched and the order is a permutation."""
    import torch
    g = np.load(os.path.join(GOLD, 'signals_holonomic.npz'))
    m = _mk(n)
    st = 0.1 / n_samp
    m.feedback(sample_time=st)
    assert m._fb['n_samp'] == n_samp
    xf, pf = _canary_rows(m)
    knots, T = g['knots'], m.T
    c = np.stack([g['coeffs'][(3 * b + 2) % 12, b % 4] for b in range(n)])
    x = _np(m.x)
    x[:, m.o_spl:m.o_spl + 2 * m.L] = c.reshape(n, -1)
    m.x.copy_(torch.as_tensor(x, device=m.dev))
    p0 = m.p.clone()
    p0[:, m.o_t] = t_rel
    rng = np.random.default_rng(n)
    S = rng.uniform(-2., 2., size=(n, 2))
    tau, t_new = (t_rel + 0.1) / T, t_rel + 0.1
    s0, _, i0 = _closed_form(knots, 3, c, np.full(n, t_rel), T, st, n_samp, S, tau)
    # the ideal prediction, by the entry the plain step uses
    m.p.copy_(p0)
    m._predict(tau, t_new)
    p_ideal = m.p.clone()
    states = torch.as_tensor(S, device=m.dev)
    for fresh in (None, np.zeros(n, dtype=np.int32), (np.arange(n) % 2).astype(np.int32)):
        m.p.copy_(p0)
        m.iters.copy_(torch.arange(n, dtype=torch.int32, device=m.dev) % 3)
        m._order.fill_(-1)
        m._feedback_predict(tau, t_new, states, None, None if fresh is None else torch.as_tensor(fresh, device=m.dev), False)
        torch.cuda.synchronize()
        got = _np(m.p)
        on = np.ones(n, dtype=bool) if fresh is None else fresh != 0
        if on.any():
            err_s = np.abs(got[on, m.o_state0:m.o_state0 + 2] - s0[on]).max()
            err_i = np.abs(got[on, m.o_input0:m.o_input0 + 2] - i0[on]).max()
            print('fresh %s: state0 %.2e input0 %.2e' % (None if fresh is None else fresh.tolist(), err_s, err_i))
            assert err_s <= 1e-12 and err_i <= 1e-10
            keep = np.ones(got.shape[1], dtype=bool)
            keep[[m.o_state0, m.o_state0 + 1, m.o_input0, m.o_input0 + 1, m.o_t]] = False
            assert np.array_equal(got[on][:, keep], _np(p0)[on][:, keep]) and np.array_equal(got[on, m.o_t], np.full(on.sum(), t_new))
        assert torch.equal(m.p[torch.as_tensor(~on, device=m.dev)], p_ideal[torch.as_tensor(~on, device=m.dev)])
        assert sorted(_np(m._order).tolist()) == list(range(n))
        assert bool((pf[n] == CANARY).all()) and bool((xf[n] == CANARY).all())
    _close(m)


def test_predict_entry_on_the_holonomic3d_class():
    """n_spl = 3, another degree / basis length: the bundle's cold plan (the initial guess, its coefficients moved by a seeded
    amount so that the inputs vary over the update) against the scipy closed form, 1e-12 / 1e-10."""
    import torch
    n = 5
    m = _mk(n, workload='holonomic3d_p2p')
    assert m.n_spl == 3
    m.feedback(sample_time=0.01)
    knots, T, deg = np.asarray(m.basis.knots, dtype=float), m.T, m.basis.degree
    interior = knots[(knots > knots[0]) & (knots < knots[-1])]
    t_rel = float(interior[0] * T - 0.05)                   # (the sample grid crosses the first interior knot)
    rng = np.random.default_rng(3)
    x = _np(m.x)
    x[:, m.o_spl:m.o_spl + 3 * m.L] += rng.uniform(-0.5, 0.5, size=(n, 3 * m.L))
    m.x.copy_(torch.as_tensor(x, device=m.dev))
    c = x[:, m.o_spl:m.o_spl + 3 * m.L].reshape(n, 3, m.L)
    m.p[:, m.o_t] = t_rel
    S = rng.uniform(-2., 2., size=(n, 3))
    tau = (t_rel + 0.1) / T
    s0, _, i0 = _closed_form(knots, deg, c, np.full(n, t_rel), T, 0.01, 10, S, tau)
    m._feedback_predict(tau, t_rel + 0.1, torch.as_tensor(S, device=m.dev), None, None, False)
    got = _np(m.p)
    err_s, err_i = np.abs(got[:, m.o_state0:m.o_state0 + 3] - s0).max(), np.abs(got[:, m.o_input0:m.o_input0 + 3] - i0).max()
    print('holonomic3d (degree %d, L %d): state0 %.2e input0 %.2e' % (deg, m.L, err_s, err_i))
    assert err_s <= 1e-12 and err_i <= 1e-10
    _close(m)


def test_pinned_host_measurements_and_the_enforce_forms():
    """Pinned host `states` / `fresh` / `inputs` give the bits device tensors give.  enforce: the rows of p are the given values as
    they are, zeros for an input that was not given, and an agent without a measurement is predicted from its plan."""
    import torch
    n = 6
    m = _mk(n)
    m.feedback(sample_time=0.01)
    m.solve_cold(bends=())
    rng = np.random.default_rng(9)
    S, U = torch.as_tensor(rng.uniform(-2., 2., size=(n, 2))), torch.as_tensor(rng.uniform(-.5, .5, size=(n, 2)))
    F = torch.as_tensor((np.arange(n) % 3 != 0).astype(np.int32))
    p0 = m.p.clone()
    tau, t_new = 0.1 / m.T, 0.1
    m._predict(tau, t_new)
    p_ideal = m.p.clone()
    out = {}
    for where in ('device', 'pinned'):
        s, u, f = ((t.to(m.dev) if where == 'device' else t.pin_memory()) for t in (S, U, F))
        for form, (inputs, enforce) in dict(plain=(None, False), enforce=(None, True), enforce_inputs=(u, True)).items():
            m.p.copy_(p0)
            m._feedback_predict(tau, t_new, s, inputs, f, enforce)
            torch.cuda.synchronize()
            out[where, form] = m.p.clone()
    for form in ('plain', 'enforce', 'enforce_inputs'):
        assert torch.equal(out['device', form], out['pinned', form]), form
    on = F.bool().to(m.dev)
    st, inp = slice(m.o_state0, m.o_state0 + 2), slice(m.o_input0, m.o_input0 + 2)
    assert not torch.equal(out['device', 'plain'][on][:, st], p_ideal[on][:, st])
    for form, want in (('enforce', torch.zeros_like(U)), ('enforce_inputs', U)):
        got = out['device', form]
        assert torch.equal(got[on][:, st], S.to(m.dev)[on]) and torch.equal(got[on][:, inp], want.to(m.dev)[on])
        assert torch.equal(got[~on], p_ideal[~on]) and bool((got[:, m.o_t] == t_new).all())
    with pytest.raises(ValueError):                         # (a pageable host tensor is no address the kernel can read)
        m.solver.predict_measured(m.x, m.p, tau, t_new, S, n_samp=10, sample_time=0.01, p_off=m.p_offs, p_t=m.o_t, **m._plan)
    _close(m)


def test_device_refusals_name_the_field():
    import torch
    from omgtools.backend import OmgxError
    m = _mk(4)
    S = torch.zeros((4, 2), dtype=torch.float64, device=m.dev)
    n_par, n_var = m.tpl.n_par, m.tpl.n_var
    base = dict(m._plan, n_samp=10, sample_time=0.01, p_off=m.p_offs, p_t=m.o_t)
    p0 = m.p.clone()
    for change, word in [(dict(p_off=[n_par - 1, m.o_input0]), 'p_off[0]'), (dict(p_off=[m.o_state0, n_par - 1]), 'p_off[1]'),
                         (dict(p_t=n_par), 'p_t'), (dict(p_t=-1), 'p_t'), (dict(coeff_off=n_var - 2 * m.L + 1), 'coeff_off'),
                         (dict(n_samp=0), 'n_samp'), (dict(p_off=[m.o_state0, m.o_input0, 0, 0, 0]), 'n_out')]:
        with pytest.raises(OmgxError) as e:
            m.solver.predict_measured(m.x, m.p, 0.01, 0.1, S, **dict(base, **change))
        assert 'predict_measured' in str(e.value) and word in str(e.value), (change, str(e.value))
    with pytest.raises(ValueError):
        m.solver.predict_measured(m.x, m.p, 0.01, 0.1, S[:3], **base)
    torch.cuda.synchronize()
    assert torch.equal(m.p, p0)                             # (nothing was launched)
    _close(m)
