"""The travelled-trajectory log on the device (`omgx_batch_set_signals`, `omgx_batch_signals_append`, `omgx_batch_signals_reduce`):
one routine appends the samples a vehicle travels after every update -- stand-alone, from the epilogue of the solve kernel and from
inside the step loop of the rollout kernel -- so the three must write THE SAME BITS, the log must equal the reference's
`vehicle.signals`, and switching it on must not change a solve."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'signals_holonomic.npz')
OPTS = dict(tol=1e-3, max_iter=300)


def _mk(n, record=True, max_updates=16, mutate=None, stop=False, bends=(), cold=True, **kw):
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = workloads.holonomic_p2p(n, **kw)
    if mutate is not None:
        mutate(problem, P)
    m = BatchP2P(problem, P, ops='hip', device=torch.device('cuda', 0), options=OPTS)
    if stop:
        m.stop_at_arrival()
    if record:
        m.record_signals(sample_time=0.01, max_updates=max_updates)
    if cold:
        m.solve_cold(bends=bends)
    return m


def _same_log(a, b):
    import torch
    sa, sb = a.signals(), b.signals()
    torch.cuda.synchronize()
    return torch.equal(sa['splines'], sb['splines']) and torch.equal(sa['count'], sb['count']) and torch.equal(sa['overflow'], sb['overflow'])


def _drift(problem, P):
    tpl = problem.father.template
    rng = np.random.default_rng(5)
    for obs in problem.environment.obstacles:
        ov, oa = (tpl.entry_range(obs.label, nm, 'par') for nm in ('v', 'a'))
        P['p'][:, ov[0]:ov[1]] = rng.uniform(-0.03, 0.03, size=(len(P['p']), ov[1] - ov[0]))
        P['p'][:, oa[0]:oa[1]] = rng.uniform(-0.01, 0.01, size=(len(P['p']), oa[1] - oa[0]))


def test_stand_alone_append_equals_the_reference_signals():
    """The plans of tests/golden/signals_holonomic.npz (four agents, 12 updates, one knot crossing) through
    `omgx_batch_signals_append`: the reference's `Holonomic.store` + `Vehicle.simulate` within 1e-10."""
    import torch
    g = np.load(GOLD)
    m = _mk(4, max_updates=12, cold=False)
    assert np.array_equal(np.asarray(m.basis.knots, dtype=float), g['knots']) and m.T == float(g['horizon_time'])
    for k in range(12):
        m.x[:, m.o_spl:m.o_spl + 2 * m.L] = torch.as_tensor(g['coeffs'][k].reshape(4, -1), dtype=torch.float64, device=m.dev)
        m.p[:, m.o_t] = float(g['t_rel'][k])
        m._signals_append_now()
    s = m.signals()
    torch.cuda.synchronize()
    assert (s['count'] == 121).all() and not s['overflow'].any()
    err = max(float(np.abs(s[nm].cpu().numpy() - g[nm]).max()) for nm in ('state', 'input', 'dinput'))
    print('stand-alone append vs reference: %.3e' % err)
    assert err <= 1e-10
    m.solver.close()


def test_fused_log_equals_the_stand_alone_append_bit_for_bit():
    """16 agents, the cold solve and 12 steps with the log written by the solve kernel's epilogue; x and p after every update
    replayed through the stand-alone kernel."""
    import torch
    m = _mk(16)
    snaps = [(m.x.clone(), m.p.clone())]
    crossed = 0
    for _ in range(12):
        crossed += int(m.step())
        snaps.append((m.x.clone(), m.p.clone()))
    s = m.signals()
    log2, cnt2, ovf2 = torch.zeros_like(s['splines']), torch.zeros_like(s['count']), torch.zeros_like(s['overflow'])
    for x, p in snaps:
        m.solver.signals_append(x, p, log2, cnt2, ovf2, **m._signals_args())
    torch.cuda.synchronize()
    assert crossed == 1 and (s['count'] == 1 + 10 * 13).all() and float(s['splines'].abs().max()) > 0.1
    assert torch.equal(s['splines'], log2) and torch.equal(s['count'], cnt2) and not ovf2.any() and not s['overflow'].any()
    m.solver.close()


@pytest.mark.parametrize('n,moving', [(40, False), (1024, False), (32, True)])
def test_rollout_log_equals_the_stepwise_log_bit_for_bit(n, moving):
    """Every step of every agent logged inside ONE launch: log, count and overflow of `rollout(12)` are those of 12 `step()` calls --
    across the knot crossing, with more agents than resident workgroups, with moving obstacles."""
    import torch
    a, b = (_mk(n, mutate=_drift if moving else None) for _ in range(2))
    K = 12
    a.rollout(K)
    for _ in range(K):
        b.step()
    torch.cuda.synchronize()
    for name in ('x', 'lam', 'p', 'status', 'iters'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert _same_log(a, b)
    s = a.signals()
    assert (s['count'] == 1 + 10 * (K + 1)).all() and not s['overflow'].any()
    a.solver.close(); b.solver.close()


def _criterion(state, inp, pose, tol):
    return (np.linalg.norm(state - pose, axis=-1) <= tol * (1 + 1e-9)) & (np.linalg.norm(inp, axis=-1) <= tol * (1 + 1e-9))


def test_a_whole_manoeuvre_in_one_launch_leaves_its_whole_log():
    """64 vehicles with the stop rule, `rollout(130)`: every vehicle arrives, at different updates; the last logged column of each meets
    the reference's criterion (relative 1e-9 for two evaluation routines of one polynomial), the one before its last update does not;
    the log equals that of 130 `step()` calls bit for bit."""
    import torch
    n, K = 64, 130
    a, b = (_mk(n, max_updates=K + 1, stop=True, bends=(1.0, -1.0, 2.5, -2.5)) for _ in range(2))
    a.rollout(K)
    for _ in range(K):
        b.step()
    torch.cuda.synchronize()
    s = a.signals()
    count = s['count'].cpu().numpy()
    print('columns per agent: min %d max %d, under way: %d' % (count.min(), count.max(), int(a.under_way.sum())))
    assert not a.under_way.any() and not b.under_way.any()
    assert len(set(count.tolist())) >= 2 and ((count - 1) % 10 == 0).all() and not s['overflow'].any()
    assert _same_log(a, b) and torch.equal(a.under_way, b.under_way)
    o_pose = a.tpl.entry_range(a.veh.label, 'poseT', 'par')[0]
    pose = a.p[:, o_pose:o_pose + 2].cpu().numpy()
    st, inp = s['state'].cpu().numpy(), s['input'].cpu().numpy()
    idx = np.arange(n)
    assert _criterion(st[idx, :, count - 1], inp[idx, :, count - 1], pose, a.stop_tol).all()
    assert not _criterion(st[idx, :, count - 11], inp[idx, :, count - 11], pose, a.stop_tol).any()      # (still under way one update earlier)
    a.solver.close(); b.solver.close()


def test_the_log_changes_no_solve():
    """x, lam, p, status, iters after 12 steps, and after `rollout(12)`, with the log on and off: the same bits."""
    import torch
    on_s, off_s, on_r, off_r = (_mk(40, record=rec) for rec in (True, False, True, False))
    for _ in range(12):
        on_s.step(); off_s.step()
    on_r.rollout(12); off_r.rollout(12)
    torch.cuda.synchronize()
    for name in ('x', 'lam', 'p', 'status', 'iters'):
        assert torch.equal(getattr(on_s, name), getattr(off_s, name)), name
        assert torch.equal(getattr(on_r, name), getattr(off_r, name)), name
        assert torch.equal(getattr(on_r, name), getattr(on_s, name)), name
    # the fused store and the fused log together: both written, the solves unchanged; the log off again: only the store
    both = _mk(40)
    f64 = dict(dtype=torch.float64, device=both.dev)
    out, t0 = torch.zeros((40, 3, 2, 101), **f64), torch.zeros(40, **f64)
    both.solver.set_store(out, None, t0, both.o_spl, 2, both.basis.degree, both.basis.knots, 3, 101, 0.1 / both.T, 1.0 / both.T)
    for _ in range(12):
        both.step()
    torch.cuda.synchronize()
    assert torch.equal(both.x, on_s.x) and torch.equal(both.lam, on_s.lam) and _same_log(both, on_s) and float(out.abs().max()) > 0.1
    sig = both.signals()
    kept_log, kept_count = sig['splines'].clone(), sig['count'].clone()
    both.record_signals(on=False)
    out.zero_()
    both.step(); on_s.step()
    torch.cuda.synchronize()
    assert torch.equal(both.x, on_s.x) and float(out.abs().max()) > 0.1
    assert torch.equal(sig['splines'], kept_log) and torch.equal(sig['count'], kept_count)      # (switched off: no longer written)
    both.solver.set_store(None)
    for m in (on_s, off_s, on_r, off_r, both):
        m.solver.close()


def test_an_overflowing_log_writes_nothing_outside_its_columns():
    """The log of 16 agents inside a buffer of sentinels -- one more agent block and a tail behind it --, one column short of the third
    update: the stand-alone kernel, the solve kernel and the rollout kernel drop the append (overflow set, count kept), the columns
    beyond count and everything behind the log keep the sentinel."""
    import torch
    B, cap, SENT = 16, 1 + 10 * 3 - 1, -7.25
    m = _mk(B, record=False)
    blk = 3 * 2 * cap
    buf = torch.full(((B + 1) * blk + 64,), SENT, dtype=torch.float64, device=m.dev)
    log = buf[:B * blk].view(B, 3, 2, cap)
    count, ovf = (torch.zeros(B, dtype=torch.int32, device=m.dev) for _ in range(2))
    args = dict(coeff_off=m.o_spl, n_spl=2, degree=m.basis.degree, knots=m.basis.knots, n_samp=10, p_t=m.o_t, sample_time=0.01, inv_T=1.0 / m.T)
    m.solver.signals_append(m.x, m.p, log, count, ovf, **args)                 # 11 columns
    m.solver.set_signals(log, count, ovf, **args)
    m.step()                                                                   # 21
    torch.cuda.synchronize()
    assert (count == 21).all() and not ovf.any() and (log[..., :21] != SENT).all() and (log[..., 21:] == SENT).all()
    kept = log.clone()
    m.step()                                                                   # the solve kernel: 31 > 30
    torch.cuda.synchronize()
    assert (ovf == 1).all() and (count == 21).all() and torch.equal(log, kept)
    ovf.zero_()
    m.solver.signals_append(m.x, m.p, log, count, ovf, **args)                 # the stand-alone kernel
    torch.cuda.synchronize()
    assert (ovf == 1).all() and (count == 21).all() and torch.equal(log, kept)
    ovf.zero_()
    m.rollout(3)                                                               # the rollout kernel, every step
    torch.cuda.synchronize()
    assert (ovf == 1).all() and (count == 21).all() and torch.equal(log, kept)
    assert (buf[B * blk:] == SENT).all()
    m.solver.set_signals(None)
    from omgtools.backend import OmgxError
    with pytest.raises(OmgxError):                                             # cap below the first append: refused by the library
        m.solver.set_signals(log[..., :10].contiguous(), count, ovf, **args)
    m.solver.close()


def test_summary_against_numpy_on_the_downloaded_log():
    """`omgx_batch_signals_reduce` on the log of a whole manoeuvre (64 vehicles, stop rule, one rollout; about 1300 columns each):
    columns, motion time and the maxima exact, the path length within 1e-12 relative (n * eps = 1.4e-13 for 1300 positive terms, with
    room for the other summation order)."""
    import torch
    n, K = 64, 130
    m = _mk(n, max_updates=K + 1, stop=True, bends=(1.0, -1.0, 2.5, -2.5))
    m.rollout(K)
    sm = m.summary().cpu().numpy()
    s = m.signals()
    torch.cuda.synchronize()
    log, count = s['splines'].cpu().numpy(), s['count'].cpu().numpy()
    o_pose = m.tpl.entry_range(m.veh.label, 'poseT', 'par')[0]
    pose = m.p[:, o_pose:o_pose + 2].cpu().numpy()

    def norms(a):                                   # [2, c] -> [c]: each square and the sum rounded on its own
        return np.sqrt(a[0] * a[0] + a[1] * a[1])
    worst = 0.0
    for b in range(n):
        c = int(count[b])
        st, inp, din = (log[b, o, :, :c] for o in range(3))
        assert sm[b, 0] == c and sm[b, 1] == (c - 1) * 0.01
        assert sm[b, 3] == norms(inp).max() and sm[b, 4] == norms(din).max(), b
        assert sm[b, 5] == norms(st[:, -1:] - pose[b][:, None])[0] and sm[b, 6] == norms(inp[:, -1:])[0] and sm[b, 7] == 0.0
        path = norms(np.diff(st, axis=1)).sum()
        worst = max(worst, abs(sm[b, 2] - path) / path)
    print('path length: largest relative difference %.3e' % worst)
    assert worst <= 1e-12 and sm[:, 2].min() > 0.5
    m.solver.close()


def test_spill_class_logs_on_the_per_step_path():
    """Quadrotor (degree 4, KKT store in a slab): state, dstate, ddstate of 8 agents logged by the solve kernel's epilogue equal the
    stand-alone append bit for bit; `rollout` still refuses the class."""
    import torch
    from omgtools import workloads
    from omgtools.backend import OmgxError
    from omgtools.batch import BatchP2P
    problem, P = workloads.quadrotor_p2p(8)
    q = BatchP2P(problem, P, ops='hip', device=torch.device('cuda', 0), options=dict(P['solver_options'], tol=1e-3, max_iter=300))
    q.record_signals(sample_time=0.01, max_updates=8)
    q.solve_cold()
    snaps = [(q.x.clone(), q.p.clone())]
    for _ in range(6):
        q.step()
        snaps.append((q.x.clone(), q.p.clone()))
    s = q.signals()
    assert s['splines'].shape[1] == 3 and 'state' not in s
    log2, cnt2, ovf2 = torch.zeros_like(s['splines']), torch.zeros_like(s['count']), torch.zeros_like(s['overflow'])
    for x, p in snaps:
        q.solver.signals_append(x, p, log2, cnt2, ovf2, **q._signals_args())
    torch.cuda.synchronize()
    assert (s['count'] == 71).all() and float(s['splines'].abs().max()) > 0.1
    assert torch.equal(s['splines'], log2) and torch.equal(s['count'], cnt2)
    with pytest.raises(OmgxError):
        q.rollout(2)
    q.solver.close()


def test_three_sub_batches_give_the_same_log():
    """`StreamedP2P.record_signals / signals / summary`: the sub-batches' logs concatenated equal the log of one `BatchP2P`."""
    import torch
    from omgtools import workloads
    from omgtools.batch import StreamedP2P
    n = 64
    one = _mk(n)
    problem, P = workloads.holonomic_p2p(n)
    three = StreamedP2P(problem, P, n_streams=3, device=torch.device('cuda', 0), options=OPTS)
    three.record_signals(sample_time=0.01, max_updates=16)
    three.solve_cold(bends=())
    for _ in range(11):
        one.step(); three.step()
    sa, sb = one.signals(), three.signals()
    ma, mb = one.summary(), three.summary()
    torch.cuda.synchronize()
    assert (sa['count'] == 121).all()
    for key in ('splines', 'count', 'overflow', 'state', 'input', 'dinput'):
        assert torch.equal(sa[key], sb[key]), key
    assert torch.equal(ma, mb) and np.array_equal(sa['time'], sb['time'])
    one.solver.close(); three.close()
