"""The plant's first-order actuator lag on the device (`omgx_batch_set_plant_lag`): one out-of-line routine serves the stand-alone
simulate launch and the plant instances of the rollout kernel, so both must write THE SAME BITS; they must equal the reference's
`Vehicle.simulate` with `_ode_1storder` within the recorded error of its odeint, and the host loop's numpy statements; and a loop
that sets no lag, or clears it, must not change."""
import math
import os

import numpy as np
import pytest

from test_plant_lag_cpu import check_against_lag_fixture, fixtures, replay_lag_fixture

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)


def _dist(n, max_updates, stdev=0.02, seed=7):
    from omgtools.batch import input_disturbance
    return input_disturbance(n, 2, max_updates, 10, 1001, fc=0.1, stdev=stdev, seed=seed)


def _taus(n, seed=9):
    """Per-agent time constants drawn from [0.02, 0.5]."""
    return np.random.default_rng(seed).uniform(0.02, 0.5, n)


def _mk(n, max_updates=16, dist='noise', tc='drawn', mutate=None, stop=None, record=True, cold=True, plant=True, cls=None, **kw):
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = workloads.holonomic_p2p(n)
    if mutate is not None:
        mutate(problem, P)
    m = (cls or BatchP2P)(problem, P, device=torch.device('cuda', 0), options=OPTS, **kw)
    if plant:
        m.plant(sample_time=0.01, max_updates=max_updates, disturbance=_dist(n, max_updates) if isinstance(dist, str) else dist,
                time_constant=_taus(n) if isinstance(tc, str) else tc)
    if stop is not None:
        m.stop_at_arrival(stop_tol=stop)
    if record:
        m.record_signals(sample_time=0.01, max_updates=max_updates)
    if cold:
        m.solve_cold(bends=())
    return m


def _drift(problem, P):
    tpl = problem.father.template
    rng = np.random.default_rng(5)
    for obs in problem.environment.obstacles:
        ov, oa = (tpl.entry_range(obs.label, nm, 'par') for nm in ('v', 'a'))
        P['p'][:, ov[0]:ov[1]] = rng.uniform(-0.03, 0.03, size=(len(P['p']), ov[1] - ov[0]))
        P['p'][:, oa[0]:oa[1]] = rng.uniform(-0.01, 0.01, size=(len(P['p']), oa[1] - oa[0]))


def _equal_everywhere(a, b):
    """x, lam, p, status, iters, the log with count and overflow, every plant_state() array: the same bits."""
    import torch
    sa, sb, pa, pb = a.signals(), b.signals(), a.plant_state(), b.plant_state()
    torch.cuda.synchronize()
    for name in ('x', 'lam', 'p', 'status', 'iters'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ('splines', 'count', 'overflow'):
        assert torch.equal(sa[name], sb[name]), name
    for name in pa:
        assert torch.equal(pa[name], pb[name]), name


def _close(*ms):
    for m in ms:
        if hasattr(m, 'close'):
            m.close()
        else:
            m.solver.close()


@pytest.mark.parametrize('chained', [False, True])
def test_stand_alone_kernels_equal_the_reference_and_the_host_glue(chained):
    """The plans of signals_holonomic.npz and the disturbance of plant_holonomic.npz through `omgx_batch_plant_predict / _simulate`
    with the lag of plant_lag_holonomic.npz: the bounds of tests/test_plant_lag_cpu.py against the reference, and the `HostP2P` glue
    on identical inputs within 1e-12 (the bound of tests/test_gpu_plant.py for the plain plant)."""
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    g, p, q = fixtures()
    tc = float(q['time_constant'])
    dev = _mk(4, max_updates=12, dist=p['dist'], tc=tc, cold=False)
    assert np.array_equal(np.asarray(dev.basis.knots, dtype=float), g['knots']) and dev.T == float(g['horizon_time'])

    def get(t):
        return t.cpu().numpy()

    def put(t, a):
        t.copy_(torch.as_tensor(np.ascontiguousarray(a), dtype=t.dtype, device=t.device))
    state0, input0 = replay_lag_fixture(dev, g, q, dev._plant_predict, dev._plant_simulate, chained, get, put)
    sig = {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in dev.signals().items()}
    st = {k: v.cpu().numpy() for k, v in dev.plant_state().items()}
    assert (st['n_upd'] == 12).all() and not st['overflow'].any()
    check_against_lag_fixture(g, p, q, sig, state0, input0, chained)
    # the host glue on identical inputs
    problem, P = workloads.holonomic_p2p(4)
    host = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    host.plant(sample_time=0.01, max_updates=12, disturbance=p['dist'], time_constant=tc)
    host.record_signals(sample_time=0.01, max_updates=12)

    def hput(dst, src):
        dst[...] = src
    h_state0, h_input0 = replay_lag_fixture(host, g, q, host._plant_predict, host._plant_simulate, chained, np.asarray, hput)
    hs, hp = host.signals(), host.plant_state()
    err = max([float(np.abs(sig['splines'] - hs['splines']).max()), float(np.abs(state0[1:] - h_state0[1:]).max()),
               float(np.abs(input0[1:] - h_input0[1:]).max())] + [float(np.abs(st[k] - hp[k]).max()) for k in ('state', 'state_prev', 'input_last')])
    print('device against the host glue: %.2e' % err)
    assert err <= 1e-12 and np.array_equal(sig['count'], hs['count']) and np.array_equal(st['n_upd'], hp['n_upd'])
    _close(dev)


@pytest.mark.parametrize('n,moving', [(40, False), (520, False), (32, True)])
def test_rollout_equals_the_stepwise_loop_bit_for_bit(n, moving):
    """`rollout(12)` against 12 `step()` calls with lag (per-agent time constants from [0.02, 0.5]), disturbance and log on, across
    the knot crossing at t = 1.0: with more agents (520) than the 512 resident workgroups, so the slot hand-out runs, and with
    drifting obstacles."""
    a, b = (_mk(n, mutate=_drift if moving else None) for _ in range(2))
    K = 12
    crossings = a.rollout(K)
    for _ in range(K):
        b.step()
    _equal_everywhere(a, b)
    s, ps = a.signals(), a.plant_state()
    assert crossings == 1 and (s['count'] == 1 + 10 * (K + 1)).all() and not s['overflow'].any()
    assert (ps['n_upd'] == K + 1).all() and not ps['overflow'].any()
    # the lag acted: the last applied input is the last logged one, and not the commanded one of a plant without lag
    cnt = int(s['count'][0])
    assert bool((ps['input_last'] == s['input'][:, :, cnt - 1]).all())
    if moving:
        assert len(a.obst) > 0
    _close(a, b)


def test_streamed_sub_batches_equal_one_handle():
    """`StreamedP2P(n_streams=3)` against one handle, 48 agents, the cold solve and 12 steps: disturbance and per-agent time
    constants sliced per sub-batch, log and plant state concatenated -- the same bits."""
    from omgtools.batch import StreamedP2P
    a = _mk(48, cls=StreamedP2P, n_streams=3)
    b = _mk(48)
    for _ in range(12):
        a.step(); b.step()
    _equal_everywhere(a, b)
    assert (b.plant_state()['n_upd'] == 13).all()
    _close(a, b)


def test_order_of_the_two_registrations_and_clearing():
    """`set_plant_lag` before or after `set_plant`: one `rollout(6)` each gives the same bits.  Setting the lag and clearing it
    (`time_constant=None`) gives the bits of a loop that never set it, and the plain step of a loop without a plant still runs the
    lean solve instance."""
    import torch
    n = 24
    tc = _taus(n)
    dec = np.array([math.exp(-0.01 / t) for t in tc])
    # a: the lag is handed over by plant(), ahead of the first set_plant (the rollout registers the plant).  b: the plant is
    # registered first, with the lag off, the lag afterwards -- and the rollout does not register the plant again
    a, b = _mk(n), _mk(n, cold=False)
    b.solver.set_plant_lag(None)
    b.solver.set_plant(b._plant_args(), b._plant_log_args())
    b.solver.set_plant_lag(tc, dec, 0.01)
    b.solve_cold(bends=())
    b._plant_rollout = lambda: None
    a.rollout(6)
    b.rollout(6)
    _equal_everywhere(a, b)
    assert float((a.signals()['input'] - _plain_inputs(n)).abs().max()) > 1e-4      # (and the lag was on in both)
    _close(a, b)
    # set and cleared against never set
    c, d = _mk(n, tc=None, cold=False), _mk(n, tc=None, cold=False)
    c.plant(sample_time=0.01, max_updates=16, disturbance=_dist(n, 16), time_constant=tc)
    c.plant(sample_time=0.01, max_updates=16, disturbance=_dist(n, 16), time_constant=None)
    for m in (c, d):
        m.solve_cold(bends=())
        m.step()
        m.rollout(5)
    _equal_everywhere(c, d)
    assert c.solver.workspace()['last_instance'] == d.solver.workspace()['last_instance'] == 1      # (no stop rule, no fused log: lean)
    _close(c, d)
    e = _mk(n, plant=False, record=False, cold=False)
    e.plant(sample_time=0.01, max_updates=16, time_constant=0.1)
    e.plant(on=False)
    e.solve_cold(bends=())
    e.step()
    torch.cuda.synchronize()
    assert e.solver.workspace()['last_instance'] == 1
    _close(e)


def _clock(m, K):
    from omgtools.splines import step_clock
    out, t = [], m.time
    for _ in range(K):
        t, tau, t_rel, crossed = step_clock(t, m.update_time, m.knot_time, m.T)
        out.append((tau, t_rel, crossed))
    return out


def _plain_inputs(n):
    """The logged inputs of the same loop without the lag, after the cold solve and a rollout of 6."""
    m = _mk(n, tc=None)
    m.rollout(6)
    out = m.signals()['input'].clone()
    _close(m)
    return out


STOP_TOL, NEAR, MAX_STEPS = 1e-3, (0, 5, 10, 15), 100      # (with a time constant of 0.3 s the four arrive after some 75 updates, not 23)


def _near_targets(problem, P):
    """poseT of four agents moved to 0.3 m from their start: they arrive within the run (the construction of tests/test_gpu_plant.py)."""
    tpl = problem.father.template
    label = problem.vehicles[0].label
    s0, pT = (tpl.entry_range(label, nm, 'par')[0] for nm in ('state0', 'poseT'))
    for b in NEAR:
        d = P['p'][b, pT:pT + 2] - P['p'][b, s0:s0 + 2]
        P['p'][b, pT:pT + 2] = P['p'][b, s0:s0 + 2] + 0.3 * d / np.linalg.norm(d)
        L = len(problem.vehicles[0].basis)
        o_spl = tpl.entry_range(label, 'splines_seg0', 'var')[0]
        for k in range(2):      # (the initial guess on the straight line to the new target)
            P['x0'][b, o_spl + k * L:o_spl + (k + 1) * L] = np.linspace(P['p'][b, s0 + k], P['p'][b, pT + k], L)


def _meets(state, inp, pose, tol):
    return (np.sqrt(((state - pose) ** 2).sum(axis=-1)) <= tol) & (np.sqrt((inp ** 2).sum(axis=-1)) <= tol)


def test_stop_rule_on_the_lagged_input():
    """16 agents, four of them with a target 0.3 m away, time constant 0.3, a disturbance during the first five updates, the stop rule
    on.  Stepwise: an agent stops at the first update where the criterion holds on its last logged column -- travelled state and
    LAGGED input (a relative 1e-9 for the order of the squares) --, a lagged input that has not decayed keeps it running.  The
    rollout stops every agent at the same update."""
    import torch
    n = 16
    dist = _dist(n, MAX_STEPS + 1, stdev=0.02)
    dist[:, :, 5:, :] = 0.
    a, b = (_mk(n, max_updates=MAX_STEPS + 1, dist=dist, tc=0.3, mutate=_near_targets, stop=STOP_TOL) for _ in range(2))
    o_pose = b.tpl.entry_range(b.veh.label, 'poseT', 'par')[0]
    pose = b.p[:, o_pose:o_pose + 2].cpu().numpy()
    stopped_at, held_back = {}, 0
    for k in range(1, MAX_STEPS + 1):
        s = b.signals()
        cnt = s['count'].cpu().numpy()
        idx = np.arange(n)
        last_state, last_in = s['state'].cpu().numpy()[idx, :, cnt - 1], s['input'].cpu().numpy()[idx, :, cnt - 1]
        assert np.array_equal(last_in, b.plant_state()['input_last'].cpu().numpy())
        b.step()
        uw, cnt2 = b.under_way.cpu().numpy(), b.signals()['count'].cpu().numpy()
        for q in range(n):
            if q in stopped_at:
                assert uw[q] == 0 and cnt2[q] == cnt[q], (q, k)
            elif uw[q] == 0:                        # stopped at this update: the criterion held on its last logged column
                assert _meets(last_state[q], last_in[q], pose[q], STOP_TOL * (1 + 1e-9)), (q, k)
                assert cnt2[q] == cnt[q]
                stopped_at[q] = k
            else:                                   # under way: it did not hold, and the update was logged
                assert not _meets(last_state[q], last_in[q], pose[q], STOP_TOL * (1 - 1e-9)), (q, k)
                assert cnt2[q] == cnt[q] + 10
                # (at the target already, and kept running by the lagged input alone)
                held_back += int(_meets(last_state[q], 0. * last_in[q], pose[q], STOP_TOL * (1 - 1e-9)))
        if all(q in stopped_at for q in NEAR):
            break
    print('stopped at update:', stopped_at, '; updates run at the target because of the lagged input:', held_back)
    assert all(q in stopped_at for q in NEAR), stopped_at
    assert held_back > 0
    K = k
    done = 0
    while done < K:                                 # (the same updates in launches of at most 20 steps)
        a.rollout(min(20, K - done))
        done += min(20, K - done)
    torch.cuda.synchronize()
    assert torch.equal(a.under_way, b.under_way)
    sa, sb = a.signals(), b.signals()
    assert torch.equal(sa['count'], sb['count']) and torch.equal(sa['splines'], sb['splines'])
    for name in ('x', 'lam', 'status'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name, v in a.plant_state().items():
        assert torch.equal(v, b.plant_state()[name]), name
    _close(a, b)


def test_a_plant_with_another_sample_time_is_refused():
    """The lag was set with sample_time 0.01: a plant of 0.02 is refused by the stand-alone entry, by the registration and by the
    rollout, nothing is launched (x, p, the plant's arrays and the log stay as they are), and the loop carries on afterwards."""
    import torch
    from omgtools.backend import OmgxError
    n = 8
    m = _mk(n)
    m.step()
    torch.cuda.synchronize()
    keep = dict((nm, getattr(m, nm).clone()) for nm in ('x', 'p', 'lam'))
    keep.update((nm, v.clone()) for nm, v in m.plant_state().items())
    keep['log'] = m.signals()['splines'].clone()
    other = dict(m._plant_args(), sample_time=0.02)
    with pytest.raises(OmgxError) as e:
        m.solver.plant_simulate(m.x, m.p, other, None)
    assert 'sample_time' in str(e.value)
    with pytest.raises(OmgxError) as e:
        m.solver.set_plant(other, None)
    assert 'sample_time' in str(e.value)
    # the rollout: the plant registered with the lag's sample time, the lag then set again with another one
    m.solver.set_plant(m._plant_args(), m._plant_log_args())
    tc = _taus(n)
    m.solver.set_plant_lag(tc, np.array([math.exp(-0.02 / t) for t in tc]), 0.02)
    with pytest.raises(OmgxError) as e:
        m.solver.rollout(m.p, m.x, m.lb, m.ub, m.lam, m.status, m.iters, *zip(*_clock(m, 2)), p_off=m.p_offs, p_t=m.o_t, obstacles=m.obst,
                         dt=m.update_time, shift_entries=m.shift_entries, shift_T=m.shift_mats, lam_perm=m.perm,
                         cross_options=m.cross_options or None, **m._plan)
    assert 'sample_time' in str(e.value) and 'rollout' in str(e.value)
    with pytest.raises(OmgxError):
        m.rollout(2)                                  # (and through the loop: the registration of the plant is refused)
    torch.cuda.synchronize()
    for nm in ('x', 'p', 'lam'):
        assert torch.equal(getattr(m, nm), keep[nm]), nm
    for nm, v in m.plant_state().items():
        assert torch.equal(v, keep[nm]), nm
    assert torch.equal(m.signals()['splines'], keep['log'])
    m.solver.set_plant_lag(tc, np.array([math.exp(-0.01 / t) for t in tc]), 0.01)
    m.rollout(2)
    torch.cuda.synchronize()
    assert (m.plant_state()['n_upd'] == 4).all()
    _close(m)
