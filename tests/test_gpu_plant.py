"""The plant in the loop on the device (`omgx_batch_plant_simulate`, `omgx_batch_plant_predict`, `omgx_batch_set_plant`): the
simulated vehicle of the reference's default options with an input disturbance.  One pair of routines serves the stand-alone
launches and the plant instance of the rollout kernel, so both must write THE SAME BITS; they must equal the reference's
`Vehicle.simulate` / `Vehicle.predict` and the host loop's numpy statements; and a loop that never asks for a plant must not change."""
import os

import numpy as np
import pytest

from test_plant_cpu import check_against_fixture, plan_inputs, replay_fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
OPTS = dict(tol=1e-3, max_iter=300)


def _dist(n, max_updates, stdev=0.02, seed=7):
    from omgtools.batch import input_disturbance
    return input_disturbance(n, 2, max_updates, 10, 1001, fc=0.1, stdev=stdev, seed=seed)


def _mk(n, max_updates=16, dist='noise', mutate=None, stop=None, record=True, cold=True, plant=True, cls=None, build=None, **kw):
    """build(n) -> (problem, P): another class than config 2 (tests/test_gpu_workspace_cells.py)."""
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = (build or workloads.holonomic_p2p)(n)
    if mutate is not None:
        mutate(problem, P)
    m = (cls or BatchP2P)(problem, P, device=torch.device('cuda', 0), options=OPTS, **kw)
    if plant:
        m.plant(sample_time=0.01, max_updates=max_updates, disturbance=_dist(n, max_updates) if isinstance(dist, str) else dist)
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
    """The plans and the disturbance of tests/golden/plant_holonomic.npz through `omgx_batch_plant_predict / _simulate`: the three
    bounds of tests/test_plant_cpu.py against the reference, and the `HostP2P` glue on identical inputs within 1e-12."""
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    from oracle import port_binding
    g, p = np.load(os.path.join(GOLD, 'signals_holonomic.npz')), np.load(os.path.join(GOLD, 'plant_holonomic.npz'))
    dev = _mk(4, max_updates=12, dist=p['dist'], cold=False)
    assert np.array_equal(np.asarray(dev.basis.knots, dtype=float), g['knots']) and dev.T == float(g['horizon_time'])

    def get(t):
        return t.cpu().numpy()

    def put(t, a):
        t.copy_(torch.as_tensor(np.ascontiguousarray(a), dtype=t.dtype, device=t.device))
    state0, input0 = replay_fixture(dev, g, p, dev._plant_predict, dev._plant_simulate, chained, get, put)
    sig = {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in dev.signals().items()}
    st = {k: v.cpu().numpy() for k, v in dev.plant_state().items()}
    assert (st['n_upd'] == 12).all() and not st['overflow'].any()
    check_against_fixture(g, p, sig, state0, input0, chained)
    # the host glue on identical inputs
    problem, P = workloads.holonomic_p2p(4)
    host = BatchP2P(problem, P, ops=port_binding, options=OPTS)
    host.plant(sample_time=0.01, max_updates=12, disturbance=p['dist'])
    host.record_signals(sample_time=0.01, max_updates=12)

    def hput(dst, src):
        dst[...] = src
    h_state0, h_input0 = replay_fixture(host, g, p, host._plant_predict, host._plant_simulate, chained, np.asarray, hput)
    hs, hp = host.signals(), host.plant_state()
    err = max([float(np.abs(sig['splines'] - hs['splines']).max()), float(np.abs(state0[1:] - h_state0[1:]).max()),
               float(np.abs(input0[1:] - h_input0[1:]).max())] + [float(np.abs(st[k] - hp[k]).max()) for k in ('state', 'state_prev', 'input_last')])
    print('device against the host glue: %.2e' % err)
    assert err <= 1e-12 and np.array_equal(sig['count'], hs['count']) and np.array_equal(st['n_upd'], hp['n_upd'])
    _close(dev)


@pytest.mark.parametrize('n,moving', [(40, False), (520, False), (32, True)])
def test_rollout_equals_the_stepwise_loop_bit_for_bit(n, moving):
    """`rollout(12)` against 12 `step()` calls with the plant and the log on, across the knot crossing at t = 1.0: with more agents
    (520) than the 512 resident workgroups, so the slot hand-out runs, and with drifting obstacles."""
    import torch
    a, b = (_mk(n, mutate=_drift if moving else None) for _ in range(2))
    K = 12
    crossings = a.rollout(K)
    for _ in range(K):
        b.step()
    _equal_everywhere(a, b)
    s, ps = a.signals(), a.plant_state()
    assert crossings == 1 and (s['count'] == 1 + 10 * (K + 1)).all() and not s['overflow'].any()
    assert (ps['n_upd'] == K + 1).all() and not ps['overflow'].any()
    if moving:
        assert len(a.obst) > 0
    _close(a, b)


def test_streamed_sub_batches_equal_one_handle():
    """`StreamedP2P(n_streams=3)` against one handle, 48 agents, the cold solve and 12 steps: the disturbance sliced per sub-batch,
    log and plant state concatenated -- the same bits."""
    from omgtools.batch import StreamedP2P
    a = _mk(48, cls=StreamedP2P, n_streams=3)
    b = _mk(48)
    for _ in range(12):
        a.step(); b.step()
    _equal_everywhere(a, b)
    assert (b.plant_state()['n_upd'] == 13).all()
    _close(a, b)


def test_feedback_identity_on_the_device():
    """16 agents, plant state and p around every step.  The state a solve starts from is the state the vehicle had one update ago plus
    the nominal trapezoid of the plan travelled since (scipy's B-splines, a cumulative sum written here): 1e-12; the logged input
    columns minus the plan's own inputs are the disturbance that was supplied: 1e-12."""
    import torch
    n, K = 16, 12
    dist = _dist(n, K + 1)
    m = _mk(n, max_updates=K + 1, dist=dist)
    knots, T, st = np.asarray(m.basis.knots, dtype=float), m.T, 0.01
    lo, nn = m.o_spl, 2 * m.L
    worst_fb, worst_in = 0.0, 0.0
    for k in range(K + 1):
        x, t_rel = m.x.cpu().numpy(), m.p[:, m.o_t].cpu().numpy()
        u = np.stack([plan_inputs(knots, x[b, lo:lo + nn].reshape(2, m.L), float(t_rel[b]), T, st, 10) for b in range(n)])
        logged = m.signals()['input'][:, :, 1 + 10 * k:11 + 10 * k].cpu().numpy()
        worst_in = max(worst_in, float(np.abs(logged - u[..., 1:] - dist[:, :, k, 1:]).max()))
        if k == K:
            break
        prev = m.plant_state()['state_prev'].cpu().numpy()
        m.step()
        state0 = m.p[:, m.o_state0:m.o_state0 + 2].cpu().numpy()
        worst_fb = max(worst_fb, float(np.abs(prev + st * np.cumsum((u[..., :-1] + u[..., 1:]) / 2.0, axis=-1)[..., -1] - state0).max()))
    print('state0 against state_prev + nominal trapezoid: %.2e; logged input - plan - disturbance: %.2e' % (worst_fb, worst_in))
    assert worst_fb <= 1e-12 and worst_in <= 1e-12
    assert float(np.abs(dist).max()) > 1e-3
    _close(m)


STOP_TOL, NEAR, MAX_STEPS = 1e-3, (0, 5, 10, 15), 60


def _near_targets(problem, P, agents=NEAR):
    """poseT of four agents moved to 0.3 m from their start: they arrive within the run."""
    tpl = problem.father.template
    label = problem.vehicles[0].label
    s0, pT = (tpl.entry_range(label, nm, 'par')[0] for nm in ('state0', 'poseT'))
    for b in agents:
        d = P['p'][b, pT:pT + 2] - P['p'][b, s0:s0 + 2]
        P['p'][b, pT:pT + 2] = P['p'][b, s0:s0 + 2] + 0.3 * d / np.linalg.norm(d)
        L = len(problem.vehicles[0].basis)
        o_spl = tpl.entry_range(label, 'splines_seg0', 'var')[0]
        for k in range(2):      # (the initial guess on the straight line to the new target)
            P['x0'][b, o_spl + k * L:o_spl + (k + 1) * L] = np.linspace(P['p'][b, s0 + k], P['p'][b, pT + k], L)


def _meets(state, inp, pose, tol):
    return (np.sqrt(((state - pose) ** 2).sum(axis=-1)) <= tol) & (np.sqrt((inp ** 2).sum(axis=-1)) <= tol)


def test_stop_rule_on_the_travelled_state():
    """16 agents, four of them with a target 0.3 m away, a disturbance during the first five updates, the stop rule on.  Stepwise: an
    agent's log stops growing at the first update where the criterion holds on its last logged column (travelled state, applied
    input; a relative 1e-9 for the order of the squares), `under_way` is 0 from then on, plan and multipliers stay bit-identical.
    The rollout stops every agent at the same update."""
    import torch
    n = 16
    dist = _dist(n, MAX_STEPS + 1, stdev=0.02)
    dist[:, :, 5:, :] = 0.
    a, b = (_mk(n, max_updates=MAX_STEPS + 1, dist=dist, mutate=_near_targets, stop=STOP_TOL) for _ in range(2))
    o_pose = b.tpl.entry_range(b.veh.label, 'poseT', 'par')[0]
    pose = b.p[:, o_pose:o_pose + 2].cpu().numpy()
    stopped_at, frozen = {}, {}
    for k in range(1, MAX_STEPS + 1):
        s = b.signals()
        cnt = s['count'].cpu().numpy()
        idx = np.arange(n)
        last_state, last_in = s['state'].cpu().numpy()[idx, :, cnt - 1], s['input'].cpu().numpy()[idx, :, cnt - 1]
        b.step()
        uw, cnt2 = b.under_way.cpu().numpy(), b.signals()['count'].cpu().numpy()
        for q in range(n):
            if q in stopped_at:
                assert uw[q] == 0 and cnt2[q] == cnt[q], (q, k)
                assert torch.equal(b.x[q], frozen[q][0]) and torch.equal(b.lam[q], frozen[q][1]), (q, k)
            elif uw[q] == 0:                        # stopped at this update: the criterion held on its last logged column
                assert _meets(last_state[q], last_in[q], pose[q], STOP_TOL * (1 + 1e-9)), (q, k)
                assert cnt2[q] == cnt[q]
                stopped_at[q], frozen[q] = k, (b.x[q].clone(), b.lam[q].clone())
            else:                                   # under way: it did not hold, and the update was logged
                assert not _meets(last_state[q], last_in[q], pose[q], STOP_TOL * (1 - 1e-9)), (q, k)
                assert cnt2[q] == cnt[q] + 10
        if all(q in stopped_at for q in NEAR):
            break
    print('stopped at update:', stopped_at)
    assert all(q in stopped_at for q in NEAR), stopped_at
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


def test_plant_off_changes_nothing():
    """A loop that never calls `plant` and one that called `plant(on=False)`: the same bits after the cold solve and 12 steps, and the
    plain step still runs the lean instance of the solve kernel."""
    import torch
    a = _mk(40, plant=False, record=False)
    b = _mk(40, plant=False, record=False, cold=False)
    b.plant(on=False)
    b.solve_cold(bends=())
    for _ in range(12):
        a.step(); b.step()
    torch.cuda.synchronize()
    for name in ('x', 'lam', 'p', 'status', 'iters'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.solver.workspace()['last_instance'] == 1 and b.solver.workspace()['last_instance'] == 1
    with pytest.raises(RuntimeError):
        b.plant_state()
    _close(a, b)


def test_more_updates_than_the_plant_holds():
    """max_updates = 3, the cold solve and 4 steps (stepwise and in one launch): the fourth and fifth update set the plant's `overflow`,
    write nothing -- the arrays, guarded by a canary row behind them, and the log stay as they are -- and the run ends clean."""
    import torch
    n = 8
    dist = _dist(n + 1, 3)
    dist[n] = 777.
    for roll in (False, True):
        m = _mk(n, max_updates=3, dist=dist[:n], cold=False)
        # (the canary: the disturbance the device reads is the first n blocks of a tensor with one more)
        full = torch.as_tensor(dist, dtype=torch.float64, device=m.dev)
        m._pl['dist'] = full[:n]
        m.solve_cold(bends=())
        m.rollout(2) if roll else [m.step() for _ in range(2)]
        s, ps = m.signals(), m.plant_state()
        torch.cuda.synchronize()
        assert (ps['n_upd'] == 3).all() and not ps['overflow'].any() and (s['count'] == 31).all()
        keep = dict((k, v.clone()) for k, v in ps.items() if k != 'overflow')
        log = s['splines'].clone()
        m.rollout(2) if roll else [m.step() for _ in range(2)]
        s, ps = m.signals(), m.plant_state()
        torch.cuda.synchronize()
        assert (ps['overflow'] == 1).all() and (ps['n_upd'] == 3).all() and (s['count'] == 31).all() and not s['overflow'].any()
        for k, v in keep.items():
            assert torch.equal(ps[k], v), k
        assert torch.equal(s['splines'], log) and bool((full[n] == 777.).all())
        assert float(s['input'].abs().max()) < 100.          # (no canary value was read as a disturbance)
        _close(m)
