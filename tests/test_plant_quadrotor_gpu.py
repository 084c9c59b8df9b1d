"""The Quadrotor's plant on the device (`omgx_batch_plant_quadrotor_simulate / _predict`, include/omgx.h OMGX_HAS_PLANT_QUADROTOR): the
two stand-alone kernels against the reference's own `Quadrotor` (tests/golden/plant_quadrotor.npz) and against the host twin, the
prediction from measured states against the plant's (the same bits), sub-batches on streams, the stop rule on the travelled state,
the disturbance in the log, the limits, and a loop that switches the plant off again."""
import numpy as np
import pytest

from test_plant_quadrotor_cpu import N_SAMP, check_against_quad_fixture, fixture, host_replay, replay_quad_fixture

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)
LOOP = ('x', 'lam', 'p', 'status', 'iters')
NEAR, STOP_TOL = (0, 5, 10, 15), 1e-2      # (the Quadrotor's own default stop_tol, `vehicles/quadrotor.py:42`)


def _dist(n, max_updates, stdev=0.05, seed=7):
    from omgtools.batch import input_disturbance
    return input_disturbance(n, 2, max_updates, N_SAMP, 501, fc=0.1, stdev=stdev, seed=seed)


def _mk(n, max_updates=8, dist='noise', plant=True, feedback=False, record=True, stop=None, cold=True, mutate=None, cls=None, **kw):
    import torch
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = workloads.quadrotor_p2p(n)
    if mutate is not None:
        mutate(problem, P)
    m = (cls or BatchP2P)(problem, P, device=torch.device('cuda', 0), options=OPTS, **kw)
    if plant:
        m.plant(sample_time=0.01, max_updates=max_updates, disturbance=_dist(n, max_updates) if isinstance(dist, str) else dist, model='quadrotor')
    if feedback:
        m.feedback(sample_time=0.01, model='quadrotor')
    if stop is not None:
        m.stop_at_arrival(stop_tol=stop)
    if record:
        m.record_signals(sample_time=0.01, max_updates=max_updates)
    if cold:
        m.solve_cold()
    return m


def _close(*ms):
    for m in ms:
        if hasattr(m, 'close'):
            m.close()
        else:
            m.solver.close()


def _same_loop(a, b, names=LOOP):
    import torch
    torch.cuda.synchronize()
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize('chained', [False, True])
def test_stand_alone_kernels_equal_the_reference_and_the_host_twin(chained):
    """The 4 fixture agents, 8 updates (the fifth solve lies behind a knot crossing) through the two kernels: the bounds of
    tests/test_plant_quadrotor_cpu.py against the reference, and the host twin on identical inputs within 1e-10 -- the chain is 80
    Runge-Kutta steps whose sin / cos differ by a few ulps between the two libraries on terms h u1 <= 0.2: about 1e-13 accumulated
    (observed on an MI355X: 1.2e-13, chained and per update; against the reference 6.3e-7 per update and 6.1e-6 chained, the fixture's
    own ode_dev figures)."""
    import torch
    q = fixture()
    dev = _mk(4, max_updates=8, dist=q['dist'], cold=False)
    assert np.array_equal(np.asarray(dev.basis.knots, dtype=float), q['knots']) and dev.T == float(q['horizon_time'])

    def get(t):
        return t.cpu().numpy()

    def put(t, a):
        t.copy_(torch.as_tensor(np.ascontiguousarray(a), dtype=t.dtype, device=t.device))
    pred = replay_quad_fixture(dev, q, dev._plant_predict, dev._plant_simulate, chained, get, put)
    sig = {k: (v.cpu().numpy() if hasattr(v, 'cpu') else v) for k, v in dev.signals().items()}
    st = {k: v.cpu().numpy() for k, v in dev.plant_state().items()}
    assert (st['n_upd'] == 8).all() and not st['overflow'].any()
    check_against_quad_fixture(q, sig, pred, chained)
    host, h_pred = host_replay(chained, q)
    hs, hp = host.signals(), host.plant_state()
    err = max([float(np.abs(sig[k] - hs[k]).max()) for k in ('splines', 'state', 'input')] + [float(np.abs(pred[:, 1:] - h_pred[:, 1:]).max())] +
              [float(np.abs(st[k] - hp[k]).max()) for k in ('state', 'state_prev', 'input_last', 'dspl_last')])
    print('device against the host twin: %.2e' % err)
    assert err <= 1e-10
    assert np.array_equal(sig['count'], hs['count']) and np.array_equal(st['n_upd'], hp['n_upd'])
    assert np.array_equal(sig['overflow'], hs['overflow']) and np.array_equal(st['overflow'], hp['overflow'])
    _close(dev)


def test_measured_states_equal_to_state_prev_give_the_plants_bits():
    """8 agents, the cold solve and 6 steps across the knot crossing.  Loop A runs with the plant; loop B runs with `feedback` and is
    fed loop A's state_prev before every step (a device tensor, or a pinned host tensor), with loop A's plan and parameters restored:
    the same bits in x, lam, p, status and iters after every step."""
    import torch
    a = _mk(8, record=False)
    b = _mk(8, plant=False, feedback=True, record=False)
    _same_loop(a, b)
    crossings = 0
    for k in range(6):
        for name in LOOP:
            getattr(b, name).copy_(getattr(a, name))
        S = a.plant_state()['state_prev'].clone()
        if k % 2:
            torch.cuda.synchronize()
            S = S.cpu().pin_memory()
        crossings += int(a.step())
        assert int(b.step(states=S)) == int(k == 3)
        _same_loop(a, b)
    assert crossings == 1 and bool((a.status == 0).all())
    assert float(a._pl['dist'].abs().max()) > 1e-3 and bool((a.plant_state()['n_upd'] == 7).all())
    _close(a, b)


def test_an_agent_without_a_fresh_measurement_gets_the_ideal_prediction():
    """fresh = 0: exactly the bits the ideal `step()` writes into spl0 / dspl0 / ddspl0 (and then the same solve); fresh = 1 with
    `enforce`: the measured position, at rest."""
    import torch
    ideal = _mk(8, plant=False, record=False)
    fed = _mk(8, plant=False, feedback=True, record=False)
    enf = _mk(8, plant=False, feedback=True, record=False)
    _same_loop(ideal, fed)
    fresh = torch.tensor([1, 0, 0, 1, 0, 1, 1, 0], dtype=torch.int32, device=ideal.dev)
    stale = (fresh == 0).nonzero().flatten()
    S = torch.randn(8, 5, dtype=torch.float64, device=ideal.dev, generator=torch.Generator(device=ideal.dev).manual_seed(3)) * 0.1
    o0, o2 = ideal.p_offs[0], ideal.p_offs[2]
    S[:, :2] += ideal.p[:, o0:o0 + 2]
    seen = {}

    def keep(m):
        seen[id(m)] = m.p.clone()
    ideal.step(before_solve=keep)
    fed.step(states=S, fresh=fresh, before_solve=keep)
    enf.step(states=S, fresh=fresh, enforce=True, before_solve=keep)
    torch.cuda.synchronize()
    p_i, p_f, p_e = seen[id(ideal)], seen[id(fed)], seen[id(enf)]
    assert torch.equal(p_f[stale], p_i[stale]) and torch.equal(p_e[stale], p_i[stale])
    for name in ('x', 'lam', 'status', 'iters'):
        assert torch.equal(getattr(fed, name)[stale], getattr(ideal, name)[stale]), name
    live = fresh.nonzero().flatten()
    assert torch.equal(p_e[live, o0:o0 + 2], S[live, :2]) and not bool(p_e[live, ideal.p_offs[1]:o2 + 2].any())
    assert torch.equal(p_f[live, ideal.p_offs[1]:o2 + 2], p_i[live, ideal.p_offs[1]:o2 + 2])      # (dspl0 / ddspl0: the plan's, fresh or not)
    assert float((p_f[live, o0:o0 + 2] - p_i[live, o0:o0 + 2]).abs().max(dim=1).values.min()) > 1e-3      # (spl0: integrated from the measurement)
    assert torch.equal(p_f[:, ideal.o_t], p_i[:, ideal.o_t])
    _close(ideal, fed, enf)


def test_sub_batches_on_streams_equal_one_handle():
    """`StreamedP2P(n_streams=3)` against one handle, 24 agents, the cold solve and 6 steps: the same bits everywhere."""
    import torch
    from omgtools.batch import StreamedP2P
    dist = _dist(24, 8)
    one = _mk(24, dist=dist)
    many = _mk(24, dist=dist, cls=StreamedP2P, n_streams=3)
    crossings = 0
    for _ in range(6):
        crossings += int(one.step())
        many.step()
    _same_loop(one, many)
    sa, sb, pa, pb = one.signals(), many.signals(), one.plant_state(), many.plant_state()
    torch.cuda.synchronize()
    assert set(sa) == set(sb) and {'state', 'input', 'splines', 'count', 'overflow'} <= set(sa)
    for name in sa:
        if name != 'time':
            assert torch.equal(sa[name], sb[name]), name
    assert set(pa) == set(pb) and 'dspl_last' in pa
    for name in pa:
        assert torch.equal(pa[name], pb[name]), name
    assert crossings == 1 and bool((sa['count'] == 1 + N_SAMP * 7).all()) and tuple(sa['state'].shape) == (24, 5, 81)
    _close(one, many)


def _near_targets(problem, P):
    """poseT of four agents moved to 5 cm from their start: they arrive within the run."""
    tpl, label = problem.father.template, problem.vehicles[0].label
    s0, pT = (tpl.entry_range(label, nm, 'par')[0] for nm in ('spl0', 'poseT'))
    L, o_spl = len(problem.vehicles[0].basis), tpl.entry_range(label, 'splines_seg0', 'var')[0]
    for b in NEAR:
        d = P['p'][b, pT:pT + 2] - P['p'][b, s0:s0 + 2]
        P['p'][b, pT:pT + 2] = P['p'][b, s0:s0 + 2] + 0.05 * d / np.linalg.norm(d)
        for k in range(2):      # (the initial guess on the straight line to the new target, clamped like the workload's)
            c = np.linspace(P['p'][b, s0 + k], P['p'][b, pT + k], L - 8)
            P['x0'][b, o_spl + k * L:o_spl + (k + 1) * L] = np.r_[[c[0]] * 4, c, [c[-1]] * 4]


def test_stop_rule_on_the_travelled_state():
    """16 agents, four of them with a target 5 cm away, a disturbance during the first three updates, the stop rule on.  An agent
    stops at the first update where the rule holds on what `plant_state()` showed ahead of the step (travelled position against poseT,
    the plan's velocity at the last travelled sample; a relative 1e-9 for the order of the squares); from then on its plan, its
    multipliers and its plant state stay bit-identical and its log stops growing.  The rest run on."""
    import torch
    n, max_steps = 16, 40
    dist = _dist(n, max_steps + 1, stdev=0.02)
    dist[:, :, 3:, :] = 0.
    m = _mk(n, max_updates=max_steps + 1, dist=dist, mutate=_near_targets, stop=STOP_TOL)
    pose = m.p[:, m._pl['o_pose']:m._pl['o_pose'] + 2].cpu().numpy()

    def meets(state, dspl, tol):
        return (np.sqrt(((state[:, :2] - pose) ** 2).sum(axis=1)) <= tol) & (np.sqrt((dspl ** 2).sum(axis=1)) <= tol)
    stopped_at, frozen = {}, {}
    for k in range(1, max_steps + 1):
        ps = {nm: v.cpu().numpy() for nm, v in m.plant_state().items()}
        cnt = m.signals()['count'].cpu().numpy()
        m.step()
        uw, cnt2 = m.under_way.cpu().numpy(), m.signals()['count'].cpu().numpy()
        ps2 = m.plant_state()
        for b in range(n):
            if b in stopped_at:
                assert uw[b] == 0 and cnt2[b] == cnt[b], (b, k)
                assert torch.equal(m.x[b], frozen[b][0]) and torch.equal(m.lam[b], frozen[b][1]), (b, k)
                assert all(torch.equal(ps2[nm][b], frozen[b][2][nm]) for nm in ps2), (b, k)
            elif uw[b] == 0:                        # stopped at this update: the rule held on the travelled state
                assert meets(ps['state'], ps['dspl_last'], STOP_TOL * (1 + 1e-9))[b], (b, k)
                assert cnt2[b] == cnt[b] and all(np.array_equal(ps2[nm][b].cpu().numpy(), ps[nm][b]) for nm in ps2), (b, k)
                stopped_at[b], frozen[b] = k, (m.x[b].clone(), m.lam[b].clone(), {nm: v[b].clone() for nm, v in ps2.items()})
            else:                                   # under way: it did not hold, and the update was travelled and logged
                assert not meets(ps['state'], ps['dspl_last'], STOP_TOL * (1 - 1e-9))[b], (b, k)
                assert cnt2[b] == cnt[b] + N_SAMP and ps2['n_upd'][b] == ps['n_upd'][b] + 1, (b, k)
        if all(b in stopped_at for b in NEAR):
            break
    print('stopped at update:', stopped_at)
    assert sorted(stopped_at) == list(NEAR), stopped_at
    assert bool(m.arrived(STOP_TOL)[list(NEAR)].all()) and not bool(m.plant_state()['overflow'].any())
    _close(m)


def test_the_logged_input_is_the_plans_plus_the_disturbance():
    """8 agents, the cold solve and 5 steps: the logged `input` minus the plan's own (u1, u2) -- scipy B-splines on the plan of every
    update, no code shared with the package -- minus the supplied disturbance is at most 1e-10; the logged state starts every update
    where the last one ended, and column 0 is the first plan's own sample 0."""
    from scipy.interpolate import BSpline
    n, n_upd, g = 8, 6, 9.81
    dist = _dist(n, n_upd)
    assert np.abs(dist).max() > 1e-3
    m = _mk(n, max_updates=n_upd, dist=dist, cold=False)
    knots, T, worst = np.asarray(m.basis.knots, dtype=float), m.T, 0.0
    for k in range(n_upd):
        m.step() if k else m.solve_cold()
        c = m.x[:, m.o_spl:m.o_spl + 2 * m.L].cpu().numpy().reshape(n, 2, m.L)
        t_rel = m.p[:, m.o_t].cpu().numpy()
        sig = m.signals()
        logged, state = sig['input'].cpu().numpy(), sig['state'].cpu().numpy()
        for b in range(n):
            u = (t_rel[b] + np.arange(N_SAMP + 1) * 0.01) / T
            spl = BSpline(knots, c[b].T, 4)
            dd, ddd = spl.derivative(2)(u).T / T ** 2, spl.derivative(3)(u).T / T ** 3
            u1 = np.sqrt(dd[0] ** 2 + (dd[1] + g) ** 2)
            u2 = (ddd[0] * (dd[1] + g) - dd[0] * ddd[1]) / ((dd[1] + g) ** 2 + dd[0] ** 2)
            cols = slice(k * N_SAMP + 1, (k + 1) * N_SAMP + 1)
            worst = max(worst, np.abs(logged[b, :, cols] - np.array([u1, u2])[:, 1:] - dist[b, :, k, 1:]).max())
            if k == 0:
                d1 = spl.derivative(1)(u[:1]).T / T
                s0 = np.r_[spl(u[:1])[0], d1[:, 0], np.arctan2(dd[0, 0], dd[1, 0] + g)]
                worst = max(worst, np.abs(state[b, :, 0] - s0).max(), np.abs(logged[b, :, 0] - [u1[0], u2[0]]).max())
    print('logged input - plan - disturbance: %.2e' % worst)
    assert worst <= 1e-10
    ps = m.plant_state()
    assert bool((sig['count'] == 1 + N_SAMP * n_upd).all())
    assert np.array_equal(ps['state'].cpu().numpy(), state[:, :, -1]) and np.array_equal(ps['state_prev'].cpu().numpy(), state[:, :, -1 - N_SAMP])
    assert np.array_equal(ps['input_last'].cpu().numpy(), logged[:, :, -1])
    _close(m)


def test_limits_and_offsets():
    """An update beyond `max_updates` writes nothing and sets `overflow`; a log that is full drops the append and the vehicle travels
    on; offsets outside p are refused by name."""
    import torch
    from omgtools.backend import OmgxError
    m = _mk(4, max_updates=2)
    m.step()
    before = {k: v.clone() for k, v in m.plant_state().items()}
    sig = m.signals()
    cnt, logs = sig['count'].clone(), [sig[k].clone() for k in ('state', 'input', 'splines')]
    assert bool((before['n_upd'] == 2).all()) and not bool(before['overflow'].any()) and bool((cnt == 1 + 2 * N_SAMP).all())
    m.step()
    torch.cuda.synchronize()
    after, sig = m.plant_state(), m.signals()
    assert bool((after['overflow'] == 1).all()) and torch.equal(sig['count'], cnt) and not bool(sig['overflow'].any())
    for k in ('state', 'state_prev', 'input_last', 'dspl_last', 'n_upd'):
        assert torch.equal(after[k], before[k]), k
    for k, old in zip(('state', 'input', 'splines'), logs):
        assert torch.equal(sig[k], old), k
    _close(m)
    # the log holds one update less than the plant simulates
    m = _mk(4, max_updates=3, record=False, cold=False)
    m.record_signals(sample_time=0.01, cap=1 + 2 * N_SAMP)
    m.solve_cold()
    m.step()
    m.step()
    torch.cuda.synchronize()
    sig, ps = m.signals(), m.plant_state()
    assert bool((sig['count'] == 1 + 2 * N_SAMP).all()) and bool((sig['overflow'] == 1).all())
    assert bool((ps['n_upd'] == 3).all()) and not bool(ps['overflow'].any())
    # offsets outside p
    n_par = m.tpl.n_par
    for field, value, word in (('p_off', [0, n_par - 1, 4], 'p_off[1]'), ('p_t', n_par, 'p_t'), ('p_poseT', n_par - 1, 'p_poseT'),
                               ('coeff_off', m.tpl.n_var - 3, 'coefficients outside x')):
        args = dict(m._quad_args(m._pl), **{field: value})
        with pytest.raises(OmgxError) as e:
            m.solver.plant_quadrotor_predict(m.x, m.p, 0.02, 0.1, args)
        assert 'plant_quadrotor_predict' in str(e.value) and word in str(e.value), str(e.value)
        with pytest.raises(OmgxError) as e:
            m.solver.plant_quadrotor_simulate(m.x, m.p, args)
        assert 'plant_quadrotor_simulate' in str(e.value) and word in str(e.value), str(e.value)
    _close(m)


def test_switching_the_plant_off_restores_the_loop():
    """`plant(on=False)` gives the bits of a loop that never had a plant, the fused log included."""
    import torch
    a = _mk(8, cold=False)
    a.plant(on=False)
    b = _mk(8, plant=False, cold=False)
    for m in (a, b):
        m.solve_cold()
        for _ in range(4):
            m.step()
    _same_loop(a, b)
    sa, sb = a.signals(), b.signals()
    torch.cuda.synchronize()
    assert set(sa) == set(sb) and 'state' not in sa
    for name in ('splines', 'count', 'overflow'):
        assert torch.equal(sa[name], sb[name]), name
    assert bool((sa['count'] == 1 + N_SAMP * 5).all())
    with pytest.raises(RuntimeError):
        a.plant_state()
    _close(a, b)
