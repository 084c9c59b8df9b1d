"""`BatchP2P.mission` on the device (`omgx_batch_set_mission`, `omgx_batch_mission_advance`): the leg switch is ONE out-of-line routine
with two callers -- the stand-alone launch and the mission instances of the rollout kernel -- so the stand-alone launch must write the
bits of the numpy twin, `rollout(K)` those of K x `rollout(1)`, a mission without further goals those of the stop-rule rollout, and a
leg start those of a fresh batch's cold solve; the whole mission is held against the host twin.  8 agents, and 520: one round of
resident workgroups plus eight, so the slot hand-out is in play."""
import functools

import numpy as np
import pytest

from mission_cases import fly, mission_batch, mission_goals, snapshot

pytestmark = pytest.mark.gpu

OPTS = dict(tol=1e-3, max_iter=300)
MAX_UPDATES = 110


@functools.lru_cache(maxsize=None)
def _plant_kw_cached(n):
    """A disturbance and per-agent lag, as tests/test_plant_lag_gpu.py uses them."""
    from omgtools.batch import input_disturbance
    # (drawn for eight agents and repeated over the batch: the filter is the slow part of a 520-agent realisation; the lags all differ)
    dist = np.tile(input_disturbance(8, 2, MAX_UPDATES, 10, 41, fc=0.1, stdev=0.02, seed=7), (n // 8, 1, 1, 1))
    return dict(sample_time=0.01, max_updates=MAX_UPDATES, disturbance=dist, time_constant=np.random.default_rng(9).uniform(0.02, 0.5, n))


def _plant_kw(n):
    return dict(_plant_kw_cached(n))


def _device(n, plant=False, **kw):
    import torch
    return mission_batch(n, 'hip', OPTS, plant=_plant_kw(n) if plant else None, device=torch.device('cuda', 0), **kw)


def _same_bits(a, b, hist):
    """a: the mission in one launch, b: step by step with the arrays after every step in `hist`.  Every array of the mission and the
    agents' status the same bits; x, lam and p the same bits for the agents under way, and for an agent that has stopped x as it was at
    the step it stopped at -- without the plant the launches that follow still run the glue of their first step on a stopped agent
    ahead of the stop test, as the stop-rule rollout does (tests/test_gpu_rollout.py), so there its p and x move on."""
    import torch
    torch.cuda.synchronize()
    sa, sb = snapshot(a), snapshot(b)
    for nm in ('iters', 'status', 'under_way', 'leg', 'clock', 'arrivals'):
        assert np.array_equal(sa[nm], sb[nm]), nm
    go = sa['under_way']
    for nm in ('x', 'lam', 'p'):
        assert np.array_equal(sa[nm][go], sb[nm][go]), nm
    for r in np.flatnonzero(~go):
        k = min(k for k, h in enumerate(hist) if not h['under_way'][r])
        assert np.array_equal(sa['x'][r], hist[k]['x'][r]), r
    if a._pl is not None:
        for nm in ('x', 'lam', 'p'):                                      # (with the plant a stopped agent is left alone altogether)
            assert np.array_equal(sa[nm], sb[nm]), nm
        pa, pb = a.plant_state(), b.plant_state()
        for nm in pa:
            assert torch.equal(pa[nm], pb[nm]), nm


def _switched_and_finished(m, n_goals, within=None, everyone=True):
    """The two conditions a mission test needs: agents with a further goal have started their second leg (`within`: by that step;
    everyone=False: some of them -- a vehicle that lags behind a disturbed input may take longer than the test flies), and one
    agent finished its whole mission at a step at which another was still under way."""
    arr = snapshot(m)['arrivals']
    first = arr[n_goals >= 1, 0]
    assert ((first >= 0).all() if everyone else (first >= 0).any()) and (within is None or (first < within).all())
    done = arr[np.arange(m.B), n_goals]
    assert (done >= 0).any() and ((done < 0).any() or done[done >= 0].min() < done.max())


@pytest.mark.parametrize('plant', [False, True])
@pytest.mark.parametrize('n', [8, 520])
def test_the_stand_alone_switch_writes_the_bits_of_the_numpy_twin(n, plant):
    """`omgx_batch_mission_advance` against `HostP2P.mission_advance` on identical inputs, every agent meeting a wide stop rule: x, lam, p,
    leg, clock, arrivals and under_way bit-equal -- agents with and without a further goal, with the plant the travelled state."""
    from omgtools.batch import BatchP2P
    dev, P = _device(n, plant, warmup=3, mission=False)
    try:
        host = BatchP2P(dev.problem, P, ops=None, options=OPTS)
        if plant:
            host.plant(**_plant_kw(n))
            for nm, a in dev.plant_state().items():
                host._pl[nm][...] = a.cpu().numpy()
        host.p, host.x, host.lam, host.time = dev.host('p').copy(), dev.host('x').copy(), dev.host('lam').copy(), dev.time
        goals, n_goals = mission_goals(dev)
        for m in (dev, host):
            m.stop_at_arrival(stop_tol=100.0)
            m.mission(goals, n_goals)
            m.mission_advance()
        got, want = snapshot(dev), snapshot(host)
        for nm in ('x', 'lam', 'p', 'leg', 'clock', 'arrivals', 'under_way'):
            assert np.array_equal(got[nm], want[nm]), nm
        assert np.array_equal(got['leg'], np.minimum(n_goals, 1)) and np.array_equal(got['under_way'], n_goals >= 1)
    finally:
        dev.solver.close()


@pytest.mark.parametrize('plant', [False, True])
@pytest.mark.parametrize('n', [8, 520])
def test_a_mission_in_one_launch_is_the_mission_step_by_step(n, plant):
    """`rollout(K)` = K x `rollout(1)` with missions, bit for bit, logs included -- agents switching, finishing and carrying on at
    different steps inside the launch; with the plant under a disturbance and a per-agent lag too."""
    import torch
    K = 70
    # (a vehicle that lags behind its plan now and then runs a warm solve to the iteration cap, and a step lasts as long as its slowest
    # solve: a cap of 40 on the steps keeps the 520-agent case short; a leg's cold solve keeps the cap of `solve_cold`)
    kw = dict(max_iter_step=40) if plant else {}
    one, _ = _device(n, plant, **kw)
    many, _ = _device(n, plant, **kw)
    try:
        n_goals = one._ms['n_goals'].cpu().numpy()
        it_log = torch.zeros((K, n), dtype=torch.int32, device=one.dev)
        st_log = torch.full((K, n), -1, dtype=torch.int32, device=one.dev)
        one.rollout(K, iters_log=it_log, status_log=st_log)
        hist = fly(many, K)
        _same_bits(one, many, hist)
        assert np.array_equal(it_log.cpu().numpy(), np.array([h['iters'] for h in hist]))
        assert np.array_equal(st_log.cpu().numpy(), np.array([h['status'] for h in hist]))
        assert abs(one.time - many.time) < 1e-12
        _switched_and_finished(one, n_goals, within=40 if n == 8 and not plant else None, everyone=not plant)
        assert set(n_goals.tolist()) == {0, 1, 2, 3} and snapshot(one)['leg'].max() >= (1 if plant else 3)
    finally:
        one.solver.close(); many.solver.close()


@pytest.mark.parametrize('n', [8, 520])
def test_without_further_goals_a_mission_is_the_stop_rule_rollout(n):
    import torch
    ruled, _ = _device(n, mission=False)
    flown, _ = _device(n, mission=False)
    try:
        flown.mission(mission_goals(flown)[0], np.zeros(n, dtype=np.int32))
        K = 30                                                            # (some agents have arrived by then and some have not)
        logs = [(torch.zeros((K, n), dtype=torch.int32, device=ruled.dev), torch.full((K, n), -1, dtype=torch.int32, device=ruled.dev)) for _ in range(2)]
        ruled.rollout(K, iters_log=logs[0][0], status_log=logs[0][1])
        flown.rollout(K, iters_log=logs[1][0], status_log=logs[1][1])
        torch.cuda.synchronize()
        for nm in ('x', 'lam', 'p', 'status', 'iters', 'under_way'):
            assert torch.equal(getattr(ruled, nm), getattr(flown, nm)), nm
        assert torch.equal(logs[0][0], logs[1][0]) and torch.equal(logs[0][1], logs[1][1])
        under = flown.host('under_way') != 0
        assert 0 < under.sum() < n
        st = snapshot(flown)
        assert (st['leg'] == 0).all() and np.array_equal(st['arrivals'][:, 0] >= 0, ~under)
    finally:
        ruled.solver.close(); flown.solver.close()


@pytest.mark.parametrize('n', [8, 520])
def test_a_leg_start_is_a_fresh_batchs_cold_solve(n):
    """Stepping with `rollout(1)`: for the agents whose `leg` advanced, a fresh `DeviceP2P` built from their rows of p after the call and
    the linspace guess gives the mission's x, lam, status, iters with `solve_cold(bends=(), fused=False)` -- bit for bit -- and the
    following updates of both, over a knot crossing of the leg's own clock, stay bit-identical."""
    import torch
    from omgtools.batch import BatchP2P
    m, P = _device(n)
    goals = m._ms['goals'].cpu().numpy()
    L, nd = m.L, m.n_dim
    fresh, checked = None, 0
    try:
        for k in range(70):
            before = snapshot(m)
            m.rollout(1)
            after = snapshot(m)
            idx = np.flatnonzero(after['leg'] != before['leg'])
            if not len(idx):
                continue
            guess = np.tile(np.asarray(P['x0'][0], dtype=float), (len(idx), 1))
            for r, b in enumerate(idx):
                s_old = before['p'][b, m.o_state0:m.o_state0 + nd]
                guess[r, m.o_spl:m.o_spl + nd * L] = np.concatenate([np.linspace(s_old[a], goals[b, before['leg'][b], a], L) for a in range(nd)])
            fresh = BatchP2P(m.problem, dict(P, p=after['p'][idx], x0=guess), ops='hip', device=m.dev, options=OPTS)
            fresh.solve_cold(bends=(), fused=False)
            crossings, same = 0, np.ones(len(idx), dtype=bool)
            for j in range(13):
                if j:
                    crossings += int(fresh.step())
                    m.rollout(1)
                now = snapshot(m)
                same &= now['under_way'][idx] & (now['leg'][idx] == after['leg'][idx])      # (an agent that switches again leaves the comparison)
                for nm in ('x', 'lam', 'p', 'status', 'iters'):
                    assert np.array_equal(fresh.host(nm)[same], now[nm][idx][same]), (k, j, nm)
                assert (now['clock'][idx][same] == j).all()
            assert crossings == 1
            fresh.solver.close()
            fresh, checked = None, checked + int(same.any())                  # (a group whose agents all switched again inside the 13 updates shows nothing of the crossing)
            if checked == 2:
                break
        assert checked == 2
    finally:
        m.solver.close()
        if fresh is not None:
            fresh.solver.close()


def test_the_device_mission_against_the_host_twin():
    """The whole mission, device loop against host loop (oracle port), with the options and the bounds of tests/test_gpu_batch_mpc.py for
    device against host build: the same switch steps, the same status log, positions to 2e-4 and velocities to 2e-3."""
    import torch
    from oracle import port_binding
    opts = dict(tol=1e-5, max_iter=300)
    dev, _ = mission_batch(8, 'hip', opts, device=torch.device('cuda', 0), max_iter_step=300)
    host, _ = mission_batch(8, port_binding, opts, max_iter_step=300)
    try:
        hd, hh = fly(dev, 60), fly(host, 60)
        n_goals = host._ms['n_goals']
        s0, i0, worst_iters = dev.o_state0, dev.o_input0, 0
        for k, (d, h) in enumerate(zip(hd, hh)):
            for nm in ('leg', 'clock', 'arrivals', 'under_way', 'status'):
                assert np.array_equal(d[nm], h[nm]), (k, nm)
            go = h['under_way']
            assert np.abs(d['p'][go, s0:s0 + 2] - h['p'][go, s0:s0 + 2]).max(initial=0.0) < 2e-4, k
            assert np.abs(d['p'][go, i0:i0 + 2] - h['p'][go, i0:i0 + 2]).max(initial=0.0) < 2e-3, k
            worst_iters = max(worst_iters, int(np.abs(d['iters'] - h['iters']).max()))
        print('largest difference of an iteration count, device against host: %d' % worst_iters)
        _switched_and_finished(dev, n_goals)
    finally:
        dev.solver.close()
