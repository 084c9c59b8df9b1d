"""The mission every mission test flies (tests/test_mission_cpu.py, tests/test_mission_gpu.py).  The config-2 arena is four metres
across, so the legs go back to an agent's start and forth to its first goal again, with `stop_tol = 1.5` (arrival some way out, a leg of
about twenty updates: a knot crossing of the leg's own clock inside); 0, 1, 2, 3 further goals in turn over the batch.  The mission is
set after `WARMUP` plain updates -- the first leg then carries on from a batch clock that is not zero -- and the first arrivals come
some 25 updates later: agents switch, finish and carry on at different updates inside 40 of them."""
import numpy as np

STOP_TOL = 1.5
WARMUP = 25


def mission_goals(m):
    """(goals [B, 3, n_dim], n_goals [B]) for the batch `m`, from its agents' start positions and first goals as its first guess and p
    hold them (host arrays, whichever executor)."""
    n, L = m.n_dim, m.L
    x0 = np.asarray(m._x0, dtype=float)
    start = np.stack([x0[:, m.o_spl + k * L] for k in range(n)], axis=1)
    o_pose = m._o_pose('mission')
    goal0 = m.host('p')[:, o_pose:o_pose + n].copy()
    goals = np.ascontiguousarray(np.stack([start, goal0, start], axis=1))
    return goals, (np.arange(m.B) % 4).astype(np.int32)


def mission_batch(n, ops, options, stop_tol=STOP_TOL, warmup=WARMUP, mission=True, plant=None, build=None, **kw):
    """(batch, P): n agents of the config-2 workload, stop rule on, cold solve, `warmup` plain updates, then the mission.  plant: the
    keyword arguments of `BatchP2P.plant`, called ahead of the cold solve.  build(n) -> (problem, P): another class than config 2
    (tests/test_gpu_workspace_cells.py)."""
    from omgtools import workloads
    from omgtools.batch import BatchP2P
    problem, P = (build or workloads.holonomic_p2p)(n)
    m = BatchP2P(problem, P, ops=ops, options=options, **kw)
    if plant is not None:
        m.plant(**plant)
    m.stop_at_arrival(stop_tol=stop_tol)
    m.solve_cold(bends=())
    for _ in range(warmup):
        m.step()
    if mission:
        m.mission(*mission_goals(m))
    return m, P


def snapshot(m):
    out = dict((nm, m.host(nm).copy()) for nm in ('x', 'lam', 'p', 'iters', 'status'))
    out['under_way'] = m.host('under_way') != 0
    st = m.mission_state()
    out.update((nm, (st[nm].cpu().numpy() if hasattr(st[nm], 'cpu') else st[nm]).copy()) for nm in ('leg', 'clock', 'arrivals'))
    return out


def fly(m, n_updates):
    """`n_updates` times `rollout(1)`; the arrays after every update."""
    hist = []
    for _ in range(n_updates):
        m.rollout(1)
        hist.append(snapshot(m))
    return hist
