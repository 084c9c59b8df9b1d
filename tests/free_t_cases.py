"""Shared by tests/test_free_t_cpu.py and tests/test_free_t_gpu.py: the free-end-time batch of `scenarios.holonomic_free_t_p2p`, random
plans with the horizons that walk through every branch of one `omgx_batch_free_t_advance` call, and the conditions a finished
manoeuvre has to meet."""
import os

import numpy as np

UPDATE_TIME, SAMPLE_TIME = 0.1, 0.01
SEED = 20240807 + 7          # (the builder's default; every one of its 8 agents arrives on the host port)
# one agent per branch: the ordinary step; T < 2 update_time twice (0.15: the shortened update, 0.1: dt = 0, the identity); the
# stop clause (0.05) and a NaN; an agent whose flag is 0 already (index 5, T = 10); s = 1 exactly (T = 2 update_time); 0.25
BRANCH_T = np.array([10., 0.25, 0.15, 0.1, 0.05, 10., np.nan, 0.2])
MASKED = 5
_cache = {}


def batch(n_agents=8, knot_intervals=5):
    """(problem, P) of the builder, built once per shape (the template is read only); no solver is made for the front end's own
    `problem.init()` -- the tests hand the batch to the executor they are about."""
    key = (n_agents, knot_intervals)
    if key not in _cache:
        import omgtools.backend as be
        from omgtools.scenarios import holonomic_free_t_p2p
        saved = be.create_nlp
        be.create_nlp = lambda tpl, opt, name='': (None, 0.)
        try:
            _cache[key] = holonomic_free_t_p2p(n_agents, knot_intervals=knot_intervals, seed=SEED)
        finally:
            be.create_nlp = saved
    problem, P = _cache[key]
    return problem, dict(p=P['p'].copy(), x0=P['x0'].copy())


def tables(problem, P):
    """The free-T tables `BatchP2P` builds for the problem (no executor: the host class with no solver object)."""
    from omgtools.batch import BatchP2P
    m = BatchP2P(problem, P, ops=object(), update_time=UPDATE_TIME)
    return m._ft, m


def random_plans(ft, tpl, T, seed=3):
    """x [B, n_var], p [B, n_par]: smooth random coefficient sets of order 1 everywhere, x[:, o_T] = T."""
    rng = np.random.default_rng(seed)
    B = len(T)
    x = np.cumsum(rng.normal(0., 0.3, (B, tpl.n_var)), axis=1)
    p = rng.normal(0., 1., (B, tpl.n_par))
    x[:, ft['o_T']] = T
    return x, p


def written_columns(ft):
    """Indices of x an advance may write: the entries and T."""
    idx = [ft['o_T']]
    for off, rows, cols, _ in ft['entries']:
        idx += list(range(off, off + rows * cols))
    return np.array(sorted(idx))


def check_manoeuvre(summary, p0, p_end, o_state0, o_pose, counts):
    """Every agent arrived within 1e-2 of its goal; its motion time is (columns - 1) sample_time and at least what the velocity
    limit of the class (0.5 per axis) allows."""
    summary, counts = np.asarray(summary), np.asarray(counts)
    assert (summary[:, 5] < 1e-2).all(), summary[:, 5]
    assert np.array_equal(summary[:, 0], counts) and np.allclose(summary[:, 1], (counts - 1) * SAMPLE_TIME, rtol=0, atol=1e-12)
    far = np.abs(p_end[:, o_pose:o_pose + 2] - p0[:, o_state0:o_state0 + 2]).max(axis=1)
    assert (summary[:, 1] >= far / 0.5).all(), (summary[:, 1], far / 0.5)


def reference_run():
    """tests/golden/free_t_holonomic.npz (generator: tests/golden/generate_free_t_golden.py): the reference's own free-end-time run with
    a recorder in the place of its solver."""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'free_t_holonomic.npz'), allow_pickle=True)


def reference_tables(g, ft, u):
    """The tables `ft` with, per basis, the (fit, proj) the reference used at update u."""
    degrees = [int(g['degree_%d' % j]) for j in range(int(g['n_bases']))]
    bases = []
    for bs in ft['bases']:
        j = degrees.index(bs['degree'])
        assert np.array_equal(g['knots_%d' % j], bs['knots'])
        bases.append(dict(bs, fit=g['fit_%d_%d' % (u, j)], proj=np.ascontiguousarray(g['proj_%d_%d' % (u, j)])))
    return dict(ft, bases=bases)


def check_against_reference_x0(ft, x_old, x_new, x0_ref):
    """The shifted entries against the x0 the reference's solver was called with: the reference zeroes the entries of its
    transformation below 1e-10, at most L per row -- L 1e-10 max|c|; T to rounding."""
    for off, rows, cols, _ in ft['entries']:
        sl = slice(off, off + rows * cols)
        assert np.abs(x_new[sl] - x0_ref[sl]).max() <= rows * 1e-10 * np.abs(x_old[sl]).max(), off
    assert abs(x_new[ft['o_T']] - x0_ref[ft['o_T']]) <= 1e-12
