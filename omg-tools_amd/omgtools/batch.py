"""`BatchP2P`: B independent point-to-point agents driven through the receding-horizon loop with everything resident on the device.

The reference loops `Deployer.update` -> `problem.predict / solve / store` (`execution/deployer.py:43-79`) for one agent in Python.
Here one MPC step of the whole batch is: (1) ideal prediction -- the initial condition of the next solve is the current plan
evaluated `update_time` ahead (`vehicles/vehicle.py:323-326`, C++ `Vehicle::predict` Vehicle.cpp:61-80); (2) horizon bookkeeping
`t = time since the last knot crossing` and, on a crossing, the warm-start shift of every `seg` spline variable
(`problems/point2point.py:187-198`, `basics/optilayer.py:470-490`) plus an index shift of the multipliers; (3) `omgx_batch_solve`
with a primal-dual warm start.

Layout: `BatchP2P` states that protocol once -- tables and options from the template, `solve_cold`, `step`, `rollout`, the stop rule,
the log -- and branches on no executor.  Where the [B, *] arrays live and who computes on them sits behind its hooks (`_allocate,
_predict, _shift, _solve, _cold, _rollout, _norm, _stop_rule, _signals_alloc, _signals_fused, _signals_append_now,
_signals_summary, _free_t_set, _free_t_advance, _zeros, _plant_alloc, _plant_lag, _plant_predict, _plant_simulate, _plant_rollout, _feedback_predict, _script_alloc, _script_advance, _mission_alloc, _mission_off, _mission_clock_max, _mission_run, _mission_advance`), written once per executor: `DeviceP2P` (`ops='hip'`, the only product path: launches of the library on torch tensors, torch
being the allocator / stream only; no data leaves HBM between steps) and `HostP2P` (`ops=<a host solver object>`: the same
statements in numpy, how the parity tests and the CPU baseline of bench.py replay the loop; this package never imports the
oracle).  `BatchP2P(problem, P, ops=...)` hands out the executor `ops` names.  The clock of a step is `splines.step_clock`, the
obstacle motion `splines.advance_obstacles`: shared with the formation loops.

`BatchP2P.plant` puts a simulated vehicle into the loop (the reference's default `ideal_prediction=False, ideal_update=False`, with an
optional input disturbance): step (1) then starts the solve from the state the vehicle had one update ago integrated under the planned
inputs, and after step (3) the vehicle travels the update under the applied inputs (include/omgx.h OMGX_HAS_PLANT has the statements);
with `time_constant` the vehicle applies them through the reference's first-order actuator lag (OMGX_HAS_PLANT_LAG); with
`model='quadrotor'` the vehicle is the Quadrotor's own model, per step (OMGX_HAS_PLANT_QUADROTOR; `feedback(model='quadrotor')` likewise).
`BatchP2P.feedback` lets `step` take states measured outside the loop instead (`step(states=...)`, the reference's
`Deployer.update(current_time, states, ...)`; include/omgx.h OMGX_HAS_FEEDBACK): a loop has one source of states.
`BatchP2P.obstacle_script` moves the obstacles by the reference's `simulation={'trajectories': ...}` -- jumps of position, velocity
or acceleration at given times (include/omgx.h OMGX_HAS_OBSTACLE_SCRIPT; `splines.advance_obstacles_scripted` in numpy).
`BatchP2P.mission` gives every agent a list of goals: inside `rollout` an agent that arrives starts its next leg -- fresh guess, cold
solve, a clock of its own -- instead of ending its loop (include/omgx.h OMGX_HAS_MISSION; `mission_next_leg_numpy` in numpy).

A free-end-time problem (`Point2point(..., freeT=True)`: `FreeTPoint2point`, one Holonomic or Holonomic3D vehicle) runs another
protocol, stated once in `BatchP2P._step_free_t`: T is a variable of every agent, there is no knot clock, and a step is advance (the stop
clause T < update_time, the prediction on the old plan and the old T, the plan re-expressed on what is left of it, T reduced -- one
launch, include/omgx.h OMGX_HAS_FREE_T; `free_t_advance_numpy` in numpy), obstacle motion, warm-started solve, and with `record_signals`
the append on every agent's own horizon (`free_t_append_numpy`).  `horizon()` returns the current T per agent; `rollout`, `plant`,
`feedback` and `mission` are refused on such a batch.
"""
import math
import os

import numpy as np

from .splines import SCRIPT_EPS, advance_obstacles, advance_obstacles_scripted, shiftoverknot_T, step_clock


# solver options of a knot-crossing step (BatchP2P `cross_options`)
CROSS_OPTIONS = {}


def input_disturbance(B, n_in, n_updates, n_samp, n_horizon, fc, stdev, mean=None, seed=0):
    """A realisation of the reference's input disturbance for `BatchP2P.plant`: [B, n_in, n_updates, n_samp + 1].  The reference's
    recipe (`Vehicle.add_disturbance`, `vehicles/vehicle.py:433-448`) per agent, input and update: normal noise (mean, stdev) of the
    length of the planned horizon (`n_horizon` samples), low-pass filtered forwards and backwards by a third-order Butterworth filter
    with cut-off `fc` (as a fraction of the Nyquist frequency); of it the vehicle meets the samples 0 .. n_samp of the update.  Drawn
    from a seeded numpy generator: the same array for the same arguments.  stdev / mean: scalars or one value per input."""
    from scipy.signal import butter, filtfilt
    stdev = np.broadcast_to(np.asarray(stdev, dtype=float), (int(n_in),))
    mean = np.zeros(int(n_in)) if mean is None else np.broadcast_to(np.asarray(mean, dtype=float), (int(n_in),))
    if int(n_horizon) < int(n_samp) + 1:
        raise ValueError('input_disturbance: the horizon (%d samples) is shorter than an update (%d)' % (n_horizon, n_samp + 1))
    rng = np.random.default_rng(seed)
    noise = rng.normal(mean[None, :, None, None], stdev[None, :, None, None], (int(B), int(n_in), int(n_updates), int(n_horizon)))
    num, den = butter(3, fc, 'low')
    return np.ascontiguousarray(filtfilt(num, den, noise, axis=-1)[..., :int(n_samp) + 1])


_SCRIPT_KINDS = ('position', 'velocity', 'acceleration')
SCRIPT_MAX_EVENTS, SCRIPT_MAX_OBSTACLES = 32, 8      # (include/omgx.h omgx_obstacle_script)


def random_obstacle_script(B, n_obst, n_dim, n_events, t_max, scale, seed=0, grid=0.1):
    """A seeded realisation of per-agent obstacle scripts for `BatchP2P.obstacle_script(events=...)`, for tests and studies (the
    counterpart of `input_disturbance`): dict `time` [B, n_events] (uniform in (0, t_max], ascending per agent; every second event
    of an agent is moved onto the next multiple of `grid` -- the update grid of a loop with that update time -- so that on-grid and
    off-grid events both occur), `obstacle` [B, n_events] (0 .. n_obst - 1), `kind` [B, n_events] (0 / 1 / 2 = position / velocity /
    acceleration) and `value` [B, n_events, n_dim] (normal, standard deviation `scale`).  The same arrays for the same arguments."""
    rng = np.random.default_rng(seed)
    B, E = int(B), int(n_events)
    time = rng.uniform(0.0, float(t_max), (B, E))
    on_grid = np.ceil(time / grid) * grid
    time[:, 1::2] = np.minimum(on_grid, np.floor(float(t_max) / grid + 1e-9) * grid)[:, 1::2]
    time = np.sort(np.maximum(time, 1e-3), axis=1)
    return dict(time=time, obstacle=rng.integers(0, int(n_obst), (B, E)).astype(np.int32), kind=rng.integers(0, 3, (B, E)).astype(np.int32),
                value=np.ascontiguousarray(rng.normal(0.0, float(scale), (B, E, int(n_dim)))))


def dual_shift_perm(father, extrapolate=True):
    """perm[r] = row whose multiplier warm-starts row r after the horizon moved by one knot interval (-1: none).  Spline-valued
    constraint entries are indexed by B-spline coefficients: moving the horizon by one interval drops the first `mult` coefficients
    (mult = multiplicity of the interior knots of that entry's basis); scalar rows keep their multiplier.  The rows that enter at
    the end of the horizon have no predecessor: with `extrapolate` they start from the multiplier of the last row that has one (for
    the terminal-slack rows that is the right magnitude: the objective weight of the last coefficients), otherwise from zero (-1)
    -- a zero multiplier on a row that is active at the solution removes that row's curvature from the first Newton system, and the
    first step of the crossing solve is cut to ~1e-6 by the fraction-to-boundary rule."""
    tpl = father.template
    perm = np.arange(tpl.n_con, dtype=np.int64)
    for label, child in father.children.items():
        for cname in child._constraints:
            key = (label, child._add_label(cname))
            off, rows, _ = tpl.con_layout[key]
            if cname not in child._splines_dual:
                continue
            basis = child._splines_dual[cname]['basis']
            interior = basis.knots[(basis.knots > basis.knots[0]) & (basis.knots < basis.knots[-1])]
            if len(interior) == 0:
                continue
            mult = int(np.sum(interior == interior[0]))
            idx = np.arange(rows) + mult
            perm[off:off + rows] = off + np.minimum(idx, rows - 1) if extrapolate else np.where(idx < rows, off + idx, -1)
    return perm


# -- free end time: the step glue of `Point2point(..., freeT=True)` (include/omgx.h OMGX_HAS_FREE_T has the statements) ----------------
FREE_T_REFUSAL = ('%s: not with a free-end-time problem -- the rollout kernel and the plant entries carry one inv_T, '
                  'every agent of this batch has a horizon of its own')


def free_t_basis_tables(basis):
    """(fit [n_fit], proj [len(basis), n_fit]) of a basis with equidistant knots: the reference's `shift_spline(coeffs, s, basis)`
    (`basics/spline_extra.py:88-99`, here `splines.shift_spline_T`) projects the piece on [s, 1] onto the basis with equidistant
    knots on that interval -- the affine image of `basis` itself, so  c' = proj . y,  y_j = spline(s + (1 - s) fit_j)  for every s.
    Any other basis: NotImplementedError."""
    k, d = np.asarray(basis.knots, dtype=float), basis.degree
    inner = k[d:len(k) - d]
    steps = np.diff(inner)
    if (np.any(k[:d + 1] != k[0]) or np.any(k[len(k) - d - 1:] != k[-1]) or k[0] != 0.0 or k[-1] != 1.0 or len(steps) < 1
            or np.any(steps <= 0.0) or np.abs(steps - steps.mean()).max() > 1e-9 * steps.mean()):
        raise NotImplementedError('free end time: the shift of a basis whose knots are not equidistant on [0, 1] is not a constant table')
    fit = basis.fit_points()
    return fit, np.linalg.pinv(basis.eval_basis(fit))


def spline_der_numpy(c, knots, degree, u, dord=0):
    """dord-th derivative (spline-domain units) at the points u [n] of the splines with coefficients c [..., L]: [..., n].  The
    device routines' statements (`spline_der_at`, `span_of`): the span k_j < u <= k_{j+1}, clamped into the basis, so a point a
    rounding error outside [0, 1] is on the polynomial of the nearest span."""
    c, kk, u = np.asarray(c, dtype=float), np.asarray(knots, dtype=float), np.atleast_1d(np.asarray(u, dtype=float))
    dg, nk = int(degree), len(knots)
    j = np.full(u.shape, dg, dtype=np.int64)
    for q in range(dg + 1, nk - dg - 1):
        j = np.where(kk[q] < u, q, j)
    v = [c[..., j - dg + r] for r in range(dg + 1)]
    with np.errstate(divide='ignore', invalid='ignore'):
        for o in range(1, dord + 1):
            for r in range(dg, o - 1, -1):
                i = j - dg + r
                den = kk[i + dg - o + 1] - kk[i]
                v[r] = np.where(den != 0.0, (dg - o + 1) * (v[r] - v[r - 1]) / den, 0.0)
        g = dg - dord
        for lev in range(1, g + 1):
            for r in range(dg, dord + lev - 1, -1):
                i = j - dg + r
                den = kk[i + g - lev + 1] - kk[i]
                a = np.where(den != 0.0, (u - kk[i]) / den, 0.0)
                v[r] = (1.0 - a) * v[r - 1] + a * v[r]
    return v[dg]


def free_t_advance_numpy(x, p, under_way, update_time, ft):
    """`omgx_batch_free_t_advance` in numpy, in place on x [B, n_var], p [B, n_par] and under_way [B] (or None: every agent).  ft: the
    tables of `BatchP2P` for a free-end-time problem -- `o_T`, the plan `coeff_off, n_spl, degree, knots`, `p_off`, `p_t`, `entries`
    [(offset, rows, cols, basis)], `bases` [dict(degree, knots, fit, proj)].  The resample-and-project form, so s = 1 is defined."""
    ut, o_T = float(update_time), ft['o_T']
    n_spl, L = ft['n_spl'], len(ft['knots']) - ft['degree'] - 1
    for b in range(x.shape[0]):
        if under_way is not None and not under_way[b]:
            continue
        T = float(x[b, o_T])
        if not T >= ut:
            if under_way is not None:
                under_way[b] = 0
            continue
        c = x[b, ft['coeff_off']:ft['coeff_off'] + n_spl * L].reshape(n_spl, L)
        for o, off in enumerate(ft['p_off']):
            if off < 0:
                continue
            v = spline_der_numpy(c, ft['knots'], ft['degree'], [ut / T], o)[:, 0]
            for _ in range(o):
                v = v / T
            p[b, off:off + n_spl] = v
        if ft['p_t'] >= 0:
            p[b, ft['p_t']] = 0.0
        dt, rem = (T - ut, T) if T < 2.0 * ut else (ut, T - ut)
        s = dt / rem
        for off, rows, cols, ib in ft['entries']:
            bs = ft['bases'][ib]
            y = spline_der_numpy(x[b, off:off + rows * cols].reshape(cols, rows), bs['knots'], bs['degree'], s + (1.0 - s) * bs['fit'])
            acc = np.zeros((cols, rows))
            for j in range(len(bs['fit'])):             # (ascending, every product and sum rounded on its own)
                acc = acc + bs['proj'][None, :, j] * y[:, j, None]
            x[b, off:off + rows * cols] = acc.reshape(-1)
        x[b, o_T] = rem


def free_t_append_numpy(x, under_way, log, count, overflow, ft, n_samp, sample_time):
    """`omgx_batch_free_t_append` in numpy, in place on log [B, n_der, n_spl, cap], count [B], overflow [B] (or None)."""
    ut, st, o_T = float(ft['update_time']), float(sample_time), ft['o_T']
    n_der, n_spl, cap = log.shape[1], ft['n_spl'], log.shape[3]
    L = len(ft['knots']) - ft['degree'] - 1
    for b in range(x.shape[0]):
        if under_way is not None and not under_way[b]:
            continue
        T = float(x[b, o_T])
        if not T >= st:
            continue
        n_b = int(n_samp) if T >= ut else min(int(n_samp), int(math.floor(T / st + 5e-7)))
        if n_b < 1:
            continue
        inv_T = 1.0 / T
        cnt = int(count[b])
        first = 0 if cnt == 0 else 1
        n_col = n_b + 1 - first
        if cnt < 0 or cnt + n_col > cap:
            if overflow is not None:
                overflow[b] = 1
            continue
        u = np.arange(first, n_b + 1) * (st * inv_T)
        c = x[b, ft['coeff_off']:ft['coeff_off'] + n_spl * L].reshape(n_spl, L)
        for o in range(n_der):
            log[b, o, :, cnt:cnt + n_col] = spline_der_numpy(c, ft['knots'], ft['degree'], u, o) * inv_T ** o
        count[b] = cnt + n_col


class BatchP2P(object):
    """The protocol; the module docstring has the layout."""

    def __new__(cls, problem, P, ops='hip', *args, **kw):
        if cls is BatchP2P:
            if ops != 'hip' and isinstance(ops, str):
                raise ValueError("ops must be 'hip' or an injected host solver object (tests / CPU baseline)")
            cls = DeviceP2P if ops == 'hip' else HostP2P
        return object.__new__(cls)

    def __init__(self, problem, P, ops='hip', device=None, options=None, update_time=0.1,
                 max_iter_step=None, shift_every_spline=True, straggler_first=True, cross_options=None):
        # max_iter_step: iteration cap of a receding-horizon step (default: the cold-solve cap; an agent that hits it keeps its last
        # strictly feasible iterate and restarts cold next step).  shift_every_spline: on a knot crossing shift every spline variable
        # like the generated C++ does (`export/export.py:414-439`); False = the Python rule, names containing 'seg' only
        # (`optilayer.py:482`), which leaves the stale leading coefficient of g* / eps_* (it carries no cost just before the crossing,
        # so the barrier parks it far from its bound).  cross_options: solver options of the step right after a knot crossing (the
        # shifted plan sits on the boundary of the rows that enter the horizon and its multipliers are index-shifted: a wider push
        # into the interior and the barrier parameter of the shifted point itself)
        self.cross_options = dict(cross_options) if cross_options is not None else dict(CROSS_OPTIONS)
        self.problem = problem
        father = problem.father
        self.tpl = tpl = father.template
        if len(problem.vehicles) != 1:
            raise NotImplementedError('BatchP2P drives single-vehicle problems (one agent = one vehicle); '
                                      'a problem with %d vehicles needs the prediction of each of them' % len(problem.vehicles))
        veh = problem.vehicles[0]
        self.veh, self.basis = veh, veh.basis
        self.L, self.n_dim, self.n_spl = len(veh.basis), veh.n_dim, veh.n_spl
        # free end time (`Point2point(..., freeT=True)`): T is a variable of every agent, there is no knot clock
        self._ft = None
        if (problem.label, 'T') in tpl.var_layout:
            self._free_t_tables(problem, cross_options)
        self.T = None if self._ft is not None else float(problem.options['horizon_time'])
        self.knot_time = None if self._ft is not None else float(problem.knot_time)
        self.update_time = float(update_time)
        self.B = P['p'].shape[0]
        self.o_spl = tpl.entry_range(veh.label, 'splines_seg0', 'var')[0]
        # initial conditions the prediction writes: time derivatives 0, 1, (2) of the plan at the time of the next solve
        # (`vehicles/holonomic.py:88-89,153-159`: state0, input0; `vehicles/quadrotor.py:76-85,110-114`: spl0, dspl0, ddspl0)
        names = ('spl0', 'dspl0', 'ddspl0') if (veh.label, 'spl0') in tpl.par_layout else ('state0', 'input0')
        self.p_offs = [tpl.entry_range(veh.label, nm, 'par')[0] for nm in names]
        self.o_state0, self.o_input0 = self.p_offs[0], self.p_offs[1]
        self.o_t = tpl.entry_range(problem.label, 't', 'par')[0]
        # obstacle motion model between two solves (`environment/obstacle.py:246-264` without bouncing):
        # the parameters x, v, a of every obstacle are the values AT the time of the solve
        # (`obstacle.py:142-155` reads signals[...][:, -1]; the template extrapolates them back by t)
        self.obst = []
        for obs in problem.environment.obstacles:
            ox, ov, oa = (tpl.entry_range(obs.label, nm, 'par') for nm in ('x', 'v', 'a'))
            if np.any(P['p'][:, ov[0]:ov[1]] != 0.) or np.any(P['p'][:, oa[0]:oa[1]] != 0.):     # static obstacles: nothing to do
                self.obst.append((ox[0], ov[0], oa[0], ox[1] - ox[0]))
        # (a problem loaded from a bundle, `omgtools.workloads`, brings the multiplier map of a knot crossing with it)
        self.perm = father.dual_perm if hasattr(father, 'dual_perm') else dual_shift_perm(father)
        ents, mats, off = [], [], 0
        for label, name, spl in (father.shifted_entries(every_spline=shift_every_spline) if self._ft is None else ()):
            lo, rows, cols = tpl.var_layout[(label, name)]
            Tm = shiftoverknot_T(spl['basis'])
            ents.append([lo, rows, cols, off])
            mats.append(Tm.reshape(-1))
            off += Tm.size
        self.shift_entries = np.array(ents, dtype=np.int32).reshape(-1, 4)
        self.shift_mats = np.concatenate(mats) if mats else np.zeros(0)
        self._shift_dense = [(e, m.reshape(e[1], e[1])) for e, m in zip(ents, mats)]
        self.time = 0.0
        self.under_way, self.stop_tol = None, 1e-3        # (stop_at_arrival)
        self._sig = None                                  # (record_signals)
        self._pl = None                                   # (plant)
        self._fb = None                                   # (feedback)
        self._sc = None                                   # (obstacle_script)
        self._ms = None                                   # (mission)
        self._x0 = P['x0']                                # (the batch's first guess: `mission` keeps its agent-independent part)
        self._plan_ready = False                          # (solve_cold has run: x holds a plan)
        # (warm_mu_factor 0.1: a step starts at the barrier parameter the previous solve of the agent ended with, tol / 10,
        # unless the shifted point is far off that central path -- a tenth of its average complementarity then: at tol 1e-3
        # the same iterates as factor 0, at 1e-6 0.03 % instead of 0.4 % of the steps end at the iteration cap)
        self.opts = dict(tol=1e-3, max_iter=300, warm_mu_factor=0.1, warm_z_floor=0.1, warm_z_cap=0.0)
        self.opts.update(options or {})
        self.max_iter_cold = self.opts['max_iter']
        from .backend import DEFAULT_OPTIONS
        self._base_extra = dict((k, self.opts.get(k, DEFAULT_OPTIONS[k])) for k in self.cross_options)   # (what a non-crossing step resets them to)
        self.max_iter_step = int(max_iter_step) if max_iter_step else self.max_iter_cold
        self.straggler_first = bool(straggler_first)
        self._allocate(P, ops, device)
        if self._ft is not None:
            self._ft.update(coeff_off=self.o_spl, n_spl=self.n_spl, degree=self.basis.degree, knots=np.asarray(self.basis.knots, dtype=float),
                            p_off=list(self.p_offs), p_t=self.o_t, update_time=self.update_time)
            self._free_t_set()

    def _free_t_tables(self, problem, cross_options):
        """The tables of a free-end-time batch (`self._ft`): where T sits in x, and per entry of `father.shifted_entries()` -- the
        entries `FreeTPoint2point.init_step` re-expresses -- its block of x and the (fit, proj) tables of its basis."""
        father, tpl = problem.father, problem.father.template
        if hasattr(father, 'dual_perm') or not hasattr(problem, 'init_step'):
            raise NotImplementedError('BatchP2P: a free-end-time problem loaded from a bundle carries no bases for its shift; build it through the front end')
        if cross_options:
            raise ValueError('BatchP2P: cross_options belong to a knot crossing; a free-end-time problem has no knot clock')
        lay, label = tpl.par_layout, problem.vehicles[0].label
        if any((label, nm) not in lay for nm in ('state0', 'input0', 'poseT')):
            raise NotImplementedError('BatchP2P: free end time is carried for the point-mass classes (state0 / input0 / poseT: Holonomic, Holonomic3D)')
        from .backend import FREE_T_MAX_BASIS, FREE_T_MAX_ENT, FREE_T_MAX_FIT, FREE_T_MAX_ROWS
        bases, index, entries = [], {}, []
        for lbl, name, spl in father.shifted_entries():
            basis = spl['basis']
            if basis not in index:
                fit, proj = free_t_basis_tables(basis)
                index[basis] = len(bases)
                bases.append(dict(degree=basis.degree, knots=np.asarray(basis.knots, dtype=float), fit=fit, proj=np.ascontiguousarray(proj)))
            lo, rows, cols = tpl.var_layout[(lbl, name)]
            entries.append((int(lo), int(rows), int(cols), index[basis]))
        if (len(entries) > FREE_T_MAX_ENT or len(bases) > FREE_T_MAX_BASIS or any(len(bs['fit']) > FREE_T_MAX_FIT for bs in bases)
                or any(e[1] > FREE_T_MAX_ROWS for e in entries)):
            raise NotImplementedError('BatchP2P: the free-end-time shift tables exceed the limits of omgx_batch_set_free_t (include/omgx.h)')
        self._ft = dict(o_T=tpl.entry_range(problem.label, 'T', 'var')[0], entries=entries, bases=bases)

    def horizon(self):
        """[B]: the current motion time T of every agent of a free-end-time batch (a copy of x[:, o_T])."""
        if self._ft is None:
            raise RuntimeError('horizon(): the horizon of a fixed-T batch is `self.T`')
        o = self._ft['o_T']
        return self.x[:, o].clone() if hasattr(self.x, 'clone') else self.x[:, o].copy()

    # -- solves ------------------------------------------------------------------------
    def solve_cold(self, bends=(1.0, -1.0, 2.5, -2.5), fused=True):
        """Cold solve from the reference's initial guess (`get_init_spline_value`: coefficients on the straight line).  Agents that do
        not converge from it (phase I stalls: e.g. 5 % of the Quadrotor class with its five moving obstacles) are solved again from the
        same guess bent sideways by `bends[0]`, then `bends[1]` ... metres at mid-course -- a different side of the obstacles; the
        reference has no such retry (its user would re-initialise by hand), `bends=()` switches it off.  fused: the restarts run inside
        the launch of the first attempt (`omgx_batch_set_restarts`), else as separate passes over the failed agents (`restart_failed`)
        -- same guesses, same results.  Returns the largest number of restarts an agent needed (a host solver object has none: 0)."""
        self._plan_ready = True
        # the log (record_signals) takes the cold plan ONCE, after the last restart pass: the log inside the solve stays off during
        # the cold solve (an agent that a restart solves again must not be logged twice) and one stand-alone append follows
        log = self._sig is not None and self._pl is None      # (with the plant in the loop the fused log is off anyway: its simulate writes the log)
        fused_log = log and self._ft is None                  # (free end time: the append is a launch of its own behind every solve)
        if fused_log:
            self._signals_fused(False)
        try:
            n_restarts = self._cold(bends, fused)
        finally:
            if fused_log:
                self._signals_fused(True)
        if log:
            self._signals_append_now()
        if self._pl is not None:
            self._plant_simulate()                          # the vehicle travels the first update, from the plan's own sample 0
        return n_restarts

    def restart_failed(self, bends=(1.0, -1.0, 2.5, -2.5)):
        """Restart passes of a cold solve (see solve_cold); returns how many were needed."""
        return 0

    # -- one receding-horizon step ---------------------------------------------------------
    def step(self, events=None, before_solve=None, states=None, inputs=None, fresh=None, enforce=False):
        """before_solve(self): called between the glue of the step (prediction, obstacles, shift: p and x are what the
        solve will read) and the solve -- where a caller with host buffers uploads its parameters (bench.py's pipelined
        host-boundary leg).

        states [B, n_spl] (after `feedback`): the states measured at the start of the update that ends now -- the reference's
        `Deployer.update(current_time, states, ...)` -> `Vehicle.predict(state0=...)`.  Part (1) of the step is then the measured
        prediction: the solve starts from `states` integrated over the update under the current plan's inputs.  fresh [B] (0 / 1,
        None: all): an agent with 0 has no measurement at this update and is predicted from its plan.  enforce: the solve starts
        from `states` as they are, with `inputs` [B, n_spl] (None: zero) as its initial input (`enforce_states` / `enforce_inputs`).
        Device loop: device or pinned host tensors (include/omgx.h omgx_batch_predict_measured); host loop: arrays."""
        if self._ms is not None:
            raise RuntimeError('step(): a mission is on -- its agents run on clocks of their own and a solve launch has one option set and '
                               'one clock: step with rollout(1)')
        if self._ft is not None:
            if states is not None or inputs is not None or fresh is not None or enforce:
                raise NotImplementedError(FREE_T_REFUSAL % 'step(states=...)')
            return self._step_free_t(events, before_solve)
        if states is None:
            if inputs is not None or fresh is not None or enforce:
                raise ValueError('step: inputs / fresh / enforce go with states')
        else:
            if self._fb is None:
                raise RuntimeError('step(states=...): call feedback() first (it fixes the sample grid of the prediction)')
            if self._pl is not None:
                raise ValueError('step(states=...): the plant is in the loop; a loop has one source of states')
            if inputs is not None and not enforce:
                raise ValueError('step: inputs are read with enforce=True only')
            if inputs is not None and self._fb.get('model') == 'quadrotor':
                raise ValueError("step: inputs are not read with model='quadrotor' (`Quadrotor.set_initial_conditions` ignores them)")
            for nm, a, shape in (('states', states, (self.B, self._state_width())), ('inputs', inputs, (self.B, self.n_spl)), ('fresh', fresh, (self.B,))):
                if a is not None and tuple(a.shape) != shape:
                    raise ValueError('step: %s must be %s, got %s' % (nm, list(shape), list(a.shape)))
        t_now, tau, t_rel, crossed = step_clock(self.time, self.update_time, self.knot_time, self.T)
        # (1) ideal prediction on the current plan, (2) horizon bookkeeping: the initial conditions from the plan at tau and the new t
        # (with the plant in the loop: from the state the vehicle had one update ago, and the stop test on the travelled state;
        # with measured states: from those)
        if states is not None:
            self._feedback_predict(tau, t_rel, states, inputs, fresh, bool(enforce))
        elif self._pl is None:
            self._predict(tau, t_rel)
        else:
            self._plant_predict(tau, t_rel)
        self._advance_obstacles(self.time, t_now)            # (a no-op for static obstacles)
        if crossed:
            self._shift()
        self.time = t_now
        if before_solve is not None:
            before_solve(self)
        # (3) warm-started solve (ordered: `_predict` has asked for the launch order already)
        self._solve(True, events, ordered=True, extra=self.cross_options if crossed else None)
        if self._pl is not None:
            self._plant_simulate()                          # (4) the vehicle travels the update
        return crossed

    def _step_free_t(self, events, before_solve):
        """`step` of a free-end-time batch (`FreeTPoint2point`: `stop_criterium`, `init_step`, `Vehicle.predict`, solve, `simulate`):
        (1) advance -- per agent under way the stop clause T < update_time, the prediction on the old plan and the old T, the plan
        re-expressed on what is left of it, T reduced (include/omgx.h omgx_batch_free_t_advance); (2) obstacle motion, t = 0 in this
        class; (3) warm-started solve, with the arrival test of `stop_at_arrival` inside it; (4) with `record_signals` the append on
        every agent's own horizon.  `time` advances by `update_time`; nothing crosses a knot."""
        t_now = self.time + self.update_time
        self._free_t_advance()
        self._advance_obstacles(self.time, t_now)
        self.time = t_now
        if before_solve is not None:
            before_solve(self)
        self._solve(True, events)
        if self._sig is not None:
            self._signals_append_now()
        return False

    def rollout(self, n_steps, iters_log=None, status_log=None):
        """`n_steps` receding-horizon steps of every agent in ONE launch (`omgx_batch_rollout`): per agent the statements of `step` --
        prediction, obstacles, knot-crossing shift, warm-started solve -- in the same order with the same numbers, without the barrier
        between the steps of different agents (they are independent problems: each vehicle of the reference runs its own
        `Deployer.update` loop).  After `plant` the vehicle of every agent is simulated inside the launch too -- prediction from the
        travelled state, input disturbance, stop test on the travelled state: a disturbance study of a whole fleet in one launch.  A
        deployment that feeds states measured outside back steps with `step` (`feedback`, `step(states=...)`): a rollout takes none.
        Returns the number of knot crossings."""
        if self._ft is not None:
            raise NotImplementedError(FREE_T_REFUSAL % 'rollout')
        if self._pl is not None and self._pl.get('model') == 'quadrotor':
            raise NotImplementedError("rollout: the Quadrotor's plant runs per step only (`step`): the rollout kernel has no instance for it")
        if self._ms is not None:
            return self._mission_rollout(int(n_steps), iters_log, status_log)
        clock, t, t_abs = [], self.time, [self.time]
        for _ in range(int(n_steps)):
            t, tau, t_rel, crossed = step_clock(t, self.update_time, self.knot_time, self.T)
            clock.append((tau, t_rel, crossed))
            t_abs.append(t)
        self._rollout(*([c[k] for c in clock] for k in range(3)), iters_log=iters_log, status_log=status_log, t_abs=t_abs)
        self.time = t
        return int(sum(c[2] for c in clock))

    def _rollout(self, tau, t_rel, crossed, iters_log, status_log, t_abs=None):
        raise NotImplementedError('rollout is a device launch')

    # -- missions: a list of goals per agent -------------------------------------------------------------
    def mission(self, goals, n_goals=None, on=True):
        """Give every agent a list of goals to fly one after the other inside `rollout`, as the reference's examples do with a second
        `simulator.run()` after `vehicle.set_terminal_conditions(...)` or a `Deployer` loop over via points (include/omgx.h
        OMGX_HAS_MISSION has the statements).  goals [B, G, n_dim]: the goals AFTER the one already in p[poseT]; n_goals [B] (0 .. G,
        default G): how many of them an agent flies.  Needs `stop_at_arrival`: arrival is that rule (with `plant`: the plant's, on the
        travelled state).  From now on, when the rule holds for an agent at the head of a step of `rollout` and it has a goal left, that
        step starts the next leg instead of ending the loop: poseT <- the goal, the plan <- the reference's fresh guess (per axis
        `np.linspace` from the state0 of the PREVIOUS update, one update stale as in the reference, to the goal; every other variable
        the agent-independent value of the batch's first guess), multipliers <- 0, state0 <- the state the vehicle is in now, input0
        <- 0, t <- 0, and a cold solve (`max_iter` of `solve_cold`, the base options, no bends); from there the agent runs on its own
        clock, the leg's.  Only arrival at the last goal clears `under_way[b]`.  `mission_state()` returns `leg` [B] (index of the goal
        being flown, 0 = the one in p), `clock` [B] (receding-horizon steps of the current leg behind its first solve; starts at the
        batch's own count) and `arrivals` [B, 1 + G] (the rollout step, counted from this call, at whose head each goal was found
        reached; -1: not yet).  `rollout(1)` is the per-step form; `step()` is refused (a solve launch has one option set and one
        clock).  The batch's own `time` stays the absolute clock on the update grid.  Point-mass classes; not with an obstacle script,
        the Quadrotor's plant or a host pool.  on=False: the stop rule ends loops again."""
        if not on:
            self._ms = None
            return self._mission_off()
        if self._ft is not None:
            raise NotImplementedError(FREE_T_REFUSAL % 'mission')
        if self.under_way is None:
            raise RuntimeError('mission(): call stop_at_arrival() first -- arriving is that rule')
        if getattr(self, 'pool', None) is not None:
            raise NotImplementedError('mission: not with a host pool (its workers run the step glue themselves)')
        if self._sc is not None:
            raise NotImplementedError('mission: not with an obstacle script (the rollout kernel has no script x mission instance)')
        if self._pl is not None and self._pl.get('model') == 'quadrotor':
            raise NotImplementedError("mission: not with the Quadrotor's plant (it runs per step only, a mission inside `rollout`)")
        o_pose = self._o_pose('mission')
        if self.n_spl != self.n_dim:
            raise NotImplementedError('mission(): the fresh guess of a leg is the point-mass classes\' (one spline per axis)')
        goals = np.ascontiguousarray(goals, dtype=float)
        if goals.ndim != 3 or goals.shape[0] != self.B or goals.shape[1] < 1 or goals.shape[2] != self.n_dim or not np.isfinite(goals).all():
            raise ValueError('mission: goals must be finite [B, G, n_dim] = [%d, G >= 1, %d], got %s' % (self.B, self.n_dim, list(goals.shape)))
        G = goals.shape[1]
        n_goals = np.full(self.B, G, dtype=np.int32) if n_goals is None else np.asarray(n_goals)
        if n_goals.shape != (self.B,) or n_goals.dtype.kind not in 'iu' or (n_goals < 0).any() or (n_goals > G).any():
            raise ValueError('mission: n_goals must be [B] integers in 0 .. %d' % G)
        x0 = np.asarray(self._x0, dtype=float)
        blk = np.ones(self.tpl.n_var, dtype=bool)
        blk[self.o_spl:self.o_spl + self.n_spl * self.L] = False
        if (x0[:, blk] != x0[0, blk]).any():
            raise ValueError('mission: the first guess x0 differs between agents outside the spline block; a leg restarts from one row')
        # the leg clock carries on from the batch's: the number of updates `step_clock` needs from 0 to the batch's time
        t, n_upd = 0.0, 0
        while t < self.time - 1e-9:
            t, n_upd = step_clock(t, self.update_time, self.knot_time, self.T)[0], n_upd + 1
        if abs(t - self.time) > 1e-9:
            raise ValueError('mission: the batch time %g is not on the update grid' % self.time)
        ms = dict(G=G, o_pose=o_pose, x_reset=np.ascontiguousarray(x0[0]).copy(), steps=0)
        ms.update(self._mission_alloc(goals, n_goals.astype(np.int32), n_upd))
        self._ms = ms

    def mission_state(self):
        """dict `leg` [B], `clock` [B], `arrivals` [B, 1 + G] of `mission` (int32; device tensors on the device loop, arrays on the host loop)."""
        if self._ms is None:
            raise RuntimeError('mission_state(): call mission() first')
        return dict((nm, self._ms[nm]) for nm in ('leg', 'clock', 'arrivals'))

    def mission_advance(self):
        """The arrival test and the leg switch of `mission` WITHOUT the solve, on the batch as it stands (`omgx_batch_mission_advance`):
        an agent under way for which the rule holds starts its next leg -- the guess runs from p[state0] as it stands, state0 is where
        the vehicle is (p[state0]; with `plant` the travelled state) -- or, at its last goal, stops.  Counts as one rollout step in
        `arrivals`.  How the switch is looked at on its own: behind a solve the guess is gone."""
        if self._ms is None:
            raise RuntimeError('mission_advance(): call mission() first')
        self._mission_advance(self._ms['steps'])
        self._ms['steps'] += 1

    def _mission_table(self, n):
        """The step records (tau, t_rel, crossed) of a leg's clock 0 .. n - 1: `step_clock` iterated from the leg-local time 0 -- the
        same table for every agent and every leg, and for the first leg the records of the batch's own clock."""
        out, t = [], 0.0
        for _ in range(int(n)):
            t, tau, t_rel, crossed = step_clock(t, self.update_time, self.knot_time, self.T)
            out.append((tau, t_rel, crossed))
        return out

    def _mission_rollout(self, n_steps, iters_log, status_log):
        if n_steps < 1:
            raise ValueError('rollout: n_steps must be positive')
        if self._sc is not None:
            raise NotImplementedError('rollout: a mission and an obstacle script are both on (the rollout kernel has no script x mission instance)')
        table = self._mission_table(self._mission_clock_max() + n_steps)
        t, crossings = self.time, 0
        for _ in range(n_steps):      # (the batch's own clock: absolute, on the update grid, whatever the legs do)
            t, _, _, crossed = step_clock(t, self.update_time, self.knot_time, self.T)
            crossings += int(crossed)
        self._mission_run(table, n_steps, iters_log, status_log)
        self._ms['steps'] += n_steps
        self.time = t
        return crossings

    # -- obstacle scripts ----------------------------------------------------------------------------
    def _advance_obstacles(self, t_prev, t_now):
        """Part of `step`: the obstacles move from t_prev to t_now -- constant acceleration, and with a script (`obstacle_script`) its
        jumps."""
        if self._sc is None:
            advance_obstacles(self.p, self.obst, self.update_time)
        else:
            self._script_advance(t_prev, t_now)

    def obstacle_script(self, events=None, on=True):
        """Move the obstacles as the reference's `simulation={'trajectories': {...}}` does (`environment/obstacle.py:172-264`): at given
        times a value is added to an obstacle's position, velocity or acceleration, between these jumps it moves with constant
        acceleration.  From now on every `step` and every step inside a `rollout` launch carries the obstacles over its update with
        these events (include/omgx.h OMGX_HAS_OBSTACLE_SCRIPT has the statement: exact for the model, split at the event times, no
        sample grid); an update without an event is the plain motion, bit for bit.
        events=None: the script of the problem's own obstacles (`obstacle.simulation['trajectories']`), the same for every agent; a
        problem loaded from a bundle carries none.  Otherwise a dict of per-agent scripts: `time` [B, E] (absolute loop time, as
        `self.time`; +inf: no event), `obstacle` [B, E] (index into `problem.environment.obstacles`), `kind` [B, E] (0 / 1 / 2 =
        position / velocity / acceleration), `value` [B, E, n_dim].  Events are sorted per agent (events at one time keep their
        order) and padded.  Refused: an event at or before the current time (the reference folds an event at time 0 into the initial
        state: put it into `P`), more than 32 events of an agent, more than 8 moving obstacles.  Every obstacle an event names joins
        the moving obstacles, even when its v and a are zero in `P`.  Not modelled: `bounce`, a custom `simulation['model']`, obstacle
        `input` trajectories.
        Stopped agents: `step` advances every agent's obstacles, stopped or not; inside a `rollout` launch an agent's obstacles move
        only while its loop runs.  on=False: the plain motion again (obstacles an event has set moving keep moving)."""
        if not on:
            self._sc = None
            return
        if getattr(self, 'pool', None) is not None:
            raise NotImplementedError('obstacle_script: not with a host pool (its workers run the step glue themselves)')
        if self._ms is not None:
            raise NotImplementedError('obstacle_script: a mission is on (the rollout kernel has no script x mission instance)')
        obstacles = self.problem.environment.obstacles
        if events is None:
            rows = []
            for q, obs in enumerate(obstacles):
                sim = getattr(obs, 'simulation', None)
                if sim is None:
                    raise ValueError('obstacle_script: this problem comes from a bundle, its obstacles carry no simulation: pass events=')
                if 'model' in sim or 'input' in sim.get('trajectories', {}):
                    raise NotImplementedError("obstacle_script: a custom simulation['model'] / an 'input' trajectory is not moved in the batched loop")
                for kind, traj in sim.get('trajectories', {}).items():
                    if len(traj['time']) != len(traj['values']):
                        raise ValueError('Dimension mismatch between time array and values for ' + kind + ' trajectory.')
                    rows += [(float(tau), q, _SCRIPT_KINDS.index(kind), np.asarray(val, dtype=float)) for tau, val in zip(traj['time'], traj['values'])
                             if tau != 0]
            if not rows:
                raise ValueError('obstacle_script: no obstacle of the problem has a trajectory: pass events=')
            events = dict(time=np.tile([r[0] for r in rows], (self.B, 1)), obstacle=np.tile([r[1] for r in rows], (self.B, 1)),
                          kind=np.tile([r[2] for r in rows], (self.B, 1)), value=np.zeros((self.B, len(rows), 3)))
            for e, r in enumerate(rows):
                events['value'][:, e, :len(r[3])] = r[3]
        time = np.array(events['time'], dtype=float)
        which, kind, val = np.array(events['obstacle'], dtype=np.int64), np.array(events['kind'], dtype=np.int64), np.asarray(events['value'], dtype=float)
        if time.ndim != 2 or time.shape[0] != self.B or which.shape != time.shape or kind.shape != time.shape or val.shape[:2] != time.shape or \
                val.ndim != 3 or val.shape[2] > 3:
            raise ValueError('obstacle_script: events must be time / obstacle / kind [B, E] and value [B, E, n_dim] with B = %d' % self.B)
        live = time < np.inf
        if np.isnan(time).any() or (live & (time <= self.time + SCRIPT_EPS)).any():
            raise ValueError('obstacle_script: an event at or before the current time %g (an event at the start belongs into P)' % self.time)
        if live.sum(axis=1).max(initial=0) > SCRIPT_MAX_EVENTS:
            raise ValueError('obstacle_script: %d events of one agent, at most %d' % (live.sum(axis=1).max(), SCRIPT_MAX_EVENTS))
        if not live.any():
            raise ValueError('obstacle_script: no event')
        if (which[live] < 0).any() or (which[live] >= len(obstacles)).any() or (kind[live] < 0).any() or (kind[live] > 2).any():
            raise ValueError('obstacle_script: obstacle outside 0 .. %d or kind outside 0 .. 2' % (len(obstacles) - 1))
        obst, slot = list(self.obst), {}
        for q in sorted(set(which[live].tolist())):
            ox, ov, oa = (self.tpl.entry_range(obstacles[q].label, nm, 'par') for nm in ('x', 'v', 'a'))
            entry = (ox[0], ov[0], oa[0], ox[1] - ox[0])
            if entry not in obst:
                obst.append(entry)
            slot[q] = obst.index(entry)
        if len(obst) > SCRIPT_MAX_OBSTACLES:
            raise ValueError('obstacle_script: %d moving obstacles, at most %d' % (len(obst), SCRIPT_MAX_OBSTACLES))
        E = max(1, int(live.sum(axis=1).max()))
        order = np.argsort(time, axis=1, kind='stable')[:, :E]
        take = lambda a: np.take_along_axis(a, order, axis=1)
        time, live = take(time), take(live)
        what = np.where(live, np.vectorize(lambda q: slot.get(q, 0))(take(which)) * 3 + take(kind), 0).astype(np.int32)
        value = np.zeros((self.B, E, 3))
        value[:, :, :val.shape[2]] = np.take_along_axis(val, order[:, :, None], axis=1)
        value[~live] = 0.0
        self.obst = obst
        self._sc = self._script_alloc(np.ascontiguousarray(time), np.ascontiguousarray(what), value)

    def _eval_rows(self, tau):
        """[E_0, E_1, ...]: c @ E_o = o-th time derivative of the plan at tau."""
        rows = [self.basis.eval_basis([tau])[0]]
        for o in range(1, len(self.p_offs)):
            dbasis, Po = self.basis.derivative(o)
            rows.append(dbasis.eval_basis([tau])[0] @ Po / self.T ** o)
        return rows

    # -- the reference's stop criterion ----------------------------------------------------------
    def _o_pose(self, who, point_mass=True):
        """Offset of poseT in p, for the method `who` that reads it (point_mass: and state0 / input0)."""
        lay, label = self.tpl.par_layout, self.veh.label
        if (label, 'poseT') not in lay or (point_mass and (label, 'state0') not in lay):
            raise NotImplementedError('%s(): the class has no %s' % (who, 'state0 / input0 / poseT parameters' if point_mass else 'poseT parameter'))
        return self.tpl.entry_range(label, 'poseT', 'par')[0]

    def arrived(self, stop_tol=1e-3):
        """Per agent: the reference's `stop_criterium` (`problems/point2point.py:98-102` -> `vehicles/holonomic.py:145-151`,
        `holonomic3d.py`: |state - poseT| <= stop_tol and |input| <= stop_tol, Euclidean norms, `stop_tol` = 1e-3 by default,
        `vehicles/vehicle.py:72`) on the state the last prediction wrote into p -- the state the vehicle is in at the time of
        the current update (with `step(states=...)`: the state predicted from the measurement, or the enforced one) -- or, after `plant`,
        on the travelled state and the last applied input.  Boolean tensor (device loop) / array (host loop); the reference's `Simulator.run` ends a vehicle's
        loop at the first update for which this holds (`execution/simulator.py:39-62`).  Point-mass classes (state0 / input0 / poseT);
        with `plant(model='quadrotor')` the Quadrotor's own rule (`vehicles/quadrotor.py:104-110`): the travelled position against poseT
        and the plan's velocity at the last travelled sample."""
        pl = getattr(self, '_pl', None)
        if pl is not None and pl.get('model') == 'quadrotor':
            pose = self.p[:, pl['o_pose']:pl['o_pose'] + 2]
            return (self._norm(pl['state'][:, :2] - pose) <= stop_tol) & (self._norm(pl['dspl_last']) <= stop_tol)
        st, inp, pose = (self.p[:, o:o + self.n_dim] for o in (self.o_state0, self.o_input0, self._o_pose('arrived')))
        if pl is not None:      # (with the plant in the loop: the travelled state and the last applied input, `signals[...][:, -1]`)
            st, inp = pl['state'], pl['input_last']
        return (self._norm(st - pose) <= stop_tol) & (self._norm(inp) <= stop_tol)

    def stop_at_arrival(self, stop_tol=1e-3, on=True):
        """End every agent's loop where the reference's does: from now on an agent for which `arrived(stop_tol)` holds at an update
        is not solved at that update or any later one (`execution/simulator.py:39-62` leaves its `while` loop; a fleet's
        vehicles arrive at different updates) -- it keeps its plan, its multipliers and its status, `iters` reads 0.  Device loop:
        the rule is the solve kernel's (`omgx_batch_set_stop`, no launch of its own); `under_way` [B] (int32 tensor / bool array)
        holds who is still running.  The agents under way are solved exactly as without the rule.  `rollout` applies it too: an agent's
        loop inside the launch ends at the step its state meets the criterion (its plan stays as it is at that step).  With
        `step(states=...)` the rule still tests p[state0], p[input0]: now the state predicted from the measurement (or the enforced
        state and input), not the measurement itself."""
        if on and self._pl is not None and self._pl.get('model') == 'quadrotor':
            o_pose = self._pl['o_pose']                     # (the rule of `plant(model='quadrotor')`, on the travelled state)
        else:
            o_pose = self._o_pose('stop_at_arrival') if on else None
        if on:
            self.stop_tol = float(stop_tol)
        elif self._ms is not None:
            self.mission(None, on=False)                    # (a mission is a use of the rule: it goes with it)
        self._stop_rule(o_pose)

    # -- the travelled trajectories ----------------------------------------------------------------
    def record_signals(self, sample_time=0.01, max_updates=200, on=True, cap=None):
        """Keep the trajectories the vehicles actually travel, as the reference's `Simulator.run` returns them in `vehicle.signals`
        (`Vehicle.simulate` with `ideal_update`, `vehicles/vehicle.py:359-369`): after every update the samples 1 .. n_samp of the fresh
        plan (n_samp = update_time / sample_time), ahead of the first also sample 0.  From now on `solve_cold` (once, after its last
        restart pass), every `step` and every step inside a `rollout` launch append for the agents they solved -- inside the solve /
        rollout kernel on the device loop (`omgx_batch_set_signals`), so a whole manoeuvre in one launch leaves its whole log.  An agent
        the stop rule has stopped is not appended; one whose solve did not succeed is (the loop carries on with that plan).  Room for
        `max_updates` updates: cap = 1 + n_samp * max_updates columns per agent; an append beyond it writes nothing and sets
        `overflow` (cap=: another number of columns, at least n_samp + 1).  Called after `solve_cold`, the current plan is appended before the call returns: the log always starts with the plan
        the loop starts from.  State, input and dinput (time-derivative orders 0, 1, 2 of the plan) are kept.  on=False drops the log."""
        if not on:
            if self._sig is not None:
                self._signals_fused(False)
            self._sig = None
            return
        n_samp = int(round(self.update_time / float(sample_time), 6))
        if n_samp < 1 or int(max_updates) < 1:
            raise ValueError('record_signals: sample_time must not exceed update_time and max_updates must be positive')
        if self._fb is not None and self._fb['sample_time'] != float(sample_time):
            raise ValueError('record_signals: measured states are integrated with sample_time %g (feedback)' % self._fb['sample_time'])
        if self._pl is not None:
            if self._pl['sample_time'] != float(sample_time):
                raise ValueError('record_signals: the plant is simulated with sample_time %g' % self._pl['sample_time'])
            if self._plan_ready:
                raise RuntimeError('record_signals: with the plant in the loop the log starts with the first plan -- call it before solve_cold')
        n_der = min(3, self.basis.degree + 1)
        cap = 1 + n_samp * int(max_updates) if cap is None else int(cap)
        if cap < n_samp + 1:
            raise ValueError('record_signals: cap = %d holds less than the first append (%d columns)' % (cap, n_samp + 1))
        sig = dict(sample_time=float(sample_time), n_samp=n_samp, cap=cap, n_der=n_der, t_start=self.time)
        sig['log'], sig['count'], sig['overflow'] = self._signals_alloc((self.B, n_der, self.n_spl, cap))
        self._sig = sig
        if self._pl is not None:
            return                                          # (the plant's simulate writes the log: the fused spline log stays off)
        if self._ft is None:                                # (free end time: the append is a launch of its own behind every solve, `step`)
            self._signals_fused(True)
        if self._plan_ready:
            self._signals_append_now()

    # -- the plant in the loop --------------------------------------------------------------------
    def _quad_model(self, who, model):
        """The check behind `plant(model=...)` / `feedback(model=...)`: the one model there is, on a class that can carry it."""
        if model != 'quadrotor':
            raise ValueError("%s: model must be None (an integrator class) or 'quadrotor', got %r" % (who, model))
        lay, label = self.tpl.par_layout, self.veh.label
        if any((label, nm) not in lay for nm in ('spl0', 'dspl0', 'ddspl0', 'poseT')) or self.n_spl != 2 or self.basis.degree < 3:
            raise ValueError("%s: model='quadrotor' needs the parameters spl0 / dspl0 / ddspl0 / poseT, two splines and degree >= 3; %s has "
                             'n_spl = %d, degree = %d' % (who, label, self.n_spl, self.basis.degree))

    def _state_width(self):
        """Entries of a measured state in `step(states=...)`: n_spl for the integrator classes, 5 with `feedback(model='quadrotor')`."""
        return 5 if self._fb is not None and self._fb.get('model') == 'quadrotor' else self.n_spl

    def _plant_quadrotor(self, sample_time, max_updates, disturbance, time_constant, gravity):
        """`plant(model='quadrotor')`: the Quadrotor's own model in the loop (include/omgx.h OMGX_HAS_PLANT_QUADROTOR)."""
        self._quad_model('plant', 'quadrotor')
        if self._ms is not None:
            raise NotImplementedError("plant(): model='quadrotor' runs per step only, a mission inside `rollout`")
        if time_constant is not None:
            raise NotImplementedError("plant(): the first-order actuator lag is not simulated with model='quadrotor'")
        if self._plan_ready:
            raise RuntimeError('plant(): the vehicle starts from the first plan -- call it before solve_cold')
        n_samp = int(round(self.update_time / float(sample_time), 6))
        if n_samp < 1 or int(max_updates) < 1:
            raise ValueError('plant: sample_time must not exceed update_time and max_updates must be positive')
        if n_samp + 1 > 64:
            raise ValueError("plant: model='quadrotor' takes at most 63 samples per update, got %d" % n_samp)
        if not float(gravity) > 0.0:
            raise ValueError('plant: gravity must be positive')
        for what, g in (('log is kept', self._sig), ('measured states are integrated', self._fb)):
            if g is not None and g['sample_time'] != float(sample_time):
                raise ValueError('plant: the %s with sample_time %g' % (what, g['sample_time']))
        shape = (self.B, 2, int(max_updates), n_samp + 1)
        if disturbance is not None and tuple(disturbance.shape) != shape:
            raise ValueError('plant: disturbance must be [B, 2, max_updates, n_samp + 1] = %s, got %s' % (shape, tuple(disturbance.shape)))
        pl = dict(sample_time=float(sample_time), n_samp=n_samp, max_updates=int(max_updates), lag=None, model='quadrotor', g=float(gravity),
                  o_pose=self.tpl.entry_range(self.veh.label, 'poseT', 'par')[0])
        pl.update(self._plant_alloc(disturbance, 'quadrotor'))
        self._pl = pl
        self._signals_fused(False)                          # (the simulate writes the log, whichever of `record_signals` and this came first)

    def _plant_log(self):
        """(state [B, 5, cap], input [B, 2, cap]): the arrays the Quadrotor's simulate logs into next to the spline log, made when the
        log is first met; (None, None) without a log."""
        pl, sig = self._pl, self._sig
        if sig is None:
            pl.pop('log_state', None), pl.pop('log_input', None)
            return None, None
        if 'log_state' not in pl or pl['log_state'].shape[2] != sig['cap']:
            pl['log_state'], pl['log_input'] = self._zeros((self.B, 5, sig['cap'])), self._zeros((self.B, 2, sig['cap']))
        return pl['log_state'], pl['log_input']

    def plant(self, sample_time=0.01, max_updates=200, disturbance=None, on=True, time_constant=None, model=None, gravity=9.81):
        """Put a simulated vehicle into every agent's loop, as the reference's `Simulator.run` keeps one with its default options
        `ideal_prediction=False, ideal_update=False` (`vehicles/vehicle.py:73-75`).  From now on, after every solve (`solve_cold`,
        `step`, every step inside a `rollout` launch) the vehicle travels the update under the plan's inputs plus `disturbance`
        (`Vehicle.simulate`: the exact integral of the linearly interpolated applied input; n_samp = update_time / sample_time samples),
        and the next solve starts from the state the vehicle had ONE UPDATE AGO integrated under the undisturbed inputs
        (`Vehicle.predict`): a disturbance enters the loop one update late, as in the reference.  disturbance: array / tensor
        [B, n_spl, max_updates, n_samp + 1] added to the inputs (`input_disturbance` draws the reference's), None: none; an update beyond
        `max_updates` is not simulated and sets the plant's `overflow`.  `arrived` / `stop_at_arrival` test the travelled state and the
        last applied input; with `record_signals` the log takes the travelled state and the applied input (dinput: the plan's).  Call
        before `solve_cold`: the vehicle starts from the first plan's own sample 0.  Integrator classes (`ode` = input: Holonomic,
        Holonomic3D).

        time_constant (a scalar, or one value per agent [B]; None: none): the reference's first-order actuator lag, the vehicle
        options `{'1storder_delay': True, 'time_constant': ...}` (`vehicles/vehicle.py:378-381, 429-431`).  The vehicle then applies
        not the commanded input a (plan + disturbance) but v with v' = (a - v) / time_constant, started from the last applied input,
        and travels under v -- in closed form on the sample grid, exact for the linearly interpolated command (include/omgx.h
        OMGX_HAS_PLANT_LAG has the statements; the reference integrates with odeint).  The prediction knows no lag, as the
        reference's: a systematic model mismatch, per agent, for a robustness study of a fleet in one `rollout` launch.  `arrived` /
        `stop_at_arrival` and the log see the lagged input.  The batch reads no vehicle option on its own: a vehicle with
        '1storder_delay' set is refused unless its `time_constant` is passed here.  on=False takes the plant out again, the lag
        with it.

        model='quadrotor', gravity=...: the Quadrotor's own model (`vehicles/quadrotor.py:149-152`: state (x, y, dx, dy, theta), inputs
        thrust and pitch rate as the plan holds them) -- the vehicle travels by classical Runge-Kutta under the linearly interpolated
        applied inputs, the next solve starts from the position of `state_prev` integrated under the nominal ones, `arrived` /
        `stop_at_arrival` test the travelled position and the plan's velocity at the last travelled sample (`quadrotor.py:104-110`),
        and `signals()` gains `state` [B, 5, cap] and `input` [B, 2, cap] (include/omgx.h OMGX_HAS_PLANT_QUADROTOR has the statements).
        disturbance: [B, 2, max_updates, n_samp + 1].  The batch reads no vehicle option on its own -- a batch from a problem bundle
        knows neither `ode` nor `g` --, so the model is named here; without `model` a Quadrotor batch is refused as before.  Per step
        only (`rollout` is refused), no `time_constant`."""
        if not on:
            if self._pl is not None:
                quad = self._pl.get('model') == 'quadrotor'
                self._pl = None
                self._plant_lag(None)
                self._plant_rollout()
                if self.under_way is not None:
                    self._stop_rule(None if quad else self._o_pose('stop_at_arrival'))      # (the Quadrotor has no rule without its plant)
                if self._sig is not None:
                    self._signals_fused(True)
            return
        if self._ft is not None:
            raise NotImplementedError(FREE_T_REFUSAL % 'plant')
        if model is not None:
            self._quad_model('plant', model)
            return self._plant_quadrotor(sample_time, max_updates, disturbance, time_constant, gravity)
        lay, label = self.tpl.par_layout, self.veh.label
        cls_name = type(self.veh).__name__ if hasattr(self.veh, 'ode') else label
        if any((label, nm) not in lay for nm in ('state0', 'input0', 'poseT')) or self.n_spl != self.n_dim:
            raise NotImplementedError('plant(): %s is not an integrator class (ode = input: Holonomic, Holonomic3D, parameters state0 / '
                                      "input0 / poseT); its own model is not simulated in the batched loop unless it is named: pass "
                                      "model='quadrotor' for the Quadrotor's" % cls_name)
        if getattr(self.veh, 'options', {}).get('1storder_delay') and time_constant is None:
            raise NotImplementedError("plant(): %s has '1storder_delay' set and the batched loop reads no vehicle option on its own; pass "
                                      "time_constant=vehicle.options['time_constant'] to simulate the first-order actuator lag" % cls_name)
        if self._plan_ready:
            raise RuntimeError('plant(): the vehicle starts from the first plan -- call it before solve_cold')
        n_samp = int(round(self.update_time / float(sample_time), 6))
        if n_samp < 1 or int(max_updates) < 1:
            raise ValueError('plant: sample_time must not exceed update_time and max_updates must be positive')
        if self._sig is not None and self._sig['sample_time'] != float(sample_time):
            raise ValueError('plant: the log is kept with sample_time %g' % self._sig['sample_time'])
        if self._fb is not None and self._fb['sample_time'] != float(sample_time):
            raise ValueError('plant: measured states are integrated with sample_time %g (feedback)' % self._fb['sample_time'])
        shape = (self.B, self.n_spl, int(max_updates), n_samp + 1)
        if disturbance is not None and tuple(disturbance.shape) != shape:
            raise ValueError('plant: disturbance must be [B, n_spl, max_updates, n_samp + 1] = %s, got %s' % (shape, tuple(disturbance.shape)))
        lag = None
        if time_constant is not None:
            tc = np.asarray(time_constant, dtype=float)
            if tc.shape not in ((), (self.B,)):
                raise ValueError('plant: time_constant must be a scalar or one value per agent [%d], got %s' % (self.B, list(tc.shape)))
            tc = np.ascontiguousarray(np.broadcast_to(tc, (self.B,)))
            if not (np.isfinite(tc).all() and (tc > 0.0).all()):
                raise ValueError('plant: time_constant must be positive and finite')
            # (formed once, element by element with one exp: every executor, and every sub-batch of a streamed loop, gets the same bits)
            decay = np.array([math.exp(-float(sample_time) / t) for t in tc])
            if not (decay < 1.0).all():
                raise ValueError('plant: time_constant = %g is too long for sample_time %g (exp(-sample_time / time_constant) rounds to 1)'
                                 % (tc[decay >= 1.0][0], float(sample_time)))
            lag = (tc, decay)
        pl = dict(sample_time=float(sample_time), n_samp=n_samp, max_updates=int(max_updates), o_pose=self._o_pose('plant'), lag=lag)
        pl.update(self._plant_alloc(disturbance))
        self._plant_lag(pl)                                 # (may still refuse: the loop is as it was then)
        self._pl = pl
        if self._sig is not None:
            self._signals_fused(False)
        if self.under_way is not None:
            self._stop_rule(pl['o_pose'])                   # (the rule moves from the predicted to the travelled state)

    def plant_state(self):
        """dict `state`, `state_prev`, `input_last` [B, n_spl] (where every vehicle is at its last simulated sample, where it was one
        update earlier, the last applied input), `n_upd` [B] (updates simulated), `overflow` [B] (1: an update beyond `max_updates` was
        asked for).  Device tensors on the device loop, arrays on the host loop.  With `plant(model='quadrotor')`: state / state_prev
        [B, 5], input_last [B, 2], and `dspl_last` [B, 2], the plan's velocity at the last travelled sample."""
        if self._pl is None:
            raise RuntimeError('plant_state(): call plant() first')
        names = ('state', 'state_prev', 'input_last', 'n_upd', 'overflow') + (('dspl_last',) if self._pl.get('model') == 'quadrotor' else ())
        return dict((nm, self._pl[nm]) for nm in names)

    # -- states measured outside the loop ------------------------------------------------------------
    def feedback(self, sample_time=0.01, on=True, model=None, gravity=9.81):
        """Let `step` take measured states (`step(states=...)`): the reference's deployment contract, `Deployer.update(current_time,
        states, inputs, ..., enforce_states, enforce_inputs)` -> `Vehicle.predict(state0=...)` (`execution/deployer.py:43-79`,
        `vehicles/vehicle.py:302-337`).  Fixes the sample grid the measured state is integrated on, n_samp = update_time /
        sample_time intervals per update (the trapezoid sum of the plan's inputs: exact for the reference's linearly interpolated
        input).  Integrator classes (`ode` = input: Holonomic, Holonomic3D); a vehicle's '1storder_delay' option changes nothing here
        (`Vehicle.predict(state0=...)` has no lag in it, and the measured vehicle is outside the loop); every agent on the
        batch's one clock (no `delay`).  `rollout` takes no states.  on=False: `step` takes none again.
        model='quadrotor', gravity=...: the Quadrotor's own model (as `plant(model='quadrotor')`): `step(states=...)` takes [B, 5]
        states (x, y, dx, dy, theta), integrates them by the Runge-Kutta statements of the plant's prediction and writes the position
        into spl0, the plan's derivatives into dspl0 / ddspl0; `enforce` is `Quadrotor.set_initial_conditions` (the position, at
        rest); `inputs` are refused, the reference ignores them."""
        if not on:
            self._fb = None
            return
        if self._ft is not None:
            raise NotImplementedError(FREE_T_REFUSAL % 'feedback')
        lay, label = self.tpl.par_layout, self.veh.label
        cls_name = type(self.veh).__name__ if hasattr(self.veh, 'ode') else label
        if model is not None:
            self._quad_model('feedback', model)
            if not float(gravity) > 0.0:
                raise ValueError('feedback: gravity must be positive')
        elif any((label, nm) not in lay for nm in ('state0', 'input0', 'poseT')) or self.n_spl != self.n_dim:
            raise NotImplementedError('feedback(): %s is not an integrator class (ode = input: Holonomic, Holonomic3D, parameters state0 / '
                                      "input0 / poseT); its own model is not integrated in the batched loop unless it is named: pass "
                                      "model='quadrotor' for the Quadrotor's" % cls_name)
        if getattr(self, 'pool', None) is not None:
            raise NotImplementedError('feedback: not with a host pool (its workers run the step glue themselves)')
        n_samp = int(round(self.update_time / float(sample_time), 6))
        if n_samp < 1:
            raise ValueError('feedback: sample_time must not exceed update_time')
        if model is not None and n_samp + 1 > 64:
            raise ValueError("feedback: model='quadrotor' takes at most 63 samples per update, got %d" % n_samp)
        for what, g in (('log', self._sig), ('plant', self._pl)):
            if g is not None and g['sample_time'] != float(sample_time):
                raise ValueError('feedback: the %s is kept with sample_time %g' % (what, g['sample_time']))
        self._fb = dict(sample_time=float(sample_time), n_samp=n_samp)
        if model is not None:
            self._fb.update(model='quadrotor', g=float(gravity))

    def signals(self):
        """The log of `record_signals`: dict with `count` [B] (columns written per agent), `time` [cap] (the time of the first logged
        plan + c * sample_time), `splines` [B, n_der, n_spl, cap] (time-derivative order o of spline k in column c) and `overflow` [B]
        (1: an append did not fit and was dropped); for the point-mass classes (state0 / input0 parameters) also `state`, `input`,
        `dinput` [B, n_spl, cap] as views of `splines`.  Device tensors on the device loop (the caller's stream is ordered behind the
        launches that wrote them), arrays on the host loop.  The columns of agent b at or beyond `count[b]` are NOT DEFINED: the
        vehicles arrive at different updates, every agent's signals are its first `count[b]` columns."""
        g = self._sig
        if g is None:
            raise RuntimeError('signals(): call record_signals() first')
        tax = g['t_start'] + np.arange(g['cap']) * g['sample_time']
        out = dict(count=g['count'], time=tax, splines=g['log'], overflow=g['overflow'])
        if (self.veh.label, 'state0') in self.tpl.par_layout:
            for o, nm in enumerate(('state', 'input', 'dinput')[:g['n_der']]):
                out[nm] = g['log'][:, o]
        if self._pl is not None and self._pl.get('model') == 'quadrotor':
            # (the Quadrotor's travelled state [B, 5, cap] and applied input [B, 2, cap], at the columns of `splines`)
            out['state'], out['input'] = self._plant_log()
        return out

    def summary(self):
        """[B, 8] per agent, what `problem.final()` would report from its signals: columns, motion time (columns - 1) * sample_time,
        path length, largest |input|, largest |dinput|, |state_last - poseT|, |input_last|, 0 (reserved); Euclidean norms.  Device
        loop: `omgx_batch_signals_reduce` (one launch, fixed summation order); host loop: the same in numpy."""
        if self._sig is None:
            raise RuntimeError('summary(): call record_signals() first')
        o_pose = self._o_pose('summary', point_mass=False)
        return self._signals_summary(self.p[:, o_pose:o_pose + self.n_spl])

    def host(self, name):
        a = getattr(self, name)
        return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


class DeviceP2P(BatchP2P):
    """The device executor (`ops='hip'`): [B, *] torch tensors as plain attributes, every hook a launch of the library on them."""
    kind = 'hip'

    def _allocate(self, P, ops, device):
        import torch
        from .backend import BatchSolver
        self.torch = torch
        self.dev = device if device is not None else torch.device('cuda', 0)
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.solver = BatchSolver(self.tpl, self.B, device=self.dev.index or 0, options=self.opts)
        self.solver.set_stream(torch.cuda.current_stream().cuda_stream)
        # the plan as every glue entry of the library takes it (include/omgx.h, above omgx_store_spec): built once
        self._plan = dict(coeff_off=self.o_spl, n_spl=self.n_spl, degree=self.basis.degree, knots=self.basis.knots,
                          inv_T=1.0 / self.T if self.T else 1.0)      # (free end time: every agent's own, read from x)
        self.p = torch.as_tensor(np.ascontiguousarray(P['p']), **f64)
        self.x = torch.as_tensor(np.ascontiguousarray(P['x0']), **f64)
        self.x_new = torch.empty_like(self.x)
        self.lam = torch.zeros((self.B, self.tpl.n_con), **f64)
        self.lb, self.ub = torch.as_tensor(self.tpl.lb, **f64), torch.as_tensor(self.tpl.ub, **f64)
        self.status = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self.iters = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self._perm_idx = torch.as_tensor(np.maximum(self.perm, 0), dtype=torch.int64, device=self.dev)
        self._perm_ok = torch.as_tensor((self.perm >= 0).astype(np.float64), **f64)
        self._mask = torch.ones(self.B, dtype=torch.uint8, device=self.dev)
        self._order = torch.arange(self.B, dtype=torch.int32, device=self.dev)

    def _predict(self, tau, t_rel):
        # (the order is asked for before the prediction: its launch then carries the ordering as one more workgroup)
        if self.straggler_first:
            self.solver.order_by_iters(self.iters, self._order)
        # one kernel: the initial conditions from the plan at tau and the new t, all written into p
        self.solver.predict_ex(self.x, self.p, tau=tau, p_off=self.p_offs, p_t=self.o_t, t_value=t_rel, **self._plan)

    def _shift(self):
        if self._pl is not None and self.under_way is not None:
            # (with the plant an agent's loop ends ahead of the glue of the step: a stopped agent keeps plan and multipliers as they are)
            go = self.under_way != 0
            self.solver.shift(self.x, go.to(self.torch.uint8), self.shift_entries, self.shift_mats, device=True)
            self.lam = self.torch.where(go[:, None], self.lam.index_select(1, self._perm_idx) * self._perm_ok, self.lam)
            return
        self.solver.shift(self.x, self._mask, self.shift_entries, self.shift_mats, device=True)
        self.lam = self.lam.index_select(1, self._perm_idx) * self._perm_ok

    def _solve(self, warm, events=None, ordered=False, extra=None):
        self.solver.set_options(warm_start=int(warm), max_iter=self.max_iter_step if warm else self.max_iter_cold,
                                **dict(self._base_extra, **(extra or {})))
        if not warm:
            self.lam.zero_()
            self._x_init = self.x.clone()
        if warm and self.straggler_first and not ordered:
            # agents that needed most iterations last time are launched first
            self.solver.order_by_iters(self.iters, self._order)
        if events is not None:                 # timing events of the caller (bench.py): on the solve kernel's own dispatch
            self.solver.set_launch_events(events[0], events[1])
        self.solver.solve_device(self.p, self.x, self.lb, self.ub, self.x_new, self.lam, self.status, self.iters, bounds_shared=True)
        self.x, self.x_new = self.x_new, self.x

    def _cold(self, bends, fused):
        if not bends or not fused:
            self._solve(False)
            return self.restart_failed(bends)
        t = self.torch
        alts = t.stack([self._bent(self.x, s) for s in bends]).contiguous()
        attempts = t.zeros(self.B, dtype=t.int32, device=self.dev)
        self.solver.set_restarts(alts, attempts)
        try:
            self._solve(False)
        finally:
            self.solver.set_restarts(None)
        return int(attempts.max().item())

    def _bent(self, x_first, s):
        """The initial guess x_first with its spline coefficients moved sideways (perpendicular to start -> goal in
        the x-y plane) by s * sin^2(pi * k / (L - 1)) metres."""
        t = self.torch
        L, ns = self.L, self.n_spl
        c = x_first[:, self.o_spl:self.o_spl + ns * L].reshape(self.B, ns, L)
        d = c[:, :, -1] - c[:, :, 0]
        d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
        nrm = t.zeros_like(d)
        nrm[:, 0], nrm[:, 1] = -d[:, 1], d[:, 0]
        nrm = nrm / nrm.norm(dim=1, keepdim=True).clamp_min(1e-12)
        bump = t.sin(t.linspace(0., 1., L, dtype=t.float64, device=self.dev) * np.pi) ** 2
        alt = x_first.clone()
        alt[:, self.o_spl:self.o_spl + ns * L] += (float(s) * nrm[:, :, None] * bump[None, None, :]).reshape(self.B, -1)
        return alt

    def restart_failed(self, bends=(1.0, -1.0, 2.5, -2.5)):
        passes = 0
        for s in bends or ():
            if bool((self.status == 0).all()):
                break
            alt = self._bent(self._x_init, s)      # (_x_init: the guess the first pass started from)
            # the solved agents sit in self.x (the output of the last pass): they are skipped and keep it
            self.solver.set_options(warm_start=0, max_iter=self.max_iter_cold)
            self.solver.solve_device(self.p, alt, self.lb, self.ub, self.x, self.lam, self.status, self.iters, bounds_shared=True, only_failed=True)
            passes += 1
        return passes

    def _script_alloc(self, time, what, value):
        t = self.torch
        return dict(time=t.as_tensor(time, dtype=t.float64).to(self.dev), what=t.as_tensor(what, dtype=t.int32).to(self.dev),
                    value=t.as_tensor(value, dtype=t.float64).to(self.dev), what_host=what)

    def _script_args(self):
        return dict(self._sc, obstacles=self.obst)

    def _script_advance(self, t_prev, t_now):
        """One launch in place of the tensor statements (the library forms t_now = t_prev + update_time as `step_clock` does)."""
        self.solver.obstacles_advance(self.p, self._script_args(), t_prev, self.update_time)

    def _rollout(self, tau, t_rel, crossed, iters_log, status_log, t_abs=None):
        self._plant_rollout()
        # (the script with the absolute times of this step list, registered with the handle; taken off without one)
        if self._sc is not None or getattr(self, '_sc_registered', False):
            self.solver.set_obstacle_script(None if self._sc is None else self._script_args(), t_abs)
            self._sc_registered = self._sc is not None
        self.solver.set_options(warm_start=1, max_iter=self.max_iter_step, **self._base_extra)
        if self.straggler_first:
            self.solver.order_by_iters(self.iters, self._order)
        self.solver.rollout(self.p, self.x, self.lb, self.ub, self.lam, self.status, self.iters, tau, t_rel, crossed,
                            p_off=self.p_offs, p_t=self.o_t, obstacles=self.obst, dt=self.update_time, shift_entries=self.shift_entries, shift_T=self.shift_mats,
                            lam_perm=self.perm, cross_options=self.cross_options or None, iters_log=iters_log, status_log=status_log,
                            **self._plan)

    # -- missions: registered with the handle, flown by the rollout kernel's mission instances --------------------------------------
    def _mission_alloc(self, goals, n_goals, clock0):
        t = self.torch
        i32 = dict(dtype=t.int32, device=self.dev)
        return dict(goals=t.as_tensor(goals, dtype=t.float64).to(self.dev).contiguous(), n_goals=t.as_tensor(n_goals, dtype=t.int32).to(self.dev),
                    leg=t.zeros(self.B, **i32), clock=t.full((self.B,), clock0, **i32), arrivals=t.full((self.B, 1 + goals.shape[1]), -1, **i32))

    def _mission_set(self, n_steps):
        ms = self._ms
        spec = dict((nm, ms[nm]) for nm in ('goals', 'n_goals', 'leg', 'clock', 'arrivals', 'x_reset'))
        spec.update(o_state0=self.o_state0, o_input0=self.o_input0, o_poseT=ms['o_pose'], p_t=self.o_t, coeff_off=self.o_spl, n_spl=self.n_spl, L=self.L)
        # (a leg's first solve: what `solve_cold` sets)
        self.solver.set_mission(spec, n_steps=n_steps, step_index=ms['steps'], cold_options=dict(self._base_extra, max_iter=self.max_iter_cold))

    def _mission_off(self):
        self.solver.set_mission(None)

    def _mission_clock_max(self):
        return int(self._ms['clock'].max().item())

    def _mission_run(self, table, n_steps, iters_log, status_log):
        self._mission_set(n_steps)
        self._rollout(*([r[k] for r in table] for k in range(3)), iters_log=iters_log, status_log=status_log)

    def _mission_advance(self, step_index):
        self._plant_rollout()                               # (the plant as registered with the handle: its rule, its travelled state)
        self._mission_set(1)
        self.solver.mission_advance(self.p, self.x, self.lam, step_index)

    def _norm(self, a):
        return a.norm(dim=1)

    def _stop_rule(self, o_pose):
        """The rule is the solve kernel's: registered with the handle (o_pose None: taken off)."""
        self.under_way = None if o_pose is None else self.torch.ones(self.B, dtype=self.torch.int32, device=self.dev)
        # (with the plant in the loop the criterion is the plant's, on the travelled state: the solve kernel gets a rule that never
        # holds -- a negative tolerance -- and only honours the flags)
        where = () if o_pose is None else (self.o_state0, self.o_input0, o_pose, self.n_dim, self.stop_tol if self._pl is None else -1.0)
        self.solver.set_stop(*where, under_way=self.under_way)

    def _signals_alloc(self, shape):
        t = self.torch
        return (t.zeros(shape, dtype=t.float64, device=self.dev), t.zeros(self.B, dtype=t.int32, device=self.dev),
                t.zeros(self.B, dtype=t.int32, device=self.dev))

    def _signals_args(self):
        g = self._sig
        return dict(self._plan, n_samp=g['n_samp'], p_t=self.o_t, sample_time=g['sample_time'])

    def _signals_fused(self, on):
        """The append inside the solve / rollout kernel, on or off."""
        if not on:
            return self.solver.set_signals(None)
        g = self._sig
        self.solver.set_signals(g['log'], g['count'], g['overflow'], **self._signals_args())

    def _free_t_set(self):
        """The free-end-time tables, registered with the handle once (include/omgx.h omgx_batch_set_free_t)."""
        self.solver.set_free_t(self._ft)

    def _free_t_advance(self):
        self.solver.free_t_advance(self.x, self.p, self.update_time, under_way=self.under_way)

    def _signals_append_now(self):
        """One append of the current plan (x at the time p[:, t]) outside a solve: the stand-alone kernel."""
        g = self._sig
        if self._ft is not None:                            # (every agent on its own horizon: omgx_batch_free_t_append)
            a = self._signals_args()
            return self.solver.free_t_append(self.x, g['log'], g['count'], g['overflow'], under_way=self.under_way,
                                             **dict((k, a[k]) for k in ('coeff_off', 'n_spl', 'degree', 'knots', 'n_samp', 'sample_time')))
        self.solver.signals_append(self.x, self.p, g['log'], g['count'], g['overflow'], under_way=self.under_way, **self._signals_args())

    def _zeros(self, shape):
        return self.torch.zeros(shape, dtype=self.torch.float64, device=self.dev)

    def _plant_alloc(self, disturbance, model=None):
        t = self.torch
        f64 = dict(dtype=t.float64, device=self.dev)
        widths = dict(state=5, state_prev=5, input_last=2, dspl_last=2) if model == 'quadrotor' else \
            dict((nm, self.n_spl) for nm in ('state', 'state_prev', 'input_last'))
        out = dict((nm, t.zeros((self.B, w), **f64)) for nm, w in widths.items())
        out.update((nm, t.zeros(self.B, dtype=t.int32, device=self.dev)) for nm in ('n_upd', 'overflow'))
        out['dist'] = None if disturbance is None else t.as_tensor(disturbance, **f64).contiguous()
        return out

    def _quad_args(self, g, plant=True, log=False):
        """The keyword arguments of `BatchSolver._quad_plant_spec`: g = the plant (`self._pl`) or the feedback grid (`self._fb`)."""
        kw = dict(self._plan, n_samp=g['n_samp'], sample_time=g['sample_time'], p_off=self.p_offs, p_t=self.o_t, g=g['g'])
        if plant:
            kw.update(dict((nm, g[nm]) for nm in ('state', 'state_prev', 'input_last', 'dspl_last', 'n_upd', 'overflow', 'dist')),
                      under_way=self.under_way, max_updates=g['max_updates'], p_poseT=g['o_pose'], stop_tol=self.stop_tol)
        if log:
            kw['log_state'], kw['log_input'] = self._plant_log()
        return kw

    def _plant_args(self):
        g = self._pl
        return dict(self._plan, state=g['state'], state_prev=g['state_prev'], input_last=g['input_last'], n_upd=g['n_upd'], overflow=g['overflow'],
                    dist=g['dist'], under_way=self.under_way, n_samp=g['n_samp'], max_updates=g['max_updates'], p_t=self.o_t,
                    p_state0=self.o_state0, p_input0=self.o_input0, p_poseT=g['o_pose'], sample_time=g['sample_time'], stop_tol=self.stop_tol)

    def _plant_log_args(self):
        g = self._sig
        return None if g is None else dict(log=g['log'], count=g['count'], overflow=g['overflow'], **self._signals_args())

    def _plant_predict(self, tau, t_rel):
        # (as `_predict`: the launch carries the ordering of the next solve as one more workgroup)
        if self.straggler_first:
            self.solver.order_by_iters(self.iters, self._order)
        if self._pl.get('model') == 'quadrotor':
            return self.solver.plant_quadrotor_predict(self.x, self.p, tau, t_rel, self._quad_args(self._pl))
        self.solver.plant_predict(self.x, self.p, tau, t_rel, self._plant_args())

    def _feedback_predict(self, tau, t_rel, states, inputs, fresh, enforce):
        """One launch: the initial conditions from the measured states (device or pinned host tensors; an array is uploaded first),
        the new t, and -- as `_predict` -- the ordering of the next solve as one more workgroup."""
        t = self.torch

        def dev(a, dtype):
            if a is None or t.is_tensor(a):
                return a
            return t.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.dev)
        states, inputs, fresh = dev(states, t.float64), dev(inputs, t.float64), dev(fresh, t.int32)
        if self.straggler_first:
            self.solver.order_by_iters(self.iters, self._order)
        g = self._fb
        if g.get('model') == 'quadrotor':
            return self.solver.plant_quadrotor_predict(self.x, self.p, tau, t_rel, self._quad_args(g, plant=False), states=states, fresh=fresh,
                                                       enforce=enforce)
        self.solver.predict_measured(self.x, self.p, tau, t_rel, states, input=inputs, fresh=fresh, enforce=enforce, n_samp=g['n_samp'],
                                     sample_time=g['sample_time'], p_off=self.p_offs, p_t=self.o_t, **self._plan)

    def _plant_simulate(self):
        if self._pl.get('model') == 'quadrotor':
            return self.solver.plant_quadrotor_simulate(self.x, self.p, self._quad_args(self._pl, log=True), self._plant_log_args())
        self.solver.plant_simulate(self.x, self.p, self._plant_args(), self._plant_log_args())

    def _plant_lag(self, pl):
        """The lag of the plant `pl` (its time constants and decays, host arrays) handed to the handle; None, or a plant without: off."""
        if pl is None or pl['lag'] is None:
            return self.solver.set_plant_lag(None)
        self.solver.set_plant_lag(pl['lag'][0], pl['lag'][1], pl['sample_time'])

    def _plant_rollout(self):
        """The plant (and the log its simulate writes) as the rollout kernel reads it, registered with the handle; taken off without one."""
        if self._pl is None:
            return self.solver.set_plant(None)
        self.solver.set_plant(self._plant_args(), self._plant_log_args())

    def _signals_summary(self, target):
        g, t = self._sig, self.torch
        out = t.zeros((self.B, 8), dtype=t.float64, device=self.dev)
        self.solver.signals_reduce(g['log'], g['count'], target.contiguous(), out, **self._signals_args())
        return out


class HostP2P(BatchP2P):
    """The host executor (`ops=<solver object>`, anything with the `solve(template, p, x0, ...)` signature of the tests' oracle
    port binding): numpy arrays as plain attributes, the glue in numpy statements, the solves by `port`.  Optionally a `pool`
    (attached after construction, bench.py's CPU baseline: `solve(p, x, lam, status, iters, dw, step=...)`) whose workers run glue
    AND solve of a step per agent: `step` then only hands it the clock -- no stop rule, no log."""
    kind = 'host'

    def _allocate(self, P, ops, device):
        self.port = ops                          # injected by tests / bench.py's cpu_baseline leg
        self.n_threads = 1
        self.pool = None
        self.dw = np.zeros(self.B)            # inertia correction carried between warm solves
        self.p, self.x = np.ascontiguousarray(P['p'], dtype=float).copy(), np.ascontiguousarray(P['x0'], dtype=float).copy()
        self.lam = np.zeros((self.B, self.tpl.n_con))
        self.status, self.iters = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        self._log_in_solve = True                # (`_signals_fused`)

    def step(self, events=None, before_solve=None, states=None, inputs=None, fresh=None, enforce=False):
        if self.pool is None:
            return BatchP2P.step(self, events, before_solve, states, inputs, fresh, enforce)
        if states is not None or inputs is not None or fresh is not None or enforce:
            raise NotImplementedError('step(states=...): not with a host pool (its workers run the step glue themselves)')
        if self._ft is not None:
            raise NotImplementedError('step: a free-end-time batch does not run on a host pool (its workers carry the fixed-T step glue)')
        t_now, tau, t_rel, crossed = step_clock(self.time, self.update_time, self.knot_time, self.T)
        self.time = t_now
        self._solve(True, step_desc=self._pool_step(tau, t_rel, crossed), extra=self.cross_options if crossed else None)
        return crossed

    def _pool_step(self, tau, t_rel, crossed):
        """Constants of this step for a pool that runs the glue per agent in its workers (field names of the `StepDesc` the pool defines)."""
        desc = self.pool.step_desc()
        rows = [np.ascontiguousarray(r) for r in self._eval_rows(tau)]
        if len(rows) != 2 or self.n_spl != self.n_dim:
            raise NotImplementedError('the pool step glue carries state0 / input0 only')
        E, Ed = rows
        obst = np.ascontiguousarray(np.array(self.obst, dtype=np.int32).reshape(-1, 4))
        perm = np.ascontiguousarray(self.perm, dtype=np.int64)
        ents = np.ascontiguousarray(self.shift_entries, dtype=np.int32)
        mats = np.ascontiguousarray(self.shift_mats, dtype=np.float64)
        desc._keep = (E, Ed, obst, perm, ents, mats)
        desc.o_spl, desc.n_dim, desc.L = self.o_spl, self.n_dim, self.L
        desc.o_state0, desc.o_input0, desc.o_t = self.o_state0, self.o_input0, self.o_t
        desc.t_rel, desc.dt = t_rel, self.update_time
        desc.E, desc.Ed = E.ctypes.data, Ed.ctypes.data
        desc.n_obst, desc.obst = len(self.obst), obst.ctypes.data
        desc.crossed, desc.n_shift = int(crossed), len(ents)
        desc.shift_entries, desc.shift_mats, desc.perm = ents.ctypes.data, mats.ctypes.data, perm.ctypes.data
        return desc

    def _predict(self, tau, t_rel):
        c = self.x[:, self.o_spl:self.o_spl + self.n_spl * self.L].reshape(self.B, self.n_spl, self.L)
        for o, E in enumerate(self._eval_rows(tau)):
            self.p[:, self.p_offs[o]:self.p_offs[o] + self.n_spl] = c @ E
        self.p[:, self.o_t] = t_rel

    def _shift(self):
        # (with the plant an agent's loop ends ahead of the glue of the step: a stopped agent keeps plan and multipliers as they are)
        go = self.under_way.copy() if self._pl is not None and self.under_way is not None else np.ones(self.B, dtype=bool)
        for (lo, rows, cols, _), Tm in self._shift_dense:
            blk = self.x[:, lo:lo + rows * cols].reshape(self.B, cols, rows)
            self.x[go, lo:lo + rows * cols] = (blk @ Tm.T).reshape(self.B, -1)[go]
        self.lam = np.where(go[:, None], np.where(self.perm >= 0, self.lam[:, np.maximum(self.perm, 0)], 0.0), self.lam)

    def _solve(self, warm, events=None, ordered=False, extra=None, step_desc=None):
        kw = dict(self.opts, warm_start=int(warm), max_iter=self.max_iter_step if warm else self.max_iter_cold, **(extra or {}))
        if self.pool is not None:
            if self.under_way is not None or self._sig is not None:
                raise NotImplementedError('stop_at_arrival / record_signals: not with a host pool (its workers run the step glue themselves)')
            if not warm:
                self.lam[:] = 0.
            self.pool.solve(self.p, self.x, self.lam, self.status, self.iters, self.dw, step=step_desc, **kw)
            return
        if self.under_way is None:
            r = self.port.solve(self.tpl, self.p, self.x, lam_g0=self.lam if warm else None, status0=self.status if warm else None,
                                n_threads=self.n_threads, dw_state=self.dw, **kw)
            self.x, self.lam, self.status, self.iters = r['x'], r['lam_g'], r['status'], r['iters']
        else:
            # the stop rule as the solve kernel applies it: the criterion on p ends an agent's loop for good; the agents
            # under way are solved as a batch of their own (independent problems: the same results), the others keep
            # their plan, their multipliers and their status, iters = 0
            if self._pl is None:                 # (with the plant in the loop `_plant_predict` has tested the travelled state)
                self.under_way &= ~self.arrived(self.stop_tol)
            idx = np.flatnonzero(self.under_way)
            self.iters = np.zeros(self.B, dtype=np.int32)
            if len(idx):
                dw = self.dw[idx].copy()
                r = self.port.solve(self.tpl, self.p[idx], self.x[idx], lam_g0=self.lam[idx] if warm else None,
                                    status0=self.status[idx] if warm else None, n_threads=self.n_threads, dw_state=dw, **kw)
                self.x[idx], self.lam[idx], self.status[idx], self.iters[idx], self.dw[idx] = r['x'], r['lam_g'], r['status'], r['iters'], dw
        if self._log_in_solve:
            self._signals_append_host(self.under_way)

    def _cold(self, bends, fused):
        self._solve(False)
        return 0

    def _norm(self, a):
        return np.linalg.norm(a, axis=1)

    def _stop_rule(self, o_pose):
        """The rule is `_solve`'s: it tests `arrived` and solves the agents under way (o_pose None: taken off)."""
        self.under_way = None if o_pose is None else np.ones(self.B, dtype=bool)

    def _signals_alloc(self, shape):
        if self.pool is not None:
            raise NotImplementedError('record_signals: not with a host pool (its workers run the step glue themselves)')
        return np.zeros(shape), np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)

    def _signals_fused(self, on):
        """The append at the end of `_solve`, on or off."""
        self._log_in_solve = bool(on)

    def _free_t_set(self):
        self._log_in_solve = False               # (the append is a step of its own behind every solve: `_step_free_t`)

    def _free_t_advance(self):
        free_t_advance_numpy(self.x, self.p, self.under_way, self.update_time, self._ft)

    def _signals_append_now(self):
        if self._ft is not None:
            g = self._sig
            return free_t_append_numpy(self.x, self.under_way, g['log'], g['count'], g['overflow'], self._ft, g['n_samp'], g['sample_time'])
        self._signals_append_host(self.under_way)

    def _signals_append_host(self, under_way):
        """`omgx_batch_signals_append` in numpy: the same semantics, `Basis.eval_basis` / `derivative` as `_eval_rows`."""
        g = self._sig
        if g is None:
            return
        for b in range(self.B):
            if under_way is None or under_way[b]:
                self._signals_append_agent(b)

    def _signals_append_agent(self, b):
        """One append for agent b; returns the column of its sample 0 (written or not), None when the append did not fit."""
        g = self._sig
        L, ns, n_samp, cap, st = self.L, self.n_spl, g['n_samp'], g['cap'], g['sample_time']
        inv_T = 1.0 / self.T
        bases = [(self.basis, None)] + [self.basis.derivative(o) for o in range(1, g['n_der'])]
        cnt = int(g['count'][b])
        first = 0 if cnt == 0 else 1
        n_col = n_samp + 1 - first
        if cnt + n_col > cap:
            g['overflow'][b] = 1
            return None
        t_rel = float(self.p[b, self.o_t])
        u = (t_rel + np.arange(first, n_samp + 1) * st) * inv_T
        c = self.x[b, self.o_spl:self.o_spl + ns * L].reshape(ns, L)
        for o, (dbasis, Po) in enumerate(bases):
            E = dbasis.eval_basis(u) if o == 0 else dbasis.eval_basis(u) @ Po * inv_T ** o
            g['log'][b, o, :, cnt:cnt + n_col] = c @ E.T
        g['count'][b] = cnt + n_col
        return cnt - first

    # -- the plant: `omgx_batch_plant_simulate / _predict` in numpy, the same statements in the same summation order ---------------
    def _zeros(self, shape):
        return np.zeros(shape)

    def _plant_alloc(self, disturbance, model=None):
        if self.pool is not None:
            raise NotImplementedError('plant: not with a host pool (its workers run the step glue themselves)')
        widths = dict(state=5, state_prev=5, input_last=2, dspl_last=2) if model == 'quadrotor' else \
            dict((nm, self.n_spl) for nm in ('state', 'state_prev', 'input_last'))
        out = dict((nm, np.zeros((self.B, w))) for nm, w in widths.items())
        out.update((nm, np.zeros(self.B, dtype=np.int32)) for nm in ('n_upd', 'overflow'))
        out['dist'] = None if disturbance is None else np.ascontiguousarray(disturbance, dtype=float).copy()
        return out

    def _plant_plan(self, b, g=None):
        """(c, t_rel, u): the plan of agent b [n_spl, L], the time it was solved at, and its inputs (time derivative) at the samples
        0 .. n_samp of the update [n_spl, n_samp + 1].  g: whose sample grid (the plant's; `_feedback_predict` passes its own)."""
        g = self._pl if g is None else g
        inv_T = 1.0 / self.T
        c = self.x[b, self.o_spl:self.o_spl + self.n_spl * self.L].reshape(self.n_spl, self.L)
        t_rel = float(self.p[b, self.o_t])
        dbasis, P1 = self.basis.derivative(1)
        tau = (t_rel + np.arange(g['n_samp'] + 1) * g['sample_time']) * inv_T
        return c, t_rel, c @ (dbasis.eval_basis(tau) @ P1 * inv_T).T

    # -- the Quadrotor's plant: `omgx_batch_plant_quadrotor_simulate / _predict` in numpy (include/omgx.h OMGX_HAS_PLANT_QUADROTOR) -----
    def _quad_plan(self, b, g):
        """(c, t_rel, u, s0, d1): the plan of agent b [2, L], the time it was solved at, its inputs (u1, u2) at the samples 0 .. n_samp of
        the update [2, n_samp + 1], its own state at sample 0 [5] and its velocity at the samples [2, n_samp + 1].  g: whose sample grid
        and gravity (the plant's or the feedback's)."""
        inv_T = 1.0 / self.T
        c = self.x[b, self.o_spl:self.o_spl + 2 * self.L].reshape(2, self.L)
        t_rel = float(self.p[b, self.o_t])
        tau = (t_rel + np.arange(g['n_samp'] + 1) * g['sample_time']) * inv_T
        der = [c @ self.basis.eval_basis(tau).T]
        for o in (1, 2, 3):
            dbasis, Po = self.basis.derivative(o)
            der.append(c @ (dbasis.eval_basis(tau) @ Po).T)
        s2 = inv_T * inv_T
        s3 = s2 * inv_T
        d1, dd, ddd = der[1] * inv_T, der[2] * s2, der[3] * s3
        u = quad_inputs_numpy(dd, ddd, g['g'])
        s0 = np.array([der[0][0, 0], der[0][1, 0], d1[0, 0], d1[1, 0], np.arctan2(dd[0, 0], dd[1, 0] + g['g'])])
        return c, t_rel, u, s0, d1

    def _quad_simulate(self):
        g, sig = self._pl, self._sig
        log_state, log_input = self._plant_log()
        for b in range(self.B):
            if self.under_way is not None and not self.under_way[b]:
                continue
            nu = int(g['n_upd'][b])
            if nu >= g['max_updates']:
                g['overflow'][b] = 1
                continue
            c, t_rel, u, s0, d1 = self._quad_plan(b, g)
            a = u + g['dist'][b, :, nu, :] if g['dist'] is not None else u
            start = s0 if nu == 0 else g['state'][b].copy()
            samples = quad_rk4_numpy(start, a, g['sample_time'], g['g'])
            if sig is not None:
                first = 0 if int(sig['count'][b]) == 0 else 1
                col = self._signals_append_agent(b)             # (the plan's own columns: the reference's `dspl` / `ddspl` signals)
                if col is not None:
                    log_state[b, :, col + 1:col + 1 + g['n_samp']] = samples[:, 1:]
                    log_input[b, :, col + 1:col + 1 + g['n_samp']] = a[:, 1:]
                    if first == 0:                              # (column 0: the plan's sample 0, undisturbed)
                        log_state[b, :, col], log_input[b, :, col] = s0, u[:, 0]
            g['state_prev'][b], g['state'][b], g['input_last'][b], g['dspl_last'][b] = start, samples[:, -1], a[:, -1], d1[:, -1]
            g['n_upd'][b] = nu + 1

    def _quad_predict(self, tau, t_rel):
        g = self._pl
        if self.under_way is not None:
            self.under_way &= ~(self.arrived(self.stop_tol) & (g['n_upd'] >= 1))
        rows = self._eval_rows(tau)
        for b in range(self.B):
            if self.under_way is not None and not self.under_way[b]:
                continue
            c, _, u, s0, _ = self._quad_plan(b, g)
            start = g['state_prev'][b] if g['n_upd'][b] >= 1 else s0
            self._quad_write(b, c, rows, quad_rk4_numpy(start, u, g['sample_time'], g['g'])[:2, -1], t_rel)

    def _quad_write(self, b, c, rows, pos, t_rel):
        """spl0 <- pos, dspl0 / ddspl0 <- the plan's derivatives (rows: `_eval_rows(tau)`), t <- t_rel."""
        self.p[b, self.p_offs[0]:self.p_offs[0] + 2] = pos
        for o in (1, 2):
            self.p[b, self.p_offs[o]:self.p_offs[o] + 2] = c @ rows[o]
        self.p[b, self.o_t] = t_rel

    def _quad_feedback_predict(self, tau, t_rel, states, fresh, enforce):
        g = self._fb
        states = np.asarray(states, dtype=float)
        go = np.ones(self.B, dtype=bool) if fresh is None else np.asarray(fresh) != 0
        new = {}
        if not enforce:                                   # (ahead of `_predict`: `_quad_plan` reads the time the plan was solved at)
            for b in np.flatnonzero(go):
                u = self._quad_plan(b, g)[2]
                new[b] = quad_rk4_numpy(states[b], u, g['sample_time'], g['g'])[:2, -1]
        self._predict(tau, t_rel)                         # (an agent without a fresh measurement; dspl0 / ddspl0 / t of every agent)
        if enforce:
            self.p[go, self.p_offs[0]:self.p_offs[0] + 2] = states[go, :2]
            for o in (1, 2):
                self.p[go, self.p_offs[o]:self.p_offs[o] + 2] = 0.0
        for b, pos in new.items():
            self.p[b, self.p_offs[0]:self.p_offs[0] + 2] = pos

    def _plant_simulate(self):
        if self._pl.get('model') == 'quadrotor':
            return self._quad_simulate()
        g, sig = self._pl, self._sig
        for b in range(self.B):
            if self.under_way is not None and not self.under_way[b]:
                continue
            nu = int(g['n_upd'][b])
            if nu >= g['max_updates']:
                g['overflow'][b] = 1
                continue
            c, t_rel, u = self._plant_plan(b)
            a = u + g['dist'][b, :, nu, :] if g['dist'] is not None else u
            if g['lag'] is not None:
                # the first-order actuator lag (include/omgx.h OMGX_HAS_PLANT_LAG): the same statements in the same order, sample by sample
                tc, E, h = g['lag'][0][b], g['lag'][1][b], g['sample_time']
                v = np.empty_like(a)
                v[:, 0] = u[:, 0] if nu == 0 else g['input_last'][b]
                for i in range(g['n_samp']):
                    s = (a[:, i + 1] - a[:, i]) / h
                    r = tc * s
                    v[:, i + 1] = (a[:, i + 1] - r) + ((v[:, i] - a[:, i]) + r) * E
                a = v                                           # (the vehicle travels under the lagged input; the log takes it)
            s0 = c @ self.basis.eval_basis([t_rel / self.T])[0] if nu == 0 else g['state'][b].copy()
            samples = s0[:, None] + g['sample_time'] * np.cumsum((a[:, :-1] + a[:, 1:]) / 2.0, axis=1)
            if sig is not None:
                col = self._signals_append_agent(b)             # (the plan's own columns: column 0 and the dinput row stay)
                if col is not None:
                    sig['log'][b, 0, :, col + 1:col + 1 + g['n_samp']] = samples
                    sig['log'][b, 1, :, col + 1:col + 1 + g['n_samp']] = a[:, 1:]
            g['state_prev'][b], g['state'][b], g['input_last'][b] = s0, samples[:, -1], a[:, -1]
            g['n_upd'][b] = nu + 1

    def _plant_predict(self, tau, t_rel):
        g = self._pl
        if g.get('model') == 'quadrotor':
            return self._quad_predict(tau, t_rel)
        if self.under_way is not None:
            self.under_way &= ~(self.arrived(self.stop_tol) & (g['n_upd'] >= 1))
        Ed = self._eval_rows(tau)[1]
        for b in range(self.B):
            if self.under_way is not None and not self.under_way[b]:
                continue
            c, t_old, u = self._plant_plan(b)
            s0 = g['state_prev'][b] if g['n_upd'][b] >= 1 else c @ self.basis.eval_basis([t_old / self.T])[0]
            self.p[b, self.o_state0:self.o_state0 + self.n_spl] = s0 + g['sample_time'] * np.cumsum((u[:, :-1] + u[:, 1:]) / 2.0, axis=1)[:, -1]
            self.p[b, self.o_input0:self.o_input0 + self.n_spl] = c @ Ed
            self.p[b, self.o_t] = t_rel

    def _plant_lag(self, pl):
        pass                                              # (`_plant_simulate` reads the plant's own `lag`)

    def _plant_rollout(self):
        pass

    def _script_alloc(self, time, what, value):
        return dict(time=time, what=what, value=value)

    def _script_advance(self, t_prev, t_now):
        advance_obstacles_scripted(self.p, self.obst, self._sc, t_prev, t_now, dt=self.update_time)

    # -- missions: the rollout kernel's MISSION instances and `omgx_batch_mission_advance` in numpy ----------------------------------
    def _mission_alloc(self, goals, n_goals, clock0):
        return dict(goals=goals.copy(), n_goals=n_goals.copy(), leg=np.zeros(self.B, dtype=np.int32), clock=np.full(self.B, clock0, dtype=np.int32),
                    arrivals=np.full((self.B, 1 + goals.shape[1]), -1, dtype=np.int32))

    def _mission_off(self):
        pass

    def _mission_clock_max(self):
        return int(self._ms['clock'].max())

    def _mission_switch(self, rows, s_old, state_now, step_index):
        ms = self._ms
        mission_next_leg_numpy(rows, ms['goals'], ms['leg'], ms['clock'], ms['arrivals'], self.p, self.x, self.lam, s_old, state_now, step_index,
                               ms['x_reset'], self.o_spl, self.L, self.o_state0, self.o_input0, ms['o_pose'], self.o_t)

    def _mission_arrived(self):
        """Who meets the stop rule now (the plant's rule asks for a simulated update, as `_plant_predict` does)."""
        return self.arrived(self.stop_tol) & ((self._pl['n_upd'] >= 1) if self._pl is not None else True)

    def _mission_advance(self, step_index):
        ms = self._ms
        hit = self.under_way & self._mission_arrived()
        start = hit & (ms['leg'] < ms['n_goals'])
        for b in np.flatnonzero(hit & ~start):
            ms['arrivals'][b, ms['leg'][b]] = step_index
        self.under_way &= ~(hit & ~start)
        now = self._pl['state'] if self._pl is not None else self.p[:, self.o_state0:self.o_state0 + self.n_dim].copy()
        self._mission_switch(np.flatnonzero(start), self.p[:, self.o_state0:self.o_state0 + self.n_dim].copy(), now, step_index)

    def _solve_rows(self, idx, warm, extra=None):
        """The agents `idx` solved as a batch of their own (independent problems: the same results), warm or -- a leg start -- cold."""
        kw = dict(self.opts, warm_start=int(warm), max_iter=self.max_iter_step if warm else self.max_iter_cold, **(extra or {}))
        dw = self.dw[idx].copy() if warm else np.zeros(len(idx))
        r = self.port.solve(self.tpl, self.p[idx], self.x[idx], lam_g0=self.lam[idx] if warm else None, status0=self.status[idx] if warm else None,
                            n_threads=self.n_threads, dw_state=dw, **kw)
        self.x[idx], self.lam[idx], self.status[idx], self.iters[idx], self.dw[idx] = r['x'], r['lam_g'], r['status'], r['iters'], dw

    def _mission_run(self, table, n_steps, iters_log, status_log):
        for k in range(n_steps):
            self._mission_step(table, self._ms['steps'] + k)
            if iters_log is not None:
                iters_log[k] = self.iters
            if status_log is not None:
                status_log[k] = self.status

    def _mission_step(self, table, step_index):
        """One step of every agent as the rollout kernel's MISSION instance runs it: the agents grouped by their leg clocks, the glue
        statements of `step` applied per group with that group's record, the switch at the stop test, then the solves -- leg starts
        cold, the others warm (the crossing ones with `cross_options`) -- each group an index sub-batch."""
        ms, pl = self._ms, self._pl
        n, o_s = self.n_dim, self.o_state0
        under0 = self.under_way.copy()
        self.iters = np.zeros(self.B, dtype=np.int32)
        snap = (self.p.copy(), self.x.copy(), self.lam.copy())
        out = [a.copy() for a in snap]
        s_old = snap[0][:, o_s:o_s + n].copy()                # (p[state0] of the previous update: read ahead of the prediction)
        final, start, crossing = (np.zeros(self.B, dtype=bool) for _ in range(3))
        for c in np.unique(ms['clock'][under0]):
            grp = under0 & (ms['clock'] == c)
            tau, t_rel, crossed = table[c]
            self.p, self.x, self.lam = (a.copy() for a in snap)
            self.under_way = grp.copy()
            if pl is None:
                self._predict(tau, t_rel)
            else:
                self._plant_predict(tau, t_rel)               # (ends the loops of the group's arrived agents ahead of the glue)
            hit = grp & ~self.under_way
            advance_obstacles(self.p, self.obst, self.update_time)
            if crossed:
                self._shift()
            if pl is None:
                hit = grp & self.arrived(self.stop_tol)
            go_on = hit & (ms['leg'] < ms['n_goals'])
            # an agent that stops for good keeps what the kernel leaves it: with the plant its rows as they were, else the glue's
            take = grp & ~(hit & ~go_on) if pl is not None else grp
            for dst, src in zip(out, (self.p, self.x, self.lam)):
                dst[take] = src[take]
            final |= hit & ~go_on
            start |= go_on
            crossing |= grp & ~hit & bool(crossed)
        self.p, self.x, self.lam = out
        for b in np.flatnonzero(final):
            ms['arrivals'][b, ms['leg'][b]] = step_index
        now = pl['state'] if pl is not None else self.p[:, o_s:o_s + n].copy()
        self._mission_switch(np.flatnonzero(start), s_old, now, step_index)
        self.under_way = under0 & ~final
        warm = self.under_way & ~start
        for idx, is_warm, extra in ((np.flatnonzero(start), False, None), (np.flatnonzero(warm & ~crossing), True, None),
                                    (np.flatnonzero(warm & crossing), True, self.cross_options)):
            if len(idx):
                self._solve_rows(idx, is_warm, extra)
        ms['clock'][warm] += 1
        if pl is not None:
            self._plant_simulate()                            # (the vehicles of the agents solved travel the update; it writes the log)
        elif self._log_in_solve:
            self._signals_append_host(self.under_way)

    def _feedback_predict(self, tau, t_rel, states, inputs, fresh, enforce):
        """`omgx_batch_predict_measured` in numpy: an agent without a fresh measurement as `_predict`, one with as `_plant_predict`
        with the measured state in the place of `state_prev` (the same statements: the same bits), or the given values (enforce)."""
        if self._fb.get('model') == 'quadrotor':
            return self._quad_feedback_predict(tau, t_rel, states, fresh, enforce)
        states = np.asarray(states, dtype=float)
        go = np.ones(self.B, dtype=bool) if fresh is None else np.asarray(fresh) != 0
        st, new = self._fb['sample_time'], {}
        if not enforce:                                   # (ahead of `_predict`: `_plant_plan` reads the time the plan was solved at)
            Ed = self._eval_rows(tau)[1]
            for b in np.flatnonzero(go):
                c, _, u = self._plant_plan(b, self._fb)
                new[b] = (states[b] + st * np.cumsum((u[:, :-1] + u[:, 1:]) / 2.0, axis=1)[:, -1], c @ Ed)
        self._predict(tau, t_rel)
        if enforce:
            self.p[go, self.o_state0:self.o_state0 + self.n_spl] = states[go]
            self.p[go, self.o_input0:self.o_input0 + self.n_spl] = 0.0 if inputs is None else np.asarray(inputs, dtype=float)[go]
        for b, (s0, i0) in new.items():
            self.p[b, self.o_state0:self.o_state0 + self.n_spl] = s0
            self.p[b, self.o_input0:self.o_input0 + self.n_spl] = i0

    def _signals_summary(self, target):
        return signals_summary_numpy(self._sig['log'], self._sig['count'], target, self._sig['sample_time'])


def mission_next_leg_numpy(rows, goals, leg, clock, arrivals, p, x, lam, s_old, state_now, step_index, x_reset, o_spl, L, o_state0, o_input0,
                           o_poseT, o_t):
    """`mission_next_leg_agent` (csrc/omgx_device.h) in numpy for the agents `rows`: the leg switch of `BatchP2P.mission`, the same
    statements in the same order (include/omgx.h OMGX_HAS_MISSION).  s_old [B, n_dim]: p[state0] of the previous update (where the
    guess starts), state_now [B, n_dim]: where the vehicle is.  The coefficients are numpy's own linspace statement --
    start + i * ((stop - start) / (L - 1)), the last one the goal itself."""
    n = goals.shape[2]
    for b in rows:
        g, s = goals[b, leg[b]], np.array(s_old[b], dtype=float)
        p[b, o_poseT:o_poseT + n] = g
        x[b] = x_reset
        step = (g - s) / (L - 1)
        c = s[:, None] + np.arange(L)[None, :] * step[:, None]
        c[:, L - 1] = g
        x[b, o_spl:o_spl + n * L] = c.reshape(-1)
        lam[b] = 0.0
        p[b, o_state0:o_state0 + n] = state_now[b]
        p[b, o_input0:o_input0 + n] = 0.0
        p[b, o_t] = 0.0
        clock[b] = 0
        arrivals[b, leg[b]] = step_index
        leg[b] += 1


def quad_inputs_numpy(dd, ddd, g):
    """The Quadrotor's inputs (u1, u2) [2, ...] from the plan's second and third time derivatives dd, ddd [2, ...]: the statements of
    `quad_inputs` (csrc/omgx_device.h), which are `vehicles/quadrotor.py:136-139`."""
    n2 = (dd[1] + g) * (dd[1] + g) + dd[0] * dd[0]
    return np.array([np.sqrt(n2), (ddd[0] * (dd[1] + g) - dd[0] * ddd[1]) / n2])


def quad_ode_numpy(s, u1, u2, g):
    """`Quadrotor.ode` (`vehicles/quadrotor.py:149-152`): state (x, y, dx, dy, theta), inputs thrust and pitch rate."""
    return np.array([s[2], s[3], u1 * math.sin(s[4]), u1 * math.cos(s[4]) - g, u2])


def quad_rk4_numpy(s0, a, h, g):
    """State samples 0 .. n [5, n + 1] of the Quadrotor from s0 [5] under the linearly interpolated input samples a [2, n + 1]: classical
    Runge-Kutta per sample interval, the statements of `quad_rk4_step` (csrc/omgx_device.h) in the same order."""
    n = a.shape[1] - 1
    out = np.empty((5, n + 1))
    s = np.array(s0, dtype=float)
    out[:, 0] = s
    for i in range(n):
        u1a, u2a, u1b, u2b = a[0, i], a[1, i], a[0, i + 1], a[1, i + 1]
        u1m, u2m = 0.5 * (u1a + u1b), 0.5 * (u2a + u2b)
        k1 = quad_ode_numpy(s, u1a, u2a, g)
        k2 = quad_ode_numpy(s + 0.5 * h * k1, u1m, u2m, g)
        k3 = quad_ode_numpy(s + 0.5 * h * k2, u1m, u2m, g)
        k4 = quad_ode_numpy(s + h * k3, u1b, u2b, g)
        s = s + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        out[:, i + 1] = s
    return out


def signals_summary_numpy(log, count, target, sample_time):
    """`omgx_batch_signals_reduce` in numpy: [B, 8] from a log [B, n_der, n_spl, cap], count [B], target [B, n_spl]."""
    log, count, target = np.asarray(log), np.asarray(count), np.asarray(target)
    B, n_der = log.shape[0], log.shape[1]
    out = np.zeros((B, 8))
    for b in range(B):
        n = int(count[b])
        if n < 1:
            continue
        sig = log[b, :, :, :n]
        nrm = lambda a: np.sqrt((a * a).sum(axis=0))
        out[b, 0], out[b, 1] = n, (n - 1) * sample_time
        out[b, 2] = nrm(np.diff(sig[0], axis=1)).sum()
        if n_der >= 2:
            out[b, 3], out[b, 6] = nrm(sig[1]).max(), nrm(sig[1])[-1]
        if n_der >= 3:
            out[b, 4] = nrm(sig[2]).max()
        out[b, 5] = nrm(sig[0][:, -1:] - target[b][:, None])[0]
    return out


def split_bounds(B, n_streams, slots=None):
    """Contiguous sub-batches [(lo, hi)] of a batch of B agents.  Without `slots`: sizes that differ by at most one.  With the number
    of workgroups the chip holds at once (`slots`): sizes in units of a quarter of it, the larger sub-batches first, the last one
    takes the remainder -- 1024 agents on 512 slots in three sub-batches: 384 / 384 / 256 instead of 342 / 341 / 341.  Measured on
    the benchmark batch (round 5, four runs each on two boxes): 2.29-2.31 M solves/s against 2.20-2.26 M for the even split, and
    against 2.19-2.22 M for 512 / 256 / 256 and 2.21-2.25 M for 416 / 416 / 192: launches whose sizes are multiples of a quarter
    of the resident workgroups leave fewer of them idle when two sub-batches share the chip."""
    from .distributed import shard_range
    even = [shard_range(B, s, n_streams) for s in range(n_streams)]
    unit = (slots or 0) // 4
    if unit < 1 or B < unit * n_streams:
        return even
    units = -(-B // unit)                                   # ceil: the last unit may be a partial one
    per = [units // n_streams + (1 if s < units % n_streams else 0) for s in range(n_streams)]
    sizes = [u * unit for u in per]
    sizes[-1] -= sum(sizes) - B
    if min(sizes) < 1:
        return even
    lo, out = 0, []
    for n in sizes:
        out.append((lo, lo + n))
        lo += n
    return out


_SUB_BATCH_STREAMS = {}


def sub_batch_streams(dev, n):
    """The HIP streams the sub-batches of a device run on: HIGH-PRIORITY streams, created once per device, shared by every
    `StreamedP2P` on it and put to use (an event record) right away.  The HIP runtime maps streams onto `GPU_MAX_HW_QUEUES`
    (four) hardware queues per priority level when they are first used -- a new queue while the level has fewer than four, else
    the least-used one -- so whether three default-priority streams got three queues depended on what the process had created
    before (the null stream, every library handle's own stream, a process group's): measured on the benchmark batch, round 6
    (`profiles/r06_stream_placement.txt`), 1.2 M instead of 2.2 M solves/s when a library handle was created ahead of the first
    `StreamedP2P`, or when a second `StreamedP2P` followed the first in a process -- two sub-batches on one queue run their
    launches one after the other.  Nothing else in a process uses the high-priority level: its first three streams get a
    queue each, whatever came before (2.15-2.20 M in all four creation orders tried, with and without a process group)."""
    import torch
    key = (dev.type, dev.index or 0)
    have = _SUB_BATCH_STREAMS.setdefault(key, [])
    while len(have) < n:
        st = torch.cuda.Stream(device=dev, priority=int(os.environ.get('OMGX_STREAM_PRIORITY', '-1')))
        if not os.environ.get('OMGX_NO_STREAM_TOUCH'):      # (developer knob: the order-dependent behaviour of rounds 5 / 6)
            torch.cuda.Event().record(st)
        have.append(st)
    return have[:n]


class StreamedP2P(object):
    """The batch as `n_streams` sub-batches, each a `BatchP2P` with its own library handle on its own HIP stream.  The problems of
    a point-to-point batch are independent, so nothing orders the steps of one sub-batch against those of another: while one waits
    for a straggler of its step, the next step of the other fills the idle workgroup slots (1024 agents, two streams: 2.07 M
    solves/s against 1.74 M on one stream; more streams lose again -- every handle launches a full grid of persistent workgroups).
    Per agent the same launches in the same order as `BatchP2P`: the same bits (tests/test_gpu_rollout.py).  Since round 5 this is
    what `receding_horizon_batch` hands out for a batch of at least two rounds of resident workgroups: the per-step product path.
    `step` returns whether the step crossed a knot; `x, p, lam, status, iters` join the streams and concatenate the sub-batches
    (`gather`); `parts[k]` / `streams[k]` give the sub-batches to callers that attach events, statistics or copies per stream."""

    def __init__(self, problem, P, n_streams=2, device=None, slots=None, **kw):
        import torch
        self.torch = torch
        B = P['p'].shape[0]
        if n_streams < 1 or n_streams > B:
            raise ValueError('%d agents do not split into %d sub-batches' % (B, n_streams))
        self.bounds = split_bounds(B, n_streams, slots)
        self.dev = device if device is not None else torch.device('cuda', 0)
        self.streams = sub_batch_streams(self.dev, n_streams) if not os.environ.get('OMGX_NO_STREAM_TOUCH') else \
            [torch.cuda.Stream(device=self.dev) for _ in range(n_streams)]
        self.parts = []
        # (the caller's stream may still be writing what the sub-batches read, and the other way round at the end)
        ready = torch.cuda.current_stream(self.dev).record_event()
        for (lo, hi), st in zip(self.bounds, self.streams):
            Ps = dict(P, p=P['p'][lo:hi], x0=P['x0'][lo:hi])
            st.wait_event(ready)
            with torch.cuda.stream(st):
                self.parts.append(DeviceP2P(problem, Ps, device=self.dev, **kw))
        self.B = B
        self.kind = 'hip'
        self.tpl, self.problem = self.parts[0].tpl, problem

    def _each(self, fn):
        out = []
        for part, st in zip(self.parts, self.streams):
            with self.torch.cuda.stream(st):
                out.append(fn(part))
        return out

    def solve_cold(self, **kw):
        return max(self._each(lambda m: m.solve_cold(**kw)))

    def restart_failed(self, *a, **kw):
        return max(self._each(lambda m: m.restart_failed(*a, **kw)))

    def step(self, events=None, before_solve=None, states=None, inputs=None, fresh=None, enforce=False):
        """events: one (start, stop) pair per sub-batch (stamped on that sub-batch's solve kernel).  states / inputs / fresh
        (`BatchP2P.step`): of the whole batch, every sub-batch gets its rows; the sub-batches' streams wait for what the caller's
        stream has enqueued so far (the tensors may still be written there)."""
        evs = events if events is not None else [None] * len(self.parts)
        hooks = before_solve if isinstance(before_solve, (list, tuple)) else [before_solve] * len(self.parts)
        fed = {}
        if states is not None or inputs is not None or fresh is not None or enforce:
            for nm, a, shape in (('states', states, (self.B, self.parts[0]._state_width())), ('inputs', inputs, (self.B, self.parts[0].n_spl)), ('fresh', fresh, (self.B,))):
                if a is not None and tuple(a.shape) != shape:
                    raise ValueError('step: %s must be %s, got %s' % (nm, list(shape), list(a.shape)))
            self.fork()
            fed = dict(states=states, inputs=inputs, fresh=fresh)
        out = []
        for (lo, hi), part, st, ev, hk in zip(self.bounds, self.parts, self.streams, evs, hooks):
            kw = dict((nm, None if a is None else a[lo:hi]) for nm, a in fed.items())
            if fed:
                kw['enforce'] = enforce
            with self.torch.cuda.stream(st):
                out.append(part.step(events=ev, before_solve=hk, **kw))
        return any(out)

    def stop_at_arrival(self, stop_tol=1e-3, on=True):
        for m in self.parts:
            m.stop_at_arrival(stop_tol, on)

    def record_signals(self, sample_time=0.01, max_updates=200, on=True, cap=None):
        """`BatchP2P.record_signals` for every sub-batch (each logs on its own stream)."""
        self._each(lambda m: m.record_signals(sample_time, max_updates, on, cap))

    def plant(self, sample_time=0.01, max_updates=200, disturbance=None, on=True, time_constant=None, model=None, gravity=9.81):
        """`BatchP2P.plant` for every sub-batch, each with its rows of the disturbance and of a per-agent time constant."""
        if on and model is not None:                         # (ahead of the first sub-batch: a refused call changes none)
            self.parts[0]._quad_model('plant', model)
            if time_constant is not None:
                raise NotImplementedError("plant(): the first-order actuator lag is not simulated with model='quadrotor'")
        tc = None
        if time_constant is not None:
            n = self.bounds[-1][1]
            tc = np.asarray(time_constant, dtype=float)
            if tc.shape not in ((), (n,)) or not (np.isfinite(tc).all() and (tc > 0.0).all()):      # (ahead of the first sub-batch: a refused call changes none)
                raise ValueError('plant: time_constant must be a positive finite scalar or one such value per agent [%d]' % n)
            tc = np.broadcast_to(tc, (n,))
        for (lo, hi), m, st in zip(self.bounds, self.parts, self.streams):
            with self.torch.cuda.stream(st):
                m.plant(sample_time, max_updates, None if disturbance is None else disturbance[lo:hi], on, None if tc is None else tc[lo:hi],
                        model=model, gravity=gravity)

    def feedback(self, sample_time=0.01, on=True, model=None, gravity=9.81):
        """`BatchP2P.feedback` for every sub-batch; `step(states=...)` then hands each its rows."""
        for m in self.parts:
            m.feedback(sample_time, on, model=model, gravity=gravity)

    def obstacle_script(self, events=None, on=True):
        """`BatchP2P.obstacle_script` for every sub-batch, each with its rows of the events."""
        for (lo, hi), m, st in zip(self.bounds, self.parts, self.streams):
            with self.torch.cuda.stream(st):
                m.obstacle_script(None if events is None else dict((k, np.asarray(v)[lo:hi]) for k, v in events.items()), on)

    def plant_state(self):
        """`BatchP2P.plant_state` of the whole batch, joined and concatenated like `signals`."""
        parts = [m.plant_state() for m in self.parts]
        self.join()
        return dict((key, self.torch.cat([q[key] for q in parts])) for key in parts[0])

    def signals(self):
        """`BatchP2P.signals` of the whole batch: the sub-batches' logs joined and concatenated, like `gather`."""
        parts = [m.signals() for m in self.parts]
        self.join()
        out = dict(time=parts[0]['time'])
        for key in parts[0]:
            if key != 'time':
                out[key] = self.torch.cat([q[key] for q in parts])
        return out

    def horizon(self):
        """`BatchP2P.horizon` of the whole batch."""
        out = self._each(lambda m: m.horizon())
        self.join()
        return self.torch.cat(out)

    def summary(self):
        out = self._each(lambda m: m.summary())
        self.join()
        return self.torch.cat(out)

    @property
    def under_way(self):
        if self.parts[0].under_way is None:
            return None
        return self.gather('under_way')

    @property
    def time(self):
        return self.parts[0].time

    @time.setter
    def time(self, t):
        for m in self.parts:
            m.time = t

    def synchronize(self):
        for st in self.streams:
            st.synchronize()

    def join(self):
        """The caller's current stream waits for everything enqueued on the sub-batches' streams (no host sync)."""
        cur = self.torch.cuda.current_stream(self.dev)
        for st in self.streams:
            cur.wait_stream(st)

    def fork(self):
        """The sub-batches' streams wait for what the caller's current stream has enqueued so far (e.g. a reset of x / p)."""
        cur = self.torch.cuda.current_stream(self.dev)
        for st in self.streams:
            st.wait_stream(cur)

    def gather(self, name):
        self.join()
        return self.torch.cat([getattr(m, name) for m in self.parts])

    def load(self, x=None, p=None):
        """x / p of the whole batch -> the sub-batches (device tensors [B, *]), ordered behind the caller's stream."""
        self.fork()
        for (lo, hi), m, st in zip(self.bounds, self.parts, self.streams):
            with self.torch.cuda.stream(st):
                if x is not None:
                    m.x.copy_(x[lo:hi])
                if p is not None:
                    m.p.copy_(p[lo:hi])

    x = property(lambda self: self.gather('x'))
    p = property(lambda self: self.gather('p'))
    lam = property(lambda self: self.gather('lam'))
    status = property(lambda self: self.gather('status'))
    iters = property(lambda self: self.gather('iters'))

    def host(self, name):
        return self.gather(name).cpu().numpy()

    def close(self):
        self.synchronize()
        for m in self.parts:
            m.solver.close()


# Sub-batches of the per-step product path: three, on streams with a hardware queue each (`sub_batch_streams`).  Measured on the
# 1024-agent batch with the streams in their own (high-priority) queue pool, round 6: two 2.09 M, three 2.20-2.25 M, four
# 2.22-2.25 M (p50 step latency 0.75 / 0.66-0.91 / 0.97-1.01 ms), five 1.42 M solves/s -- the pool has four queues, a fifth stream
# shares one and its launches queue behind another sub-batch's.
PRODUCT_PATH_STREAMS = 3


def product_path_streams(process_group=None, hw_queues=None):
    """Sub-batches of the per-step product path: `PRODUCT_PATH_STREAMS`.  (While the sub-batch streams came from the runtime's
    common pool of four hardware queues the count depended on what else the process had created -- a `torch.distributed` process
    group's stream, a library handle ahead of the first `StreamedP2P` -- and this function picked two or four under a process
    group; with the streams in a queue pool of their own, `sub_batch_streams`, three is measured the same with and without a group
    and with four or eight hardware queues: 2.20 M in each case.  The arguments are kept for callers of that version.)"""
    return PRODUCT_PATH_STREAMS


def receding_horizon_batch(problem, P, device=None, n_streams='auto', **kw):
    """The per-step product path for a batch of independent agents: a `BatchP2P`, or -- when the batch is at least two rounds
    of resident workgroups (1024 agents of config 2 on 512 slots) -- the same batch as `PRODUCT_PATH_STREAMS` stream-ordered
    sub-batch launches per step (`StreamedP2P`): a step of the whole batch is quantised in rounds of the resident workgroups and
    one straggler costs the batch a whole extra round; with the sub-batches on their own streams the next step
    of one fills the slots the stragglers of the others leave idle.  Per agent the same launches, the same bits."""
    import torch
    dev = device if device is not None else torch.device('cuda', 0)
    B = P['p'].shape[0]
    if n_streams == 'auto' or n_streams <= 1:
        whole = BatchP2P(problem, P, ops='hip', device=dev, **kw)
        # (the launch grid of the handle = the workgroups the chip holds at once, capped at the batch)
        slots = whole.solver.workspace()['n_slabs']
        if n_streams != 'auto' or B < 2 * slots:
            return whole
        whole.solver.close()
        return StreamedP2P(problem, P, n_streams=product_path_streams(), device=dev, slots=slots, **kw)
    return StreamedP2P(problem, P, n_streams=n_streams, device=dev, **kw)
