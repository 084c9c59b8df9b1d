# This file is derived from OMG-tools (meco-group/omg-tools, `omgtools/basics/spline.py`, `spline_extra.py` (API surface)).
#
# OMG-tools -- Optimal Motion Generation-tools
# Copyright (C) 2016 Ruben Van Parys & Tim Mercy, KU Leuven.
# All rights reserved.
#
# OMG-tools is free software; you can redistribute it and/or
# modify it under the terms of the GNU Lesser General Public
# License as published by the Free Software Foundation; either
# version 3 of the License, or (at your option) any later version.
# This software is distributed in the hope that it will be useful,
# but WITHOUT ANY WARRANTY; without even the implied warranty of
# MERCHANTABILITY or FITNESS FOR A PARTICULAR PURPOSE. See the GNU
# Lesser General Public License for more details.
#
# You should have received a copy of the GNU Lesser General Public
# License along with this program; if not, write to the Free Software
# Foundation, Inc., 51 Franklin Street, Fifth Floor, Boston, MA 02110-1301 USA
#
# Modifications: the public classes, option names, method order and messages of the files named
# above are kept so that scripts written for OMG-tools run unchanged where the original package is
# not installed (benchmark and test tiers of this repository); the CasADi expression layer underneath
# is replaced by explicit polynomials (symbolic.py) and the solver call by the HIP path (backend.py).
# Where the original package IS installed, use omgx_shim instead: it runs the original classes themselves.

"""B-spline bases and splines with numeric or polynomial (`Poly`) coefficients.

Host-side, construction-time spline algebra.  Behavioural spec (not code) is the
reference's `basics/spline.py` (Basis 117-205, BSplineBasis 208-324, BSpline
392-512) and `basics/spline_extra.py` (evalspline 28-55, integrals 58-85,
shift matrices 107-255, knot insertion 258-305, sampling 406-410).

Differences in *how* (results agree to rounding, pinned by tests/golden):
  * basis-change and product matrices are obtained by exact least squares on
    Chebyshev nodes of every knot span instead of collocation at the arg-max
    of a 501-point grid (`spline.py:283-306`);
  * the horizon-shift matrix is obtained from the polynomial continuation of
    the last span instead of the derivative-matching construction
    (`spline_extra.py:107-191`);
  * coefficients may be `Poly` objects (symbolic.py) where the reference uses
    CasADi MX.
"""
import numpy as np
from collections import Counter

from .symbolic import (Poly, SymbolTable, is_symbolic, matvec, as_poly_array)

_TOL = 1e-10        # entries below this are structural zeros (spline.py:305)


def _cheb_nodes(a, b, n):
    k = np.arange(n)
    x = np.cos((2 * k + 1) * np.pi / (2 * n))
    return 0.5 * (a + b) + 0.5 * (b - a) * x


class BSplineBasis(object):
    """Knot vector + degree; evaluation follows the reference's span
    convention: spans are (k_i, k_{i+1}] except the spans glued to the first
    knot, which are closed on the left (`basics/spline.py:131-136`)."""
    _cache = {}

    def __new__(cls, knots, degree):
        knots = np.asarray(knots, dtype=float)
        key = (knots.tobytes(), int(degree))
        inst = cls._cache.get(key)
        if inst is None:
            inst = object.__new__(cls)
            inst.knots = knots.copy()
            inst.degree = int(degree)
            inst._memo = {}
            cls._cache[key] = inst
        return inst

    def __len__(self):
        return len(self.knots) - self.degree - 1

    def __eq__(self, other):
        return self is other

    def __hash__(self):
        return id(self)

    def __call__(self, x):
        return self.eval_basis(x)

    # -- evaluation ----------------------------------------------------------
    def eval_basis(self, x):
        """Dense (len(x), len(self)) matrix of basis function values."""
        x = np.atleast_1d(np.asarray(x, dtype=float))
        k, d = self.knots, self.degree
        nk = len(k)
        lvl = np.zeros((nk - 1, x.size))
        for i in range(nk - 1):
            left_closed = (i < d + 1) and (k[0] == k[i])
            lo = (x >= k[i]) if left_closed else (x > k[i])
            lvl[i] = lo & (x <= k[i + 1])
        for p in range(1, d + 1):
            nxt = np.zeros((nk - p - 1, x.size))
            for i in range(nk - p - 1):
                den = k[i + p] - k[i]
                if den != 0:
                    nxt[i] += (x - k[i]) / den * lvl[i]
                den = k[i + p + 1] - k[i + 1]
                if den != 0:
                    nxt[i] += (k[i + p + 1] - x) / den * lvl[i + 1]
            lvl = nxt
        return lvl.T.copy()

    def spans(self):
        """Distinct non-empty knot spans."""
        u = np.unique(self.knots)
        return list(zip(u[:-1], u[1:]))

    def fit_points(self, degree=None):
        """Chebyshev nodes on each span, enough to pin a piecewise polynomial
        of the given degree."""
        degree = self.degree if degree is None else degree
        return np.concatenate([_cheb_nodes(a, b, degree + 2)
                               for a, b in self.spans()])

    def support(self):
        d = self.degree
        return list(zip(self.knots[:-(d + 1)], self.knots[d + 1:]))

    def greville(self):
        d = self.degree
        return [self.knots[i + 1:i + d + 1].sum() / d for i in range(len(self))]

    # -- derived bases ---------------------------------------------------------
    def derivative(self, o=1):
        """(basis of the o-th derivative, matrix P with c' = P c)."""
        key = ('der', o)
        if key not in self._memo:
            k, d, n = self.knots, self.degree, len(self)
            P = np.eye(n)
            for step in range(o):
                dd = d - step
                kk = k[step:len(k) - step]
                rows = n - step - 1
                D = np.zeros((rows, rows + 1))
                for i in range(rows):
                    w = dd / (kk[i + dd + 1] - kk[i + 1])
                    D[i, i], D[i, i + 1] = -w, w
                P = D @ P
            self._memo[key] = (BSplineBasis(k[o:len(k) - o], d - o), P)
        return self._memo[key]

    def _combine(self, other, degree):
        cs, co = Counter(self.knots.tolist()), Counter(other.knots.tolist())
        knots = []
        for b in sorted(set(cs) | set(co)):
            m = max(cs[b] + degree - self.degree if b in cs else -1,
                    co[b] + degree - other.degree if b in co else -1)
            knots += [b] * int(m)
        return BSplineBasis(knots, degree)

    def __add__(self, other):
        if isinstance(other, BSplineBasis):
            return self._combine(other, max(self.degree, other.degree))
        return self

    __radd__ = __add__
    __sub__ = __add__
    __rsub__ = __add__

    def __mul__(self, other):
        if isinstance(other, BSplineBasis):
            return self._combine(other, self.degree + other.degree)
        return self

    __rmul__ = __mul__

    def pairs(self, other):
        """Index pairs (i, j) whose supports overlap (the only non-zero
        products), in row-major order."""
        key = ('pairs', other)
        if key not in self._memo:
            pi, pj = [], []
            for i, (a0, a1) in enumerate(self.support()):
                for j, (b0, b1) in enumerate(other.support()):
                    if max(a0, b0) < min(a1, b1):
                        pi.append(i)
                        pj.append(j)
            self._memo[key] = (np.array(pi), np.array(pj))
        return self._memo[key]

    def transform(self, other):
        """T with  other(x) == self(x) @ T  (other's span inside self's)."""
        key = ('tf', other)
        if key not in self._memo:
            x = self.fit_points()
            T = np.linalg.lstsq(self.eval_basis(x), other.eval_basis(x),
                                rcond=None)[0]
            T[np.abs(T) < _TOL] = 0.
            self._memo[key] = T
        return self._memo[key]

    def product_transform(self, a, b):
        """T with (a-spline * b-spline) coefficients on self ==
        T @ (ca[pi] * cb[pj]) for (pi, pj) = a.pairs(b)."""
        key = ('ptf', a, b)
        if key not in self._memo:
            pi, pj = a.pairs(b)
            x = self.fit_points()
            prod = a.eval_basis(x)[:, pi] * b.eval_basis(x)[:, pj]
            T = np.linalg.lstsq(self.eval_basis(x), prod, rcond=None)[0]
            T[np.abs(T) < _TOL] = 0.
            self._memo[key] = T
        return self._memo[key]

    def insert_knots(self, knots):
        new = np.setdiff1d(knots, self.knots)
        return BSplineBasis(np.sort(np.r_[self.knots, new]), self.degree)

    def scale(self, factor, shift=0.):
        return BSplineBasis(self.knots * factor + shift, self.degree)


class BSpline(object):
    """basis + coefficient vector (float ndarray or object ndarray of Poly)."""

    def __init__(self, basis, coeffs):
        self.basis = basis
        if is_symbolic(coeffs):
            self.coeffs = np.asarray(coeffs, dtype=object)
        else:
            self.coeffs = np.asarray(coeffs, dtype=float).reshape(-1)

    def __len__(self):
        return len(self.basis)

    def __call__(self, x):
        if isinstance(x, Poly):
            return evalspline(self, x)
        scalar = np.isscalar(x)
        val = matvec(self.basis.eval_basis(x), self.coeffs)
        return val[0] if scalar else val

    def __neg__(self):
        return BSpline(self.basis, -self.coeffs)

    def __add__(self, other):
        if isinstance(other, BSpline):
            basis = self.basis + other.basis
            return BSpline(basis,
                           matvec(basis.transform(self.basis), self.coeffs) +
                           matvec(basis.transform(other.basis), other.coeffs))
        return BSpline(self.basis, self.coeffs + other)

    __radd__ = __add__

    def __sub__(self, other):
        return self + (-other)

    def __rsub__(self, other):
        return (-self) + other

    def __mul__(self, other):
        if isinstance(other, BSpline):
            basis = self.basis * other.basis
            pi, pj = self.basis.pairs(other.basis)
            T = basis.product_transform(self.basis, other.basis)
            return BSpline(basis, matvec(T, self.coeffs[pi] * other.coeffs[pj]))
        return BSpline(self.basis, self.coeffs * other)

    __rmul__ = __mul__

    def __pow__(self, power):
        out = self
        for _ in range(int(power) - 1):
            out = out * self
        return out

    def derivative(self, o=1):
        if o == 0:
            return self
        basis, P = self.basis.derivative(o)
        return BSpline(basis, matvec(P, self.coeffs))

    def integral(self):
        k, d = self.basis.knots, self.basis.degree
        w = (k[d + 1:] - k[:-(d + 1)]) / (d + 1)
        return (w * self.coeffs).sum()

    def insert_knots(self, knots):
        basis = self.basis.insert_knots(knots)
        return BSpline(basis, matvec(basis.transform(self.basis), self.coeffs))

    def scale(self, factor, shift=0.):
        return BSpline(self.basis.scale(factor, shift), self.coeffs)


# ---------------------------------------------------------------------------
# spline_extra equivalents
# ---------------------------------------------------------------------------

def evalspline(spline, x):
    """Spline value at x.  For a parameter-dependent x (e.g. t/T) the basis
    functions become derived atoms evaluated per agent on the device
    (reference: symbolic Cox-de Boor, `spline_extra.py:28-55`)."""
    if isinstance(x, Poly) and not x.is_constant():
        ids = SymbolTable.current().new_bspl_atoms(
            spline.basis.knots, spline.basis.degree, x)
        acc = Poly()
        for i, sym in enumerate(ids):
            acc = acc + spline.coeffs[i] * Poly.symbol(sym)
        return acc
    if isinstance(x, Poly):
        x = x.constant_value()
    return matvec(spline.basis.eval_basis([x]), spline.coeffs)[0]


def running_integral(spline):
    """Antiderivative spline (value 0 at the first knot); `spline_extra.py:58-76`."""
    k, d = spline.basis.knots, spline.basis.degree
    basis_int = BSplineBasis(np.r_[k[0], k, k[-1]], d + 1)
    w = (k[d + 1:] - k[:-(d + 1)]) / (d + 1)
    if is_symbolic(spline.coeffs):
        acc, out = Poly(), [Poly()]
        for i in range(len(spline)):
            acc = acc + spline.coeffs[i] * float(w[i])
            out.append(acc)
        coeffs = as_poly_array(out)
    else:
        coeffs = np.r_[0., np.cumsum(w * spline.coeffs)]
    return BSpline(basis_int, coeffs)


def definite_integral(spline, a, b):
    s_int = running_integral(spline)
    return evalspline(s_int, b) - evalspline(s_int, a)


def _continued_basis(basis, x):
    """Basis functions evaluated at x, where for x beyond the last knot each
    function is the polynomial continuation of its last-span piece."""
    x = np.asarray(x, dtype=float)
    out = basis.eval_basis(np.minimum(x, basis.knots[-1]))
    beyond = x > basis.knots[-1]
    if beyond.any():
        a, b = basis.spans()[-1]
        nodes = _cheb_nodes(a, b, basis.degree + 1)
        vals = basis.eval_basis(nodes)
        # Lagrange extrapolation through the d+1 nodes (exact for degree d)
        for r in np.nonzero(beyond)[0]:
            lag = np.ones(len(nodes))
            for i in range(len(nodes)):
                for j in range(len(nodes)):
                    if i != j:
                        lag[i] *= (x[r] - nodes[j]) / (nodes[i] - nodes[j])
            out[r] = lag @ vals
    return out


def extrapolate_T(basis, t_extra):
    """Matrix to the basis with one extra span [k_end, k_end + t_extra] on which
    the spline continues its last polynomial piece (`spline_extra.py:107-157`)."""
    k, d = basis.knots, basis.degree
    m = 1
    while k[-d - 2 - m] >= k[-d - 2]:
        m += 1
    knots2 = np.r_[k[:-d - 1], k[-d - 1] * np.ones(m),
                   (k[-1] + t_extra) * np.ones(d + 1)]
    basis2 = BSplineBasis(knots2, d)
    x = basis2.fit_points()
    T = np.linalg.lstsq(basis2.eval_basis(x), _continued_basis(basis, x),
                        rcond=None)[0]
    T[np.abs(T) < _TOL] = 0.
    return T


def since_knot(t, knot_time):
    """Seconds since the last knot of the receding horizon at time t: the reference's statement `np.round(t, 6) % knot_time`
    (`problems/point2point.py:177`, the parameter `t`), repaired where it contradicts the reference's own crossing test
    `int(np.round(t / knot_time, 6))` (`point2point.py:190-193`).  When t is a whole number of knot intervals whose product rounds
    above t -- T = 10 s, 11 intervals: `knot_time = (int(T * 1000) / 11) / 1000` (`point2point.py:134`) is 0.9090909090909092, one ulp
    above 10 / 11, and 11 of them exceed t = 10.0 -- the remainder comes out one interval short of zero (0.909...) while the
    crossing test has just moved the horizon on: the initial-condition rows are then evaluated 0.909 s
    into a plan that begins NOW, every vehicle re-plans from a start that violates them, and the next update jumps back.  The
    reference's IPOPT absorbs it; measured here (1024 agents of config 2, update 99 = t 10.0): the slowest agent 62 iterations,
    six for the update after.  A remainder within 1e-9 of a whole interval is the knot itself: 0."""
    rel = float(np.round(t, 6) % knot_time)
    return 0.0 if knot_time - rel < 1e-9 else rel


def step_clock(t_prev, dt, knot_time, T, t_now=None):
    """The clock of one receding-horizon update from t_prev to t_now = t_prev + dt (a caller that is handed the time of the
    update instead of forming it passes `t_now` and dt = t_now - t_prev).  Returns (t_now, tau, t_rel, crossed): tau = where on
    the current plan (in units of the horizon T) the ideal prediction reads the initial conditions of the update; t_rel = the
    parameter `t` of the update (`since_knot`); crossed = the horizon start passed a knot (`point2point.py:190-193`: shift the
    warm start).  The one statement of it: the stepwise loop, the rollout's step list and the formation loop demand the same
    bits from it."""
    if t_now is None:
        t_now = t_prev + dt
    rel_prev = since_knot(t_prev, knot_time)
    tau = (rel_prev + dt) / T
    crossed = int(np.round(t_prev / knot_time, 6)) < int(np.round(t_now / knot_time, 6))
    t_rel = since_knot(t_now, knot_time)
    return t_now, tau, t_rel, crossed


def advance_obstacles(p, obst, dt):
    """The moving obstacles of `obst` [(o_x, o_v, o_a, n_dim)] advanced by dt in the parameter array p [B, *] (numpy or torch, in
    place) between two updates: x <- x + v dt + a dt^2 / 2, v <- v + a dt (`environment/obstacle.py:246-264` without bouncing).
    These statements in this order: the rollout kernel reproduces their rounding."""
    for ox, ov, oa, nd in obst:
        px, pv, pa = p[:, ox:ox + nd], p[:, ov:ov + nd], p[:, oa:oa + nd]
        px += dt * pv + (0.5 * dt * dt) * pa
        pv += dt * pa


SCRIPT_EPS = 1e-9      # (an event within it of an update's end belongs to that update: the tolerance of `since_knot`)


def advance_obstacles_scripted(p, obst, script, t_prev, t_now, dt=None):
    """`advance_obstacles` from t_prev to t_now with an obstacle script (include/omgx.h OMGX_HAS_OBSTACLE_SCRIPT has the statement;
    the reference's `simulation={'trajectories': ...}`, `environment/obstacle.py:172-264`): script = dict `time` [B, E] (absolute,
    ascending per agent, pads +inf), `what` [B, E] (3 * index into `obst` + kind, kind 0 / 1 / 2 = position / velocity /
    acceleration), `value` [B, E, 3].  p [B, *] numpy, in place, row by row.  An event belongs to the update if
    t_prev + 1e-9 < time <= t_now + 1e-9; a row without one gets the statements of `advance_obstacles` with `dt` (None: t_now -
    t_prev; a loop passes its update time, so that an update without an event keeps the bits of the plain loop); otherwise the
    motion is split at the events, in table order, and each adds its value to its kind.  An event on t_now (within 1e-9) that
    nothing precedes in the update sees the whole-interval statements with `dt` itself.  The device routine
    `obstacles_advance_agent` makes the same roundings in the same order."""
    dt = t_now - t_prev if dt is None else dt
    time, what, value = np.asarray(script['time']), np.asarray(script['what']), np.asarray(script['value'])
    lo, hi = t_prev + SCRIPT_EPS, t_now + SCRIPT_EPS

    def move(row, h, c2):
        for ox, ov, oa, nd in obst:
            px, pv, pa = row[ox:ox + nd], row[ov:ov + nd], row[oa:oa + nd]
            px += h * pv + c2 * pa
            pv += h * pa

    for b in range(p.shape[0]):
        row, t_cur, any_event = p[b], t_prev, False
        for e in range(time.shape[1]):
            t_e = float(time[b, e])
            if not t_e > lo:
                continue
            if t_e > hi:
                break
            any_event = True
            if t_cur == t_prev and t_now - t_e <= SCRIPT_EPS:
                move(row, dt, 0.5 * dt * dt)
                t_cur = t_now
            else:
                t_to = t_e if t_e < t_now else t_now
                h = t_to - t_cur
                if h > SCRIPT_EPS:
                    move(row, h, 0.5 * h * h)
                    t_cur = t_to
            q, kind = divmod(int(what[b, e]), 3)
            if 0 <= q < len(obst):
                off, nd = obst[q][kind], obst[q][3]
                row[off:off + nd] += value[b, e, :nd]
        if not any_event:
            move(row, dt, 0.5 * dt * dt)
        else:
            h = t_now - t_cur
            if h > SCRIPT_EPS:
                move(row, h, 0.5 * h * h)


def shiftoverknot_T(basis):
    """Warm-start matrix when the horizon start passes the first interior knot:
    the new coefficients describe s(tau + delta) on the same (uniform) knot
    vector, the last span being the continuation of the old last piece
    (`spline_extra.py:165-191`)."""
    k, d = basis.knots, basis.degree
    delta = k[d + 1] - k[0]
    x = basis.fit_points()
    T = np.linalg.lstsq(basis.eval_basis(x), _continued_basis(basis, x + delta),
                        rcond=None)[0]
    T[np.abs(T) < _TOL] = 0.
    return T


def shift_over_knot(coeffs, basis):
    return matvec(shiftoverknot_T(basis), coeffs)


def shift_spline_T(basis, t_shift):
    """Matrix of the free-T warm-start shift (`spline_extra.py:88-99`): the piece of the spline on
    [t_shift, 1] re-expressed on a basis with equidistant knots on that interval (same number of
    knots, so the approximation is not exact -- it is an initial guess)."""
    d = basis.degree
    n_knots = len(basis) - d + 1
    knots2 = np.r_[t_shift * np.ones(d), np.linspace(t_shift, basis.knots[-1], n_knots),
                   basis.knots[-1] * np.ones(d)]
    return BSplineBasis(knots2, d).transform(basis)


def shiftfirstknot_T(basis, t_shift, inverse=False):
    """Matrix re-expressing a spline on the basis whose first degree+1 knots sit
    at t_shift (only the future part [t_shift, 1] is described); identity
    outside the leading (d+1)x(d+1) block (`spline_extra.py:220-255`).
    Numeric t_shift only; the per-agent device twin lives in the ADMM kernels."""
    k, d = basis.knots.copy(), basis.degree
    n = len(basis)
    k2 = k.copy()
    k2[:d + 1] = t_shift
    basis2 = BSplineBasis(k2, d)
    x = basis2.fit_points()
    x = x[x >= t_shift]
    T = np.linalg.lstsq(basis2.eval_basis(x), basis.eval_basis(x), rcond=None)[0]
    T[np.abs(T) < _TOL] = 0.
    T[d + 1:, :] = np.eye(n)[d + 1:, :]
    if inverse:
        return T, np.linalg.inv(T)
    return T


def shiftfirstknot_block(basis, t_shift):
    """Leading (d+1)x(d+1) block of `shiftfirstknot_T` for numeric OR polynomial
    (`Poly`, e.g. t/T) t_shift, by the de Boor triangle at u = t_shift on the first
    span: new coefficient i = d_d^{[d-i]}(t_shift), each entry a polynomial in
    t_shift (denominators are knot differences only).  Reference: the `_t` matrix
    chain of `spline_extra.py:220-255`."""
    k, d = basis.knots, basis.degree
    # rows[j] = coefficient vector (over c_0..c_d) of d_j^{[r]}
    one = Poly.const(1.0) if isinstance(t_shift, Poly) else 1.0
    zero = one * 0.0
    rows = [[one if a == j else zero for a in range(d + 1)] for j in range(d + 1)]
    out = [None] * (d + 1)
    out[d] = rows[d]
    for r in range(1, d + 1):
        new = [None] * (d + 1)
        for j in range(r, d + 1):
            den = k[j + d - r + 1] - k[j]
            alpha = (t_shift - k[j]) * (1.0 / den)
            new[j] = [(one - alpha) * rows[j - 1][a] + alpha * rows[j][a] for a in range(d + 1)]
        rows = new
        out[d - r] = rows[d]
    return out


def shift_knot1_fwd(cfs, basis, t_shift):
    if isinstance(t_shift, Poly):
        d = basis.degree
        blk = shiftfirstknot_block(basis, t_shift)
        cfs = np.asarray(cfs, dtype=object)
        out = cfs.copy()
        for i in range(d + 1):
            acc = Poly()
            for a in range(d + 1):
                acc = acc + blk[i][a] * cfs[a]
            out[i] = acc
        return out
    return matvec(shiftfirstknot_T(basis, t_shift), cfs)


def shift_knot1_bwd(cfs, basis, t_shift):
    return matvec(shiftfirstknot_T(basis, t_shift, inverse=True)[1], cfs)


def knot_insertion_T(basis, knots_to_insert):
    new_knots = np.sort(np.r_[basis.knots, knots_to_insert])
    basis2 = BSplineBasis(new_knots, basis.degree)
    return basis2.transform(basis), new_knots.tolist()


def crop_spline(spline, min_value, max_value):
    """Piece of the spline on [min_value, max_value] as a clamped spline."""
    k, d = spline.basis.knots, spline.basis.degree
    ins = [min_value] * (d + 1 - int(np.sum(k == min_value))) + \
          [max_value] * (d + 1 - int(np.sum(k == max_value)))
    T, knots2 = knot_insertion_T(spline.basis, ins)
    knots2 = np.asarray(knots2)
    jmin = np.searchsorted(knots2, min_value, side='left')
    jmax = np.searchsorted(knots2, max_value, side='right')
    return BSpline(BSplineBasis(knots2[jmin:jmax], d),
                   matvec(T[jmin:jmax - d - 1, :], spline.coeffs))


def concat_splines(segments, segment_times, n_insert=None):
    """Join per-segment splines (each on [0,1]) into splines on real time.
    Single-segment problems (all FixedT point-to-point problems) reduce to a
    rescale of the knot vector (`spline_extra.py:308-404`)."""
    if len(segments) != 1:
        raise NotImplementedError('multi-segment concatenation is out of the '
                                  'hot-path scope (SURVEY.md §8)')
    return [s.scale(segment_times[0]) for s in segments[0]]


def sample_splines(splines, time):
    """Host sampling helper (`spline_extra.py:406-410`); the batched device twin
    is `omgx_batch_sample`."""
    time = np.asarray(time, dtype=float)
    return [matvec(s.basis.eval_basis(time), s.coeffs) for s in splines]


def first_span_power_series(knots, degree):
    """M [(degree + 1) x (degree + 1)]: B_i(u) = sum_k M[i, k] u^k on the first knot span of a clamped basis (the only functions that
    do not vanish there are the first degree + 1), by interpolation at degree + 1 points of the span -- exact: they are polynomials
    of that degree.  Used where a spline is evaluated at a point that depends on a variable (omgx_shim, free end time)."""
    knots = np.asarray(knots, float)
    basis = BSplineBasis(knots, degree)
    inner = knots[knots > knots[0]]
    width = float(inner[0] - knots[0])
    u = knots[0] + width * (np.arange(degree + 1) + 0.5) / (degree + 1)
    V = np.vander(u - knots[0], degree + 1, increasing=True)                 # V[j, k] = u_j^k
    B = np.asarray(basis.eval_basis(u))[:, :degree + 1]                       # B[j, i] = B_i(u_j)
    M = np.linalg.solve(V, B).T                                               # B_i(u) = sum_k M[i, k] (u - knots[0])^k
    M[np.abs(M) < 1e-12 * np.abs(M).max()] = 0.0
    return M
