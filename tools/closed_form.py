"""The model families of the shape sweep (tools/sweep_cases.py) written down BY HAND: right-hand side, Jacobian and
parameter derivative as closed formulas in numpy -- no sympy, no code generator, nothing of the engine or the oracle.

The sweep compares the device with the CPU oracle and both compile the same generated header; this module is the
independent statement of what that header has to compute (tools/problems.py ``make_random_network``, ``make_chain``,
``lv12`` are the definitions; the derivatives below are derived on paper from them).  Three uses:

* ``callbacks(model, t, x, lam, s, K)``: the five callbacks in the project's conventions (``oracle.harness.Oracle.eval``:
  matrices ``M[i, j]``, row = output) -- rhs = f, jac = J, adjoint rhs = -J^T lam, quadrature rhs = (df/dp)^T lam,
  adjoint Jacobian = -J^T (signs: the reference-generated tests/golden/callbacks_sweep.json, asserted by
  tests/test_sweep_truth.py).
* the same formulas on ``mpmath.mpf`` inputs (numpy object arrays): values at 40 digits
  (tools/make_golden_callbacks_closed_form.py).  Every constant is therefore an exact fp64 number and every
  ``/ 2``, ``/ 10``, ``/ (i + 1)`` a division, never a multiplication by a rounded reciprocal.
* the same formulas on ``Terms`` inputs: next to each value the TERM SCALE sum |summand| and the number m of summands
  of the fully expanded sum of products the formula stands for (sums inside numerators expanded, product and quotient
  rules applied term by term and NOT cancelled; a denominator counts as one factor).  A rounding-error bound of an
  fp64 evaluation in any order is proportional to that scale, not to the result.
* ``augmented_rhs(model)``: the ODE with its sensitivity equations, for the truth integration
  (tools/make_golden_truth.py --sweep).
"""
import re

import numpy as np


# --------------------------------------------------------------------------------------------------------------------
# values with their term scale and term count
# --------------------------------------------------------------------------------------------------------------------
class Terms:
    """An array of sums of products: ``val`` (the sums), ``mag`` (sum of the absolute values of the summands) and
    ``cnt`` (number of summands).  + and - concatenate the summands, * multiplies them out, / divides every summand by
    the VALUE of the denominator (one factor), @ is a sum of products.  Constants enter with one summand where they
    are non-zero and none where they are zero (masks, selectors, diagonals: structural zeros)."""
    __array_ufunc__ = None          # (numpy arrays on the left defer to the reflected operators below)

    def __init__(self, val, mag=None, cnt=None):
        self.val = np.asarray(val)
        self.mag = np.abs(self.val) if mag is None else np.asarray(mag)
        self.cnt = np.ones(self.val.shape, np.int64) if cnt is None else np.asarray(cnt, np.int64)

    @staticmethod
    def const(a):
        if isinstance(a, Terms):
            return a
        a = np.asarray(a)
        return Terms(a, np.abs(a), (a != 0).astype(np.int64))

    shape = property(lambda self: self.val.shape)
    T = property(lambda self: Terms(self.val.T, self.mag.T, self.cnt.T))

    def __getitem__(self, idx):
        return Terms(self.val[idx], self.mag[idx], self.cnt[idx])

    def sum(self, axis=None):
        return Terms(self.val.sum(axis=axis), self.mag.sum(axis=axis), self.cnt.sum(axis=axis))

    def __neg__(self):
        return Terms(-self.val, self.mag, self.cnt)

    def __add__(self, o):
        o = Terms.const(o)
        return Terms(self.val + o.val, self.mag + o.mag, self.cnt + o.cnt)
    __radd__ = __add__

    def __sub__(self, o):
        return self + (-Terms.const(o))

    def __rsub__(self, o):
        return Terms.const(o) + (-self)

    def __mul__(self, o):
        o = Terms.const(o)
        return Terms(self.val * o.val, self.mag * o.mag, self.cnt * o.cnt)
    __rmul__ = __mul__

    def __truediv__(self, o):
        d = o.val if isinstance(o, Terms) else np.asarray(o)
        return Terms(self.val / d, self.mag / np.abs(d), self.cnt * np.ones(np.shape(d), np.int64))

    def __rtruediv__(self, o):
        return Terms.const(o) / self

    def __matmul__(self, o):
        o = Terms.const(o)
        return Terms(self.val @ o.val, self.mag @ o.mag, self.cnt @ o.cnt)

    def __rmatmul__(self, o):
        return Terms.const(o) @ self


def _diag(v):
    if isinstance(v, Terms):
        return Terms(np.diag(v.val), np.diag(v.mag), np.diag(v.cnt))
    return np.diag(v)


def _one(x):
    """1 in the arithmetic of ``x``: constants such as 1 / 10 must be formed there, not in fp64."""
    if isinstance(x, Terms) or x.dtype != object:
        return 1.0
    return type(x.flat[0])(1)


def _stack(rows, like):
    """2-d array of the scalars ``rows[i][j]`` (numbers, mpf or 0-d Terms) in the arithmetic of ``like``."""
    if isinstance(like, Terms):
        rows = [[Terms.const(e) for e in row] for row in rows]
        return Terms(*[_stack([[getattr(e, part)[()] for e in row] for row in rows], getattr(like, part))
                       for part in ("val", "mag", "cnt")])
    out = np.empty((len(rows), len(rows[0])), dtype=object)
    for i, row in enumerate(rows):
        for j, e in enumerate(row):
            out[i, j] = e
    return out if like.dtype == object else out.astype(like.dtype)


# --------------------------------------------------------------------------------------------------------------------
# random_network(n, p, band):  x_i' = sum_j K_ij x_j - A_i x_i sum_j K_ji - B_i x_i T / (C + T) + D_i,  T = sum_j x_j
#   A_i = sum of the s_k with k = i (mod n), 1 if there is none;  B_i = s_{(i+1) mod p} / 2;  C = 1 + s_{2 mod p};
#   D_i = s_{(3i+1) mod p} / 10;  band > 0: only the entries |i - j| <= band of K take part (inflow and column sum)
# --------------------------------------------------------------------------------------------------------------------
class RandomNetwork:
    def __init__(self, n, p, band=0):
        self.n, self.p, self.band = n, p, band
        i = np.arange(n)
        self.mask = (np.abs(i[:, None] - i[None, :]) <= band).astype(float) if band > 0 else np.ones((n, n))
        self.sel_a = (np.arange(p)[None, :] % n == i[:, None]).astype(float)          # [i, k]: s_k enters A_i
        self.no_a = (self.sel_a.sum(axis=1) == 0).astype(float)                       # A_i = 1
        self.idx_b, self.idx_c, self.idx_d = (i + 1) % p, 2 % p, (3 * i + 1) % p
        self.sel_b = (np.arange(p)[None, :] == self.idx_b[:, None]).astype(float)
        self.sel_d = (np.arange(p)[None, :] == self.idx_d[:, None]).astype(float)
        self.e_c = (np.arange(p) == self.idx_c).astype(float)

    def split(self, par):
        """(s, K) of a parameter vector in declaration order: K (n x n, row-major), then s."""
        n = self.n
        return par[n * n:], par[:n * n].reshape(n, n)

    def _parts(self, x, s, K):
        Km = K * self.mask
        colsum = Km.sum(axis=0)                     # sum_j K_ji
        A = self.sel_a @ s + self.no_a
        B = s[self.idx_b] / 2
        den = 1 + s[self.idx_c] + x.sum()           # C + T
        return Km, colsum, A, B, x.sum(), den

    def f(self, t, x, s, K):
        Km, colsum, A, B, T, den = self._parts(x, s, K)
        return Km @ x - A * x * colsum - B * x * T / den + s[self.idx_d] / 10

    def jac(self, t, x, s, K):
        """J[i, j] = d f_i / d x_j;  d/dx_j [T / (C + T)] = 1 / (C + T) - T / (C + T)^2 (not cancelled)."""
        Km, colsum, A, B, T, den = self._parts(x, s, K)
        dq = 1 / den - T / (den * den)
        ones = np.ones(self.n)
        return Km - _diag(A * colsum + B * T / den) - (B * x * dq)[:, None] * ones[None, :]

    def dfdp(self, t, x, s, K):
        """[i, k] = d f_i / d s_k: through A_i, B_i, C (d/dC [-B x T / (C + T)] = +B x T / (C + T)^2) and D_i."""
        Km, colsum, A, B, T, den = self._parts(x, s, K)
        return (-(self.sel_a * (x * colsum)[:, None]) - self.sel_b * (x * T / den / 2)[:, None]
                + (B * x * T / (den * den))[:, None] * self.e_c[None, :] + self.sel_d * (_one(x) / 10))


# --------------------------------------------------------------------------------------------------------------------
# chain(n):  x_0' = -k0 x_0 + k1;   x_i' = k0 x_{i-1} - (k0 + k1 / (i + 1)) x_i
# --------------------------------------------------------------------------------------------------------------------
class Chain:
    def __init__(self, n):
        self.n, self.p = n, 2
        self.shift = np.eye(n, k=-1)                # (shift @ x)_i = x_{i-1}
        self.ip1 = np.arange(1.0, n + 1)
        self.tail = (np.arange(n) > 0).astype(float)
        self.e0 = (np.arange(n) == 0).astype(float)

    def split(self, par):
        return par, None

    def f(self, t, x, s, K=None):
        rate = s[0] + self.tail * s[1] / self.ip1
        return (self.shift @ x) * s[0] - rate * x + self.e0 * s[1]

    def jac(self, t, x, s, K=None):
        rate = s[0] + self.tail * s[1] / self.ip1
        return self.shift * s[0] - _diag(rate)

    def dfdp(self, t, x, s, K=None):
        d0 = self.shift @ x - x
        d1 = self.e0 - x / self.ip1 * self.tail
        return d0[:, None] * np.array([1.0, 0.0])[None, :] + d1[:, None] * np.array([0.0, 1.0])[None, :]


# --------------------------------------------------------------------------------------------------------------------
# lv12:  h' = a0 h - b0 h l + a1 h / (1 + c0 h) - a2 h^2 / 10 + c2 / 10
#        l' = b1 h l - a3 l + b2 l / (1 + c1 l) - b3 l^2 / 10 + c3 / 10          s = (a0..a3, b0..b3, c0..c3)
# --------------------------------------------------------------------------------------------------------------------
class LV12:
    n, p = 2, 12

    def split(self, par):
        return par, None

    def f(self, t, x, s, K=None):
        h, l = x[0], x[1]
        a, b, c = s[0:4], s[4:8], s[8:12]
        fh = a[0] * h - b[0] * h * l + a[1] * h / (1 + c[0] * h) - a[2] * h * h / 10 + c[2] / 10
        fl = b[1] * h * l - a[3] * l + b[2] * l / (1 + c[1] * l) - b[3] * l * l / 10 + c[3] / 10
        return _stack([[fh, fl]], x)[0]

    def jac(self, t, x, s, K=None):
        h, l = x[0], x[1]
        a, b, c = s[0:4], s[4:8], s[8:12]
        dh, dl = 1 + c[0] * h, 1 + c[1] * l
        return _stack([[a[0] - b[0] * l + a[1] / dh - a[1] * h * c[0] / (dh * dh) - 2 * a[2] * h / 10, -b[0] * h],
                       [b[1] * l, b[1] * h - a[3] + b[2] / dl - b[2] * l * c[1] / (dl * dl) - 2 * b[3] * l / 10]], x)

    def dfdp(self, t, x, s, K=None):
        h, l = x[0], x[1]
        a, b, c = s[0:4], s[4:8], s[8:12]
        dh, dl = 1 + c[0] * h, 1 + c[1] * l
        zero, tenth = 0 * h, _one(x) / 10
        row_h = [h, h / dh, -(h * h) / 10, zero, -(h * l), zero, zero, zero, -(a[1] * h * h) / (dh * dh), zero, tenth, zero]
        row_l = [zero, zero, zero, -l, zero, h * l, l / dl, -(l * l) / 10, zero, -(b[2] * l * l) / (dl * dl), zero, tenth]
        return _stack([row_h, row_l], x)


def random_network(n, p, band=0):
    return RandomNetwork(n, p, band)


def chain(n):
    return Chain(n)


def lv12():
    return LV12()


def model_of(name):
    """The closed form of a sweep case (names of tools/problem_cache.py: ``lv12``, ``chain<n>``, ``rn<n>_<p>``,
    ``rnb<n>_<p>`` = band 2)."""
    if name == "lv12":
        return lv12()
    m = re.fullmatch(r"chain(\d+)", name)
    if m:
        return chain(int(m.group(1)))
    m = re.fullmatch(r"rn(b?)(\d+)_(\d+)", name)
    return random_network(int(m.group(2)), int(m.group(3)), band=2 if m.group(1) else 0)


def callbacks(model, t, x, lam, s, K=None):
    """rhs, jac, adj, quad, adjjac -- plain arrays, mpf object arrays or ``Terms``, as the inputs are."""
    f, J, P = model.f(t, x, s, K), model.jac(t, x, s, K), model.dfdp(t, x, s, K)
    return dict(rhs=f, jac=J, adj=-(J.T @ lam), quad=P.T @ lam, adjjac=-J.T)


def callbacks_with_scales(model, t, x, lam, s, K=None):
    """``callbacks`` on ``Terms``: every entry with its term scale and summand count (inputs: one summand each, zeros
    included -- a state that happens to be 0 is still a term of the formula)."""
    lift = lambda a: None if a is None else Terms(a)       # noqa: E731
    return callbacks(model, t, lift(x), lift(lam), lift(s), lift(K))


def augmented_rhs(model):
    """f(t, z, s, K) for z = [y, S (p x n, row = parameter), S0 (n x n, row = initial state)]:
    S' = J S + df/dp, S0' = J S0 (the layout of tools/make_golden_truth.py ``augmented_rhs``).  ``S0`` may hold fewer
    than n rows (a subset of the initial states)."""
    n, p = model.n, model.p

    def rhs(t, z, s, K):
        y = z[:n]
        S = z[n:n + n * p].reshape(p, n)
        S0 = z[n + n * p:].reshape(-1, n)
        J = model.jac(t, y, s, K)
        out = np.empty_like(z)
        out[:n] = model.f(t, y, s, K)
        out[n:n + n * p] = (S @ J.T + model.dfdp(t, y, s, K).T).ravel()
        out[n + n * p:] = (S0 @ J.T).ravel()
        return out
    return rhs
