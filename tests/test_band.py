"""``linear_solver="band"`` without a GPU: the Jacobian's structure, the public interface, the build plumbing, the band LU's
arithmetic and the cross-compiled band code objects.

The band is honoured where the memory-resident mapping runs (csrc/bdf_mem.hip: more than 128 states, SA_FORCE_GROUP=mem,
the sensitivity builds that land there); everywhere else the option keeps its RuntimeWarning and the dense LU.  The device
side is compared with the oracle bit for bit in tests/test_gpu_band.py."""
import math
import pickle
import random
import warnings

import numpy as np
import pytest

from sunode_amd import _native
from tests.helpers import make_problem

KW22 = {"lower_bandwidth": 2, "upper_bandwidth": 2}


# ---------------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, n, want", [("chain16", 16, (1, 0)), ("pivoting", 6, (5, 1)), ("huge_pivots", 6, (5, 1)),
                                           ("rnb12_4", 12, (11, 11)), ("brusselator1d_6", 12, (2, 2)),
                                           ("pivoting_band", 6, (1, 1))])
def test_jacobian_bandwidths(name, n, want):
    prob = make_problem(name)
    assert prob.n_states == n
    assert prob.jacobian_bandwidths() == want


def test_pivoting_band_still_needs_row_exchanges():
    """At the parameters of tests/test_gpu_parity.py::test_row_exchanges_in_the_dense_lu and the gamma of a unit step of
    a first-order BDF (gamma = h = 1) the partial-pivot choice of I - gamma J is off the diagonal."""
    prob = make_problem("pivoting_band")
    params = np.zeros((), dtype=prob.params_dtype)
    params["k"], params["w"] = [0.5, 0.3], [1000.0, 700.0]
    user_data = prob.make_user_data()
    prob.update_params(user_data, params)
    J = np.zeros((6, 6))
    assert prob.make_jac_dense()(J, 0.0, np.array([0.5, 1e-6, 0.0, 1e-6, 2e-6, 0.1]), None, user_data) == 0
    rows, cols = np.nonzero(J)
    assert (int((rows - cols).max()), int((cols - rows).max())) == prob.jacobian_bandwidths() == (1, 1)
    A = np.eye(6) - 1.0 * J
    off_diagonal = 0
    for c in range(6):              # partial pivoting, first maximum wins
        l = c + int(np.argmax(np.abs(A[c:, c])))
        off_diagonal += l != c
        A[[c, l]] = A[[l, c]]
        A[c + 1:, c] /= A[c, c]
        A[c + 1:, c + 1:] -= np.outer(A[c + 1:, c], A[c, c + 1:])
    assert off_diagonal >= 1


# ---------------------------------------------------------------------------------------------------------------
# public interface (the builds themselves are stubbed: these tests are about the arguments)
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def builds(monkeypatch):
    """Record what the solvers ask the build for instead of compiling it."""
    calls = []

    def fake(source, *a, **kw):
        calls.append(kw)
        return "unbuilt.hsaco"
    monkeypatch.setattr(_native, "build_code_object", fake)
    return calls


@pytest.fixture
def mem(monkeypatch):
    monkeypatch.setenv("SA_FORCE_GROUP", "mem")


def test_band_is_honoured_in_the_memory_resident_mapping(mem, builds):
    from sunode_amd.solver import AdjointSolver, Solver
    prob = make_problem("brusselator1d_6")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)          # no warning where the band is honoured
        s = Solver(prob, linear_solver="band", linear_solver_kwargs=KW22)
        a = AdjointSolver(prob, linear_solver="band", linear_solver_kwargs=KW22)
        ss = Solver(prob, sens_mode="simultaneous", linear_solver="band", linear_solver_kwargs=KW22)
    assert [kw.get("band") for kw in builds] == [(2, 2)] * 3
    assert s._engine_kwargs()["band"] == a._engine_kwargs()["band"] == ss._engine_kwargs()["band"] == (2, 2)
    # dense stays dense: no band keyword reaches the build
    builds.clear()
    assert "band" not in Solver(prob)._engine_kwargs() and "band" not in AdjointSolver(prob)._engine_kwargs()
    assert all("band" not in kw for kw in builds)


def test_band_of_a_large_model_is_honoured_without_forcing(monkeypatch, builds):
    from sunode_amd.solver import AdjointSolver
    monkeypatch.delenv("SA_FORCE_GROUP", raising=False)
    prob = make_problem("chain256")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        a = AdjointSolver(prob, linear_solver="band", linear_solver_kwargs={"lower_bandwidth": 1, "upper_bandwidth": 0})
    assert a._engine_kwargs()["band"] == (1, 0) and builds[-1]["band"] == (1, 0)


@pytest.mark.parametrize("cls", ["Solver", "AdjointSolver"])
def test_band_arguments_are_checked(cls, mem, builds):
    import sunode_amd.solver as S
    make = getattr(S, cls)
    prob = make_problem("brusselator1d_6")
    for kwargs in (None, {}, {"lower_bandwidth": 2}, {"upper_bandwidth": 2}):
        with pytest.raises(ValueError, match="Banded solver requires arguments lower_bandwidth and upper_bandwidth"):
            make(prob, linear_solver="band", linear_solver_kwargs=kwargs)
    for ml, mu in ((1, 2), (2, 1), (0, 0)):          # narrower than the structure: both pairs are named
        with pytest.raises(ValueError) as err:
            make(prob, linear_solver="band", linear_solver_kwargs={"lower_bandwidth": ml, "upper_bandwidth": mu})
        assert str((ml, mu)) in str(err.value) and "(2, 2)" in str(err.value)
    assert not builds
    # wider is allowed, widths are clamped to n - 1
    assert make(prob, linear_solver="band",
                linear_solver_kwargs={"lower_bandwidth": 3, "upper_bandwidth": 4})._engine_kwargs()["band"] == (3, 4)
    assert make(prob, linear_solver="band",
                linear_solver_kwargs={"lower_bandwidth": 40, "upper_bandwidth": 11})._engine_kwargs()["band"] == (11, 11)
    with pytest.raises(ValueError, match="Unknown linear solver"):
        make(prob, linear_solver="bands")


def test_band_elsewhere_keeps_its_warning_and_the_dense_lu(monkeypatch, builds):
    """The existing behaviour outside the memory-resident mapping: a RuntimeWarning, dense LU, kwargs not examined."""
    from sunode_amd import SympyProblem
    from sunode_amd.solver import AdjointSolver, Solver
    monkeypatch.delenv("SA_FORCE_GROUP", raising=False)
    one = SympyProblem({"b": ()}, {"x": ()}, lambda t, y, p: {"x": y.x}, derivative_params=[])
    with pytest.warns(RuntimeWarning, match="always uses dense LU"):
        s = Solver(one, linear_solver="band", linear_solver_kwargs={"upper_bandwidth": 1, "lower_bandwidth": 1})
    assert "band" not in s._engine_kwargs()
    prob = make_problem("brusselator1d_6")                    # 12 states: lane groups
    with pytest.warns(RuntimeWarning, match="always uses dense LU"):
        a = AdjointSolver(prob, linear_solver="band")         # (no kwargs needed where the band is not used)
    assert "band" not in a._engine_kwargs()
    with pytest.warns(RuntimeWarning, match="always uses dense LU"):
        Solver(prob, linear_solver="spgmr")
    assert all("band" not in kw for kw in builds)


def test_adjoint_solver_band_fields_pickle(mem, builds):
    from sunode_amd.solver import AdjointSolver, Solver
    prob = make_problem("pivoting_band")
    kw = {"lower_bandwidth": 1, "upper_bandwidth": 3}
    a = pickle.loads(pickle.dumps(AdjointSolver(prob, linear_solver="band", linear_solver_kwargs=kw)))
    assert a._linear_solver_kind == "band" and a._linear_solver_kwargs == kw and a._engine_kwargs()["band"] == (1, 3)
    s = pickle.loads(pickle.dumps(Solver(prob, linear_solver="band", linear_solver_kwargs=kw)))
    assert s._linear_solver_kind == "band" and s._engine_kwargs()["band"] == (1, 3) and builds[-1]["band"] == (1, 3)


# ---------------------------------------------------------------------------------------------------------------
# build plumbing
# ---------------------------------------------------------------------------------------------------------------
def test_cache_keys(mem):
    src = make_problem("brusselator1d_6").native_source()
    old_way = _native.code_object_path(src, False, False, False, False, False, None)     # the signature before band=
    assert _native.code_object_path(src) == _native.code_object_path(src, band=None) == old_way
    exact, wider = _native.code_object_path(src, band=(2, 2)), _native.code_object_path(src, band=(3, 4))
    assert len({old_way, exact, wider}) == 3
    assert _native.code_object_path(src, band=(2, 2), safe=True) not in (exact, _native.code_object_path(src, safe=True))
    assert _native.code_object_path(src, band=(50, 11)) == _native.code_object_path(src, band=(11, 11))     # clamped


def test_band_build_outside_the_memory_resident_mapping_is_an_error(monkeypatch):
    monkeypatch.delenv("SA_FORCE_GROUP", raising=False)
    src = make_problem("brusselator1d_6").native_source()
    with pytest.raises(_native.NativeBuildError, match="band"):
        _native.code_object_path(src, band=(2, 2))


# ---------------------------------------------------------------------------------------------------------------
# the arithmetic: csrc/bdf_mem.hip dense_getrf / dense_getrs and band_getrf / band_getrs, transcribed
# ---------------------------------------------------------------------------------------------------------------
def _fma():
    if hasattr(math, "fma"):
        return math.fma
    try:                                    # the C library's fused multiply-add
        import ctypes
        import ctypes.util
        f = ctypes.CDLL(ctypes.util.find_library("m")).fma
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_double] * 3
        if f(2.0 ** 27 + 1.0, 2.0 ** 27 + 1.0, -2.0 ** 54) == 2.0 ** 28 + 1.0:        # (fused: the low bit survives)
            return f
    except Exception:                       # noqa: BLE001
        pass
    return lambda a, b, c: a * b + c        # the same multiply-add in both forms


FMA = _fma()


def dense_getrf(a, n):
    """a[i][j]; returns (return code, piv, invp)"""
    piv, invp = [0] * n, [0.0] * n
    for k in range(n):
        l, best = k, abs(a[k][k])
        for i in range(k + 1, n):
            v = abs(a[i][k])
            if v > best:
                best, l = v, i
        piv[k] = l
        if a[l][k] == 0.0:
            return k + 1, piv, invp
        if l != k:
            for c in range(n):
                a[l][c], a[k][c] = a[k][c], a[l][c]
        mult = 1.0 / a[k][k]
        invp[k] = mult
        for i in range(k + 1, n):
            a[i][k] *= mult
        for j in range(k + 1, n):
            a_kj = a[k][j]
            if a_kj != 0.0:
                for i in range(k + 1, n):
                    a[i][j] = FMA(-a_kj, a[i][k], a[i][j])
    return 0, piv, invp


def dense_getrs(a, n, piv, invp, b):
    for k in range(n):
        if piv[k] != k:
            b[k], b[piv[k]] = b[piv[k]], b[k]
    for k in range(n - 1):
        bk = b[k]
        for i in range(k + 1, n):
            b[i] = FMA(-a[i][k], bk, b[i])
    for k in range(n - 1, 0, -1):
        bk = b[k] * invp[k]
        b[k] = bk
        for i in range(k):
            b[i] = FMA(-a[i][k], bk, b[i])
    if n > 0:
        b[0] = b[0] * invp[0]


class BandMatrix:
    """Column j holds rows j - ml - mu .. j + ml in 2 ml + mu + 1 slots (the device's BA(m, i, j)); an access outside a
    column's slots, or outside the matrix, is an error."""

    def __init__(self, n, ml, mu):
        self.n, self.ml, self.mu, self.lda = n, ml, mu, 2 * ml + mu + 1
        self.w = [0.0] * (self.lda * n)

    def _at(self, i, j):
        r = i - j + self.ml + self.mu
        assert 0 <= i < self.n and 0 <= j < self.n and 0 <= r < self.lda, (i, j)
        return j * self.lda + r

    def __getitem__(self, ij):
        return self.w[self._at(*ij)]

    def __setitem__(self, ij, x):
        self.w[self._at(*ij)] = x


def band_getrf(a, n, ml, mu):
    smu = ml + mu
    piv, invp = [0] * n, [0.0] * n
    for k in range(n):
        ilast, jlast = min(k + ml, n - 1), min(k + smu, n - 1)
        l, best = k, abs(a[k, k])
        for i in range(k + 1, ilast + 1):
            v = abs(a[i, k])
            if v > best:
                best, l = v, i
        piv[k] = l
        if a[l, k] == 0.0:
            return k + 1, piv, invp
        if l != k:
            for c in range(k, jlast + 1):
                a[l, c], a[k, c] = a[k, c], a[l, c]
        mult = 1.0 / a[k, k]
        invp[k] = mult
        for i in range(k + 1, ilast + 1):
            a[i, k] *= mult
        for j in range(k + 1, jlast + 1):
            a_kj = a[k, j]
            if a_kj != 0.0:
                for i in range(k + 1, ilast + 1):
                    a[i, j] = FMA(-a_kj, a[i, k], a[i, j])
    return 0, piv, invp


def band_getrs(a, n, ml, mu, piv, invp, b):
    smu = ml + mu
    for k in range(n - 1):
        if piv[k] != k:
            b[k], b[piv[k]] = b[piv[k]], b[k]
        bk = b[k]
        for i in range(k + 1, min(k + ml, n - 1) + 1):
            b[i] = FMA(-a[i, k], bk, b[i])
    for k in range(n - 1, 0, -1):
        bk = b[k] * invp[k]
        b[k] = bk
        for i in range(max(0, k - smu), k):
            b[i] = FMA(-a[i, k], bk, b[i])
    if n > 0:
        b[0] = b[0] * invp[0]


def _banded(rng, n, ml, mu, singular_column=None):
    """A banded matrix that needs exchanges: a small diagonal under large sub-diagonals."""
    rows = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            if -mu <= i - j <= ml and j != singular_column:
                rows[i][j] = rng.uniform(-1, 1) * (0.01 if i == j else 1.0 if i < j else 10.0)
    return rows


@pytest.mark.parametrize("n", [1, 2, 3, 7, 12])
@pytest.mark.parametrize("widths", [(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (5, 1), "full"])
def test_band_lu_equals_dense_lu(n, widths):
    ml, mu = (n - 1, n - 1) if widths == "full" else (min(widths[0], n - 1), min(widths[1], n - 1))     # (host clamp)
    rng = random.Random(1000 * n + 10 * ml + mu)
    exchanged = 0
    for trial in range(4):
        singular = None if trial < 3 else rng.randrange(n)
        rows = _banded(rng, n, ml, mu, singular)
        dense = [r[:] for r in rows]
        band = BandMatrix(n, ml, mu)
        for i in range(n):
            for j in range(n):
                if -mu <= i - j <= ml:
                    band[i, j] = rows[i][j]
        rc_d, piv_d, invp_d = dense_getrf(dense, n)
        rc_b, piv_b, invp_b = band_getrf(band, n, ml, mu)
        assert rc_b == rc_d
        if singular is not None:
            assert rc_d == singular + 1 and piv_b[:singular + 1] == piv_d[:singular + 1]
            continue
        assert rc_d == 0 and piv_b == piv_d and invp_b == invp_d
        exchanged += sum(p != k for k, p in enumerate(piv_d))
        for _ in range(3):
            rhs = [rng.uniform(-1, 1) for _ in range(n)]
            xd, xb = rhs[:], rhs[:]
            dense_getrs(dense, n, piv_d, invp_d, xd)
            band_getrs(band, n, ml, mu, piv_b, invp_b, xb)
            assert xb == xd
    if ml >= 1 and n >= 2:
        assert exchanged > 0            # the matrices did need row exchanges


# ---------------------------------------------------------------------------------------------------------------
# the cross-compiled band builds
# ---------------------------------------------------------------------------------------------------------------
def _ws_formula(n, ml, mu, dense_ws):
    """Band storage of csrc/bdf_mem.hip: O_A (2 ml + mu + 1) n for the forward and (2 mu + ml + 1) n for the backward
    problem (widths swapped) in one place -- the larger of the two -- and O_SJ (ml + mu + 1) n, instead of 2 n^2."""
    return dense_ws - 2 * n * n + (2 * max(ml, mu) + min(ml, mu) + 1) * n + (ml + mu + 1) * n


@pytest.mark.parametrize("name, force, band", [("chain256", None, (1, 0)), ("brusselator1d_6", "mem", (2, 2))])
def test_band_code_object_builds_within_the_dense_build_s_scratch(name, force, band, monkeypatch):
    if force:
        monkeypatch.setenv("SA_FORCE_GROUP", force)
    else:
        monkeypatch.delenv("SA_FORCE_GROUP", raising=False)
    src = make_problem(name).native_source()
    assert _native.kernel_variant(src)[0] == "bdf_mem.hip"
    dense, banded = _native.build_code_object(src), _native.build_code_object(src, band=band)
    nd, nb = _native.code_object_notes(dense), _native.code_object_notes(banded)
    assert set(nb) == set(nd) and "sa_k_forward" in nb and "sa_k_backward" in nb
    for kernel in nd:
        assert nb[kernel]["private_segment_fixed_size"] <= nd[kernel]["private_segment_fixed_size"], kernel
    md, mb = _native.code_object_meta(dense), _native.code_object_meta(banded)
    n = md["n_states"]
    assert mb["ws_doubles"] == _ws_formula(n, band[0], band[1], md["ws_doubles"]) < md["ws_doubles"]
    assert {k: v for k, v in mb.items() if k != "ws_doubles"} == {k: v for k, v in md.items() if k != "ws_doubles"}
