"""Every shape of the parity sweep against references that do not come out of the code generator.

tests/test_shape_sweep.py asserts ``array_equal`` between the device and the CPU oracle.  Both compile the same
generated header, so that bar is blind to the mathematics: a wrong sign in an emitted adjoint term, a wrong index in a
lane-family or zero-run loop, a transposed adjoint Jacobian are bit-identical on both sides.  Here the sweep's model
families are restated by hand (tools/closed_form.py: f, J, df/dp as a dozen lines of numpy each) and used twice:

* callbacks: the closed form in mpmath at 40 digits (tests/golden/callbacks_sweep_hp*.npz) at three O(1) points and
  three edge points (exact zeros, mixed magnitudes 10^+-6, signed states with T < 0) per shape, against the host build
  of the generated C and against the DEVICE functions of the engines the sweep runs;
* solutions: DOP853 truth of the closed form with its sensitivity equations (tests/golden/truth_sweep_<name>.npz)
  against the oracle's states, adjoint gradients and forward sensitivities (the device is pinned to the same files in
  tests/test_shape_sweep.py, where it also equals the oracle bit for bit).

The closed form itself is anchored to the reference's symbolic pipeline on the shapes of tests/golden/callbacks_sweep.json.

Callback tolerance (derived, not tuned): an entry that is a sum of m products, each with at most four roundings,
evaluated in fp64 in any order, with or without FMA contraction, differs from the exact value by at most
(m + 4) u sum|terms| (1 + O(u)), u = 2^-53.  The bar is |got - want| <= 2 (m + 4) u sum|terms| per entry; m and
sum|terms| (the scale of the UNCANCELLED sum of products: sums in numerators expanded, product and quotient rules
applied term by term) are part of the fixture.
"""
import os

import numpy as np
import pytest

from tests.helpers import check_matrix_summary, make_oracle, make_problem
from tests.test_shape_sweep import PINNED, _truth_bars
from tools import closed_form as cf
from tools.sweep_cases import ADJOINT_CASES, SENS_CASES, batch_of

NAMES = [c[0] for c in ADJOINT_CASES]
SENS_NAMES = [c[0] for c in SENS_CASES]
U = 2.0 ** -53
KEYS = ("rhs", "jac", "adj", "quad", "adjjac")


# ---- the high-precision callback fixture -----------------------------------------------------------------------------
def hp_fixture(golden_dir, name):
    """{key: array} of one shape from callbacks_sweep_hp.npz (+ the second file that holds the 64-state matrices)."""
    out = {}
    for fn in ("callbacks_sweep_hp.npz", "callbacks_sweep_hp_n64.npz"):
        with np.load(os.path.join(golden_dir, fn)) as d:
            out.update({k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(name + "/")})
    assert "rhs" in out, "no high-precision callbacks for %s" % name
    return out


def hp_inputs(name):
    """(t, x, lam, ps, pr) of the six points, parameters split the way the problem splits them."""
    from tools.make_golden_callbacks_closed_form import hp_points
    prob = make_problem(name)
    t, x, lam, par = hp_points(name)
    assert par.shape[1] == prob.params_subset.n_items
    return t, x, lam, par[:, prob.params_subset.subset_index], par[:, prob.params_subset.remainder_index]


def _within(got, want, scale, m, what):
    got, want = np.asarray(got, float), np.asarray(want, float)
    bound = 2.0 * (np.asarray(m, float) + 4.0) * U * np.asarray(scale, float)
    err = np.abs(got - want)
    bad = ~(err <= bound)               # (a NaN fails)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0.0)), err.shape)
        raise AssertionError("%s: %d entries beyond 2 (m + 4) u sum|terms|; worst at %s: got %r, want %r, |diff| %.3e, "
                             "bound %.3e (m = %d)" % (what, bad.sum(), i, got[i], want[i], err[i], bound[i],
                                                      np.asarray(m)[i]))
    return float(np.max(err / np.where(bound > 0, bound, 1.0))) if err.size else 0.0


def check_callbacks_hp(fix, got_of_point, n, label=""):
    """The five callbacks at the six points against the fixture; returns the largest |diff| / bound met."""
    worst = 0.0
    for k in range(6):
        got = got_of_point(k)
        what = "%s point %d " % (label, k)
        for key in ("rhs", "adj", "quad"):
            worst = max(worst, _within(np.asarray(got[key]).ravel(), fix[key][k], fix[key + "_scale"][k],
                                       fix[key + "_m"][k], what + key))
        J, AJ = np.asarray(got["jac"]).reshape(n, n), np.asarray(got["adjjac"]).reshape(n, n)
        if "jac" in fix:
            worst = max(worst, _within(J, fix["jac"][k], fix["jac_scale"][k], fix["jac_m"][k], what + "jac"))
            # the adjoint Jacobian is -J^T: negation and transposition are exact, so its reference and scales are the
            # Jacobian's, transposed (tools/make_golden_callbacks_closed_form.py asserts this on the mpmath values)
            worst = max(worst, _within(AJ, -fix["jac"][k].T, fix["jac_scale"][k].T, fix["jac_m"][k].T, what + "adjjac"))
        elif k < 3:
            for M, key in ((J, "jac"), (AJ, "adjjac")):
                check_matrix_summary(M, {q: fix["%s_%s" % (key, q)][k] for q in ("Mu", "MTw", "diag", "sample")})
        assert not np.asarray(got["codes"]).any()
    return worst


# ---- 1. the closed form is anchored to the reference's pipeline ---------------------------------------------------------
@pytest.mark.parametrize("name", PINNED)
def test_closed_form_matches_the_reference_pipeline(name, golden_dir):
    """tools/closed_form.py reproduces the reference-generated tests/golden/callbacks_sweep.json (values, signs and
    layout of all five callbacks) at that file's tolerance -- before it is used to judge anything else."""
    from tests.test_shape_sweep import _check_against_reference, pinned_fixture
    from tools.make_golden_callbacks_sweep import sweep_points
    fix = pinned_fixture(name, golden_dir)
    model = cf.model_of(name)
    assert (model.n, model.p) == (fix["n"], fix["p"])
    t, y, lam, par = sweep_points(name, fix["n"], fix["n_items"])

    def point(k):
        s, K = model.split(par[k])
        return dict(cf.callbacks(model, t[k], y[k], lam[k], s, K), codes=[0] * 5)
    _check_against_reference(fix, point)


# ---- 2. fixtures are complete ------------------------------------------------------------------------------------------
def test_sweep_fixtures_are_complete(golden_dir):
    for name in NAMES:
        model = cf.model_of(name)
        n, p = model.n, model.p
        fix = hp_fixture(golden_dir, name)
        for key, width in (("rhs", n), ("adj", n), ("quad", p)):
            for suffix in ("", "_scale", "_m"):
                assert fix[key + suffix].shape == (6, width), (name, key + suffix)
            assert np.isfinite(fix[key]).all() and (fix[key + "_scale"] >= np.abs(fix[key]) * (1 - 1e-6)).all()
        if n <= 64:
            assert fix["jac"].shape == fix["jac_scale"].shape == fix["jac_m"].shape == (6, n, n), name
        else:
            for key in ("jac", "adjjac"):
                assert fix[key + "_Mu"].shape == fix[key + "_MTw"].shape == fix[key + "_diag"].shape == (3, n), name
        d = np.load(os.path.join(golden_dir, "truth_sweep_%s.npz" % name))       # (no exists() escape: a missing file fails)
        ref = batch_of(name, 4)
        for key in ("y0", "ps", "pr", "tvals", "grads"):
            np.testing.assert_array_equal(d[key], ref[key], err_msg="%s %s" % (name, key))
        n_t = len(ref["tvals"])
        assert d["y_out"].shape == (4, n_t, n) and d["grad_params"].shape == (4, p) and d["grad_y0"].shape == (4, n)
        assert np.isfinite(d["y_out"]).all() and np.abs(d["grad_params"]).min() > 0
        if name in SENS_NAMES:
            assert d["sens"].shape == (4, n_t, p, n), name
        if not name.startswith("chain"):
            # _truth_bars divides by the per-state maximum: O(1) states everywhere but in the chain family
            assert np.abs(d["y_out"]).max(axis=(0, 1)).min() >= 1e-3, name


# ---- 3. fixtures are reproducible ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rn6_1", "rnb7_9"])
def test_sweep_fixtures_are_reproducible(name, golden_dir):
    pytest.importorskip("mpmath")
    pytest.importorskip("scipy")
    from tools.make_golden_callbacks_closed_form import shape_entry
    from tools.make_golden_truth_sweep import truth
    fix = hp_fixture(golden_dir, name)
    vec, mats = shape_entry(name)
    assert set(fix) == set(vec) | set(mats)
    for k, v in {**vec, **mats}.items():
        np.testing.assert_array_equal(fix[k], v, err_msg=k)
    d = np.load(os.path.join(golden_dir, "truth_sweep_%s.npz" % name))
    new = truth(name)
    for key in ("y_out", "grad_params", "grad_y0") + (("sens",) if name in SENS_NAMES else ()):
        assert np.max(np.abs(new[key] - d[key])) <= 1e-11 * np.abs(d[key]).max(), key


# ---- 4. two derivations of the same truth ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lv12", "rn12_4"])
def test_closed_form_truth_equals_symbolic_truth(name, golden_dir):
    """The committed truth (closed form) against the same integration driven by the project's SYMBOLIC derivation
    (tools/make_golden_truth.py ``truth_batch``: lambdified ``_sym_dydt_jac`` / ``_sym_dydp``), which is how these
    two files were produced before: two independent derivations, both 1e-13 integrations."""
    pytest.importorskip("scipy")
    from tools.make_golden_truth import truth_batch
    d = np.load(os.path.join(golden_dir, "truth_sweep_%s.npz" % name))
    y, gp, gy0 = truth_batch(make_problem(name), d["y0"], d["ps"], d["pr"], float(d["t0"]), d["tvals"], d["grads"], "DOP853")
    for got, key in ((y, "y_out"), (gp, "grad_params"), (gy0, "grad_y0")):
        assert np.max(np.abs(got - d[key])) <= 1e-10 * np.abs(d[key]).max(), key


# ---- 5. the generated C against the high-precision closed form ---------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_generated_callbacks_match_closed_form(name, golden_dir):
    """CPU: host build of the generated C (the text the kernels include) at the six points of every shape."""
    fix = hp_fixture(golden_dir, name)
    t, x, lam, ps, pr = hp_inputs(name)
    orc = make_oracle(name)
    worst = check_callbacks_hp(fix, lambda k: orc.eval(t[k], x[k], lam[k], ps[k], pr[k]), orc.n, name)
    print("%s: host build vs closed form, max |diff| / bound = %.3f" % (name, worst))


# ---- 6. the oracle's solutions against the closed-form truth -------------------------------------------------------------------
def truth_case(name, golden_dir):
    """(truth file, tolerance, state floor) of a sweep shape: the sweep's own tolerance (1e-8) except for the chain
    family, whose sweep case runs at rtol 1e-6 (no project bar there) and is asserted at rtol = atol = 1e-8 instead.
    A chain state that never exceeds atol / rtol = 1 is controlled absolutely by the integrator: its error is
    divided by max(per-state maximum, atol / rtol)."""
    d = np.load(os.path.join(golden_dir, "truth_sweep_%s.npz" % name))
    return d, 1e-8, (1.0 if name.startswith("chain") else 0.0)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_gradients_of_every_sweep_shape_match_truth(name, golden_dir):
    d, tol, floor = truth_case(name, golden_dir)
    orc = make_oracle(name)
    cfg = orc.config(rtol=tol, atol=tol, rtolB=tol, atolB=tol, rtolQB=tol, atolQB=tol)
    tv = d["tvals"]
    y, st, _ = orc.solve_forward(cfg, d["y0"], d["ps"], d["pr"], float(d["t0"]), tv, nthreads=4)
    g, lam, stb, _ = orc.solve_backward(cfg, tv[-1], float(d["t0"]), tv, d["grads"], nthreads=4)
    assert (st == 0).all() and (stb == 0).all()
    errs = _truth_bars(y, g, lam, d, state_floor=floor)
    print("%s: oracle vs truth, y %.1e dL/dp %.1e dL/dy0 %.1e" % ((name,) + errs))


@pytest.mark.parametrize("mode", ["simultaneous", "staggered"])
@pytest.mark.parametrize("name", SENS_NAMES)
def test_oracle_sensitivities_of_sweep_shapes_match_truth(name, mode, golden_dir):
    from tests.test_forward_sens import _rel_err
    d = np.load(os.path.join(golden_dir, "truth_sweep_%s.npz" % name))
    orc = make_oracle(name)
    cfg = orc.config(rtol=1e-8, atol=1e-8)
    sens0 = np.zeros((orc.p, orc.n))
    y, s, st, _ = orc.solve_sens(cfg, d["y0"], d["ps"], d["pr"], sens0, float(d["t0"]), d["tvals"], mode=mode, nthreads=4)
    assert (st == 0).all()
    err = _rel_err(s, d["sens"])
    print("%s %s: oracle sensitivities vs truth %.1e" % (name, mode, err))
    assert err < 2e-5
    assert np.max(np.abs(y - d["y_out"]) / np.abs(d["y_out"]).max(axis=(0, 1))) < 1e-5


# ---- 7. the device functions of the sweep's own engines ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_sweep_callbacks_match_closed_form(name, golden_dir):
    """GPU: ``eval_callbacks`` of the engine the sweep runs for this shape (``AdjointSolver(batch_mapping="fixed")``:
    the code object ``tools/build_sweep.py`` pre-compiles, no other build) at the six points -- every family's callback
    staging (lane families, matrix-vector blocks, zero-run loops, hoisted / packed remainder parameters) against a
    high-precision reference of the same operation, and equal to the host build bit for bit."""
    from sunode_amd.solver import AdjointSolver
    fix = hp_fixture(golden_dir, name)
    t, x, lam, ps, pr = hp_inputs(name)
    prob = make_problem(name)
    d = batch_of(name, 4)
    tol = dict(abstol=d["atol"], reltol=d["rtol"], backward_abstol=d["atol"], backward_reltol=d["rtol"],
               quad_abstol=d["atol"], quad_reltol=d["rtol"])
    eng = AdjointSolver(prob, batch_mapping="fixed", **tol)._engine()
    got = eng.eval_callbacks(t, x, lam, ps, np.array([prob.extend_remainder(row) for row in pr]))
    n = prob.n_states
    check_callbacks_hp(fix, lambda k: {key: got[key][k] for key in KEYS + ("codes",)}, n, name)
    orc = make_oracle(name)
    for k in range(len(t)):
        host = orc.eval(t[k], x[k], lam[k], ps[k], pr[k])
        for key in KEYS:
            np.testing.assert_array_equal(np.asarray(got[key][k]).ravel(), np.asarray(host[key]).ravel(),
                                          err_msg="point %d %s" % (k, key))
