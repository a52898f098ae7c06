"""Generate tests/golden/truth_sweep_<name>.npz for EVERY shape of the parity sweep (tools/sweep_cases.py) from the
hand-written closed form (tools/closed_form.py) -- not from the project's symbolic derivation, which is what the code
generator under test consumes.

For the first 4 draws of ``batch_of(name, B)``: DOP853 at rtol 1e-13 / atol 1e-15 of the ODE augmented with
S' = J S + df/dp (S(0) = 0) and S0' = J S0 (S0(0) = I), giving y(t_k) and the exact gradients of
L = sum_k g_k . y(t_k) -- the format ``_truth_bars`` of tests/test_shape_sweep.py reads (y0, ps, pr, t0, tvals, grads,
y_out, grad_params, grad_y0).  The shapes of ``SENS_CASES`` also get ``sens`` [4, n_t, p, n] (layout of
tests/golden/truth_sens_*.npz).  ``chain<n>`` runs in the sweep at rtol 1e-6, where the project has no truth bar: its
truth is on the sweep's grid and is asserted at rtol = atol = 1e-8 by a dedicated case.

    python tools/make_golden_truth_sweep.py [name ...]      (= python tools/make_golden_truth.py --sweep; needs scipy)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import closed_form as cf  # noqa: E402
from tools.sweep_cases import ADJOINT_CASES, SENS_CASES, batch_of  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
N_DRAWS = 4
NOTE = ("truth of tools/closed_form.py (hand-written f, J, df/dp), DOP853 rtol 1e-13 atol 1e-15, "
        "first %d draws of tools/sweep_cases.py batch_of(name, B)" % N_DRAWS)


def truth(name, draws=N_DRAWS, rtol=1e-13, atol=1e-15):
    """The arrays of truth_sweep_<name>.npz."""
    from scipy.integrate import solve_ivp
    model = cf.model_of(name)
    n, p = model.n, model.p
    d = batch_of(name, draws)
    K = d["pr"].reshape(n, n) if d["pr"].size else None
    tv = d["tvals"]
    rhs = cf.augmented_rhs(model)
    y_out = np.zeros((draws, len(tv), n))
    sens = np.zeros((draws, len(tv), p, n))
    grad_p = np.zeros((draws, p))
    grad_y0 = np.zeros((draws, n))
    for b in range(draws):
        z0 = np.concatenate([d["y0"][b], np.zeros(n * p), np.eye(n).ravel()])
        sol = solve_ivp(rhs, (d["t0"], tv[-1]), z0, method="DOP853", t_eval=tv, args=(d["ps"][b], K), rtol=rtol, atol=atol)
        assert sol.success, sol.message
        z = sol.y.T
        y_out[b] = z[:, :n]
        sens[b] = z[:, n:n + n * p].reshape(len(tv), p, n)
        S0 = z[:, n + n * p:].reshape(len(tv), n, n)            # [k, j (y0 index), i (state)]
        grad_p[b] = np.einsum("ki,kpi->p", d["grads"][b], sens[b])
        grad_y0[b] = np.einsum("ki,kji->j", d["grads"][b], S0)
    out = dict(y0=d["y0"], ps=d["ps"], pr=d["pr"], t0=d["t0"], tvals=tv, grads=d["grads"], y_out=y_out,
               grad_params=grad_p, grad_y0=grad_y0, note=np.array(NOTE))
    if name in [c[0] for c in SENS_CASES]:
        out["sens"] = sens
    return out


def _one(name, gold=GOLD):
    out = truth(name)
    np.savez(os.path.join(gold, "truth_sweep_%s.npz" % name), **out)
    return name


def main(names=None, gold=GOLD):
    from concurrent.futures import ProcessPoolExecutor
    names = names or [c[0] for c in ADJOINT_CASES]
    with ProcessPoolExecutor(max_workers=max(1, min(8, (os.cpu_count() or 2) - 1))) as pool:
        for name in pool.map(_one, names, [gold] * len(names)):
            print("truth_sweep_%s.npz" % name, flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or None)
