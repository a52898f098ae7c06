"""Generate tests/golden/callbacks_sweep_hp.npz (+ callbacks_sweep_hp_n64.npz): the five callbacks of EVERY shape of
the parity sweep (tools/sweep_cases.py ``ADJOINT_CASES``) from the hand-written closed form (tools/closed_form.py),
evaluated in mpmath at 40 digits and rounded to fp64 -- a high-precision reference of the same operation the generated
header implements, with no sympy and no code generator involved.

Points per shape (``hp_points``; the tests regenerate the inputs from the same repo-owned streams):
  0-2  the points of tests/golden/callbacks_sweep.json (``sweep_points``: positive O(1) inputs)
  3    exact zeros: the sweep's initial-condition pattern (chain: x = e_0; otherwise every third state 0)
  4    mixed magnitudes: states scaled by 10^+6 / 10^-6 alternating
  5    signed states with T = sum x < 0 and every denominator of the family at least 0.5 away from 0

Stored per shape ``<name>/...``:
  rhs, adj, quad                [6, n] / [6, p]   values; ``*_scale`` the term scale sum |summand| of the entry (fp32,
                                                  rounded UP), ``*_m`` its summand count (tools/closed_form.py ``Terms``)
  n <= 64:  jac, jac_scale, jac_m   [6, n, n]     (row = output); the adjoint Jacobian is -jac^T EXACTLY (negation and
                                                  transposition do not round), so it is not stored a second time
  n  > 64:  jac_Mu, jac_MTw, jac_diag, jac_sample, adjjac_...   [3, ...]   the projection form of
                                                  tools/make_golden_callbacks_network.py ``matrix_summary``, at the
                                                  points 0-2 only (projections cancel at the edge points)
The full matrices of the two 64-state shapes go to a second file so that each file stays below 1 MiB.  Data only.

    python tools/make_golden_callbacks_closed_form.py [name ...]     (needs mpmath; a few minutes)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import closed_form as cf  # noqa: E402
from tools.make_golden_callbacks_network import probe_vectors  # noqa: E402
from tools.make_golden_callbacks_sweep import sweep_points  # noqa: E402
from tools.problems import SEED, std_normal  # noqa: E402
from tools.sweep_cases import ADJOINT_CASES  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
DPS = 40
N_HP = 6
FULL_MAX = 64           # full matrices up to this many states, projections beyond
SECOND_FILE = 64        # shapes with this many states keep their full matrices in callbacks_sweep_hp_n64.npz


def n_items_of(model):
    return 12 if isinstance(model, cf.LV12) else 2 if isinstance(model, cf.Chain) else model.n ** 2 + model.p


def denominators(model, x, s):
    """The denominators of the family's formulas at (x, s)."""
    if isinstance(model, cf.RandomNetwork):
        return [1 + s[model.idx_c] + x.sum()]
    if isinstance(model, cf.LV12):
        return [1 + s[8] * x[0], 1 + s[9] * x[1]]
    return []


def hp_points(name):
    """(t, x, lam, par) with 6 rows each: the three sweep points and the three edge points built from them."""
    model = cf.model_of(name)
    n = model.n
    t, y, lam, par = sweep_points(name, n, n_items_of(model))
    stream = 3000 + sum(ord(c) for c in name)
    zeros = y[0].copy()
    if isinstance(model, cf.Chain):
        zeros[:] = 0.0
        zeros[0] = 1.0
    else:
        zeros[::3] = 0.0
    mixed = y[1] * np.where(np.arange(n) % 2 == 0, 1e6, 1e-6)
    s = model.split(par[2])[0]
    for draw in range(64):          # the first draw of the stream with T < 0 and no denominator near 0
        signed = std_normal(SEED, stream + 5, (draw + 1) * n)[draw * n:]
        if signed.sum() < 0 and all(abs(d) >= 0.5 for d in denominators(model, signed, s)):
            break
    else:
        raise AssertionError("no signed draw with T < 0 and |denominator| >= 0.5 for %s" % name)
    x = np.concatenate([y, [zeros, mixed, signed]])
    return np.tile(t, 2), x, np.tile(lam, (2, 1)), np.tile(par, (2, 1))


def _mp(a):
    import mpmath
    if a is None:
        return None
    a = np.asarray(a, float)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mpmath.mpf(float(a[idx]))
    return out


def _f64(a):
    return np.array([float(v) for v in np.asarray(a, dtype=object).ravel()]).reshape(np.shape(a))


def _f32_up(a):
    """fp32 not below the fp64 value (the scale only enters a tolerance: never round it down)."""
    a = np.asarray(a, float)
    b = a.astype(np.float32)
    low = b.astype(float) < a
    b[low] = np.nextafter(b[low], np.float32(np.inf))
    assert (b.astype(float) >= a).all()
    return b


def shape_entry(name):
    """{key: array} of one shape (keys without the ``<name>/`` prefix; ``second`` = keys of the second file)."""
    import mpmath
    mpmath.mp.dps = DPS
    model = cf.model_of(name)
    n = model.n
    t, x, lam, par = hp_points(name)
    out = {k: [] for k in ("rhs", "adj", "quad", "rhs_scale", "adj_scale", "quad_scale", "rhs_m", "adj_m", "quad_m")}
    mats = {k: [] for k in (("jac", "jac_scale", "jac_m") if n <= FULL_MAX else
                            [m + "_" + q for m in ("jac", "adjjac") for q in ("Mu", "MTw", "diag", "sample")])}
    u, w = (_mp(v) for v in probe_vectors(n))
    for k in range(N_HP):
        s, K = model.split(par[k])
        for d in denominators(model, x[k], s):
            assert abs(d) >= 0.5, (name, k, d)
        hp = cf.callbacks(model, mpmath.mpf(float(t[k])), _mp(x[k]), _mp(lam[k]), _mp(s), _mp(K))
        sc = cf.callbacks_with_scales(model, t[k], x[k], lam[k], s, K)
        for key in ("rhs", "adj", "quad"):
            out[key].append(_f64(hp[key]))
            out[key + "_scale"].append(_f32_up(sc[key].mag))
            out[key + "_m"].append(sc[key].cnt.astype(np.int32))
        if n <= FULL_MAX:
            mats["jac"].append(_f64(hp["jac"]))
            mats["jac_scale"].append(_f32_up(sc["jac"].mag))
            mats["jac_m"].append(sc["jac"].cnt.astype(np.int32))
            # (what the tests rely on when they take -jac^T as the adjoint Jacobian's reference)
            assert all(a == -b for a, b in zip(hp["adjjac"].ravel(), hp["jac"].T.ravel()))
        elif k < 3:
            for m in ("jac", "adjjac"):
                M = hp[m]
                mats[m + "_Mu"].append(_f64(M @ u))
                mats[m + "_MTw"].append(_f64(M.T @ w))
                mats[m + "_diag"].append(_f64(np.diag(M)))
                mats[m + "_sample"].append(_f64(M.ravel()[np.arange(0, n * n, 37)]))
    out = {k: np.array(v) for k, v in out.items()}
    mats = {k: np.array(v) for k, v in mats.items()}
    return out, mats


def main():
    names = sys.argv[1:] or [c[0] for c in ADJOINT_CASES]
    files = {"callbacks_sweep_hp.npz": {}, "callbacks_sweep_hp_n64.npz": {}}
    if sys.argv[1:]:                        # regenerate some shapes: keep the others
        for fn in files:
            with np.load(os.path.join(GOLD, fn)) as d:
                files[fn] = {k: d[k] for k in d.files}
    for name in names:
        vec, mats = shape_entry(name)
        second = cf.model_of(name).n == SECOND_FILE
        for k, v in vec.items():
            files["callbacks_sweep_hp.npz"]["%s/%s" % (name, k)] = v
        for k, v in mats.items():
            files["callbacks_sweep_hp_n64.npz" if second else "callbacks_sweep_hp.npz"]["%s/%s" % (name, k)] = v
        print(name, "done", flush=True)
    for fn, d in files.items():
        np.savez_compressed(os.path.join(GOLD, fn), **d)
        print(fn, os.path.getsize(os.path.join(GOLD, fn)), "bytes")


if __name__ == "__main__":
    main()
