"""Cost of per-instance output grids: Lotka-Volterra forward + adjoint at B = 65 536 (bench.py's LV problem and
tolerances), the shared grid (sa_solve_*_batch, the plain kernels) against distinct per-instance start times and
grids of the same length (sa_solve_*_batch_times, the *_t kernels), alternating, best of `reps`; and the shared grid
given as B equal rows, which isolates what the per-instance kernels cost from what distinct grids cost (lanes of a
wavefront reaching their interval ends at different times).

python tools/bench_time_grids.py [B] [reps]       (prints one JSON line)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.problem_cache import make_problem  # noqa: E402
from tools.problems import lv_batch  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    from sunode_amd.solver import AdjointSolver
    prob = make_problem("lv")
    d = lv_batch(B)
    ps = d["params"][:, prob.params_subset.subset_index]
    pr = d["params"][:, prob.params_subset.remainder_index]
    tv = d["tvals"]
    n_t = len(tv)
    rng = np.random.default_rng(1)
    t0s = rng.uniform(0.0, 0.5, B)                          # distinct rows over the same span as the shared grid
    tvs = np.sort(t0s[:, None] + rng.uniform(0.0, tv[-1], (B, n_t)), axis=1)
    tol = 1e-8
    sol = AdjointSolver(prob, abstol=tol, reltol=tol, backward_abstol=tol, backward_reltol=tol, quad_abstol=tol,
                        quad_reltol=tol)
    g = np.ones((n_t, 2))
    same = np.tile(tv, (B, 1))                               # the shared grid as B equal rows: the *_t kernels' own cost
    cases = {"shared": (0.0, tv, tv[-1]), "per_instance_equal_rows": (np.zeros(B), same, same[:, -1]),
             "per_instance": (t0s, tvs, tvs[:, -1])}
    best = {k: dict(wall_ms=1e9, kernel_ms=1e9) for k in cases}
    for _ in range(reps + 1):
        for k, (t0, grid, tb) in cases.items():
            t = time.perf_counter()
            _, st, sc = sol.solve_forward_batch(t0, grid, d["y0"], ps, pr)
            _, _, stb, scb = sol.solve_backward_batch(tb, t0, grid, g)
            wall = 1e3 * (time.perf_counter() - t)
            f, b = sol.last_kernel_ms()
            assert (st == 0).all() and (stb == 0).all()
            best[k] = dict(wall_ms=min(best[k]["wall_ms"], wall), kernel_ms=min(best[k]["kernel_ms"], f + b),
                           steps_fwd=int(sc[:, 0].sum()), steps_bwd=int(scb[:, 0].sum()))
    for k in best:
        best[k]["solves_per_s"] = B / (best[k]["wall_ms"] * 1e-3)
    ratio = {k: best[k]["kernel_ms"] / best["shared"]["kernel_ms"] for k in best}
    print(json.dumps(dict(problem="lv", B=B, n_t=n_t, tol=tol, reps=reps, **best, kernel_ratio=ratio)))


if __name__ == "__main__":
    main()
