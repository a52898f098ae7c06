"""Cost of the callback-evaluation kernel (``sa_k_eval``) of a ``mathfn_*`` problem: N points through ``eval_callbacks``.

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/profile_eval_callbacks.py mathfn_c [log2 N = 20] [repeats = 5]
    python tools/rocpd_summary.py <dir>/.../*_results.db

``mathfn_a`` (exp / log / log1p / expm1 / pow) is the yardstick the inverse / erf problems ``mathfn_c`` (asin / acos /
atan / atan2), ``mathfn_d`` (asinh / acosh / atanh / erf / erfc) and the gamma-family problem ``mathfn_e`` (loggamma /
gamma / digamma / trigamma) and the Bessel problem ``mathfn_f`` (J / Y / I / K of integer order) are compared with: five outputs of one or two
function calls each, plus their derivatives in the four other callbacks.  Arguments are drawn inside the domains (the
main paths are branch-free: their cost does not depend on the interval).  Prints the host-side wall time per call (it
includes the copies of 26 N doubles each way; the kernel time is the profiler's) and the registers / spill slots /
scratch of the code object's kernels.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from sunode_amd import _native
    from sunode_amd.solver import Solver
    from tools.kstat import kernel_stats
    from tools.problem_cache import make_problem
    name = sys.argv[1]
    N = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    prob = make_problem(name)
    path = _native.build_code_object(prob.native_source())
    print("%s: %s" % (name, os.path.basename(path)))
    print("%-14s %5s %5s %5s %6s %6s %8s %6s" % ("kernel", "vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds"))
    for row in kernel_stats(path):
        print("%-14s %5s %5s %5s %6s %6s %8s %6s" % row)
    rng = np.random.RandomState(1)
    if name == "mathfn_a":
        y = np.exp(rng.uniform(-6, 4, (N, 5)))
        par = np.exp(rng.uniform(-3, 2, (N, 5)))
    else:
        y = rng.uniform(0.05, 0.9, (N, 5))
        par = rng.uniform(1.02, 1.1, (N, 5))
        if name == "mathfn_d":
            y[:, 3:] = rng.uniform(0.05, 20.0, (N, 2))         # erf / erfc: all pieces
        if name == "mathfn_e":
            y = rng.uniform(0.05, 20.0, (N, 5))                 # all pieces of the positive axis (no reflection)
        if name == "mathfn_f":
            y = rng.uniform(0.05, 40.0, (N, 5))                 # every piece of J, Y, I, K up to 40 (I_2: the downward recurrence)
    lam, t = rng.randn(N, 5), rng.uniform(0, 50, N)
    eng = Solver(prob)._engine()
    for k in range(repeats + 1):                               # (the first call loads the code object)
        t0 = time.perf_counter()
        got = eng.eval_callbacks(t, y, lam, par, np.zeros((N, 0)))
        wall = time.perf_counter() - t0
        if k:
            print("call %d: %.1f ms wall for %d points, return codes != 0: %d" % (k, 1e3 * wall, N, int((got["codes"] != 0).sum())))


if __name__ == "__main__":
    main()
