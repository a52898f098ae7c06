"""Band against dense in the memory-resident mapping: forward + adjoint solves/s and workspace per instance.

    python tools/bench_band.py [--out profiles/band_lu_ab.txt] [--build-only] [--runs 3] [--leg-timeout 300]

Models: ``chain256`` (1, 0), ``brusselator1d(128)`` (256 states, (2, 2)) and ``chain512`` (1, 0), rtol = atol = 1e-8.  Every
leg (one model, one build, one forward + backward pass) runs in a fresh child process under its own time limit; band and
dense alternate, ``--runs`` times each, in one session.  Throughput is taken from the kernels' own times
(``last_kernel_ms``: module load and allocation excluded); the wall time of the two calls is printed next to it.

The rule of DESIGN 3.1 (SA_INTERP_FAST): the band build counts as faster when its gain over the dense build exceeds three
times the dense build's own run-to-run spread.  A leg that runs into its time limit ends the session (nothing more is
started on the device after it); the report then says so and gives the figures measured until then -- which is why
``chain512``, whose dense leg is the long one, comes last.

``--build-only`` compiles the six code objects and the problems without touching a device (the cache then travels with
the tree)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

#: (model, batch, (ml, mu)): batches of whole wavefronts whose dense workspace stays near 1 GB
CASES = [("chain256", 1024, (1, 0)), ("brusselator1d_128", 1024, (2, 2)), ("chain512", 256, (1, 0))]
TOL = 1e-8


def _batch(name, B):
    from tools.problem_cache import make_problem
    from tools.problems import brusselator1d_batch, chain_batch
    n = make_problem(name).n_states
    return chain_batch(B, n) if name.startswith("chain") else brusselator1d_batch(B, n // 2)


def _solver_kw(band):
    kw = dict(abstol=TOL, reltol=TOL, backward_abstol=TOL, backward_reltol=TOL, quad_abstol=TOL, quad_reltol=TOL)
    if band:
        kw.update(linear_solver="band", linear_solver_kwargs={"lower_bandwidth": band[0], "upper_bandwidth": band[1]})
    return kw


def build_all():
    from sunode_amd import _native
    from tools.problem_cache import make_problem
    for name, _B, band in CASES:
        src = make_problem(name).native_source()
        for b in (None, band):
            t = time.time()
            path = _native.build_code_object(src, band=b)
            print("%s %s: %s, %d workspace doubles per instance (%.0f s)"
                  % (name, "band %s" % (b,) if b else "dense", os.path.basename(path),
                     _native.code_object_meta(path)["ws_doubles"], time.time() - t), flush=True)


def leg(name, B, band):
    """One forward + backward pass; prints one JSON line."""
    import numpy as np
    from sunode_amd import _native
    from sunode_amd.solver import AdjointSolver
    from tools.problem_cache import make_problem
    prob = make_problem(name)
    d = _batch(name, B)
    sol = AdjointSolver(prob, **_solver_kw(band))
    tv = d["tvals"]
    t = time.time()
    y, st, sc = sol.solve_forward_batch(d["t0"], tv, d["y0"], d["ps"], d["pr"])
    g, lam, stb, scb = sol.solve_backward_batch(tv[-1], d["t0"], tv, d["grads"])
    wall = time.time() - t
    fwd_ms, bwd_ms = sol.last_kernel_ms()
    assert (st == 0).all() and (stb == 0).all()
    print(json.dumps(dict(name=name, B=B, band=band, wall_s=wall, fwd_ms=fwd_ms, bwd_ms=bwd_ms,
                          ws_doubles=_native.code_object_meta(sol._engine().code_object)["ws_doubles"],
                          nst=float(sc[:, 0].mean()), nsetups=float(sc[:, 2].mean() + scb[:, 2].mean()),
                          checksum=float(np.abs(g).sum()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_lu_ab.txt"))
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=300.0)
    ap.add_argument("--leg", nargs=4, metavar=("MODEL", "BATCH", "ML", "MU"), help="(internal) run one leg; ML < 0: dense")
    a = ap.parse_args()
    if a.leg:
        name, B, ml, mu = a.leg[0], int(a.leg[1]), int(a.leg[2]), int(a.leg[3])
        leg(name, B, (ml, mu) if ml >= 0 else None)
        return 0
    build_all()
    if a.build_only:
        return 0
    env = dict(os.environ, SA_GUARD="0")          # the comparison is between the two builds named here
    env.pop("SA_FORCE_GROUP", None)
    lines, rows, stopped = [], {}, None
    for name, B, band in CASES:
        for run in range(a.runs):
            for b in (band, None):
                key = (name, "band" if b else "dense")
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, str(B)] + [str(w) for w in (b or (-1, -1))]
                try:
                    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.leg_timeout)
                except subprocess.TimeoutExpired:
                    stopped = "%s %s, run %d: not finished within %.0f s at B = %d" % (name, key[1], run + 1, a.leg_timeout, B)
                    break
                if res.returncode != 0:
                    stopped = "%s %s, run %d: exit status %d\n%s" % (name, key[1], run + 1, res.returncode, res.stderr[-2000:])
                    break
                row = json.loads(res.stdout.strip().splitlines()[-1])
                rows.setdefault(key, []).append(row)
                print(row, flush=True)
            if stopped:
                break
        if stopped:
            break
    from sunode_amd import _native
    lines.append("band LU against dense LU, memory-resident mapping (csrc/bdf_mem.hip), forward + adjoint, rtol = atol = %g" % TOL)
    lines.append("toolchain %s; every leg a fresh process, band / dense alternating, %d runs each" % (_native.toolchain_id()["hash"], a.runs))
    lines.append("solves/s = B / (forward kernel + backward kernel time); wall = both calls, transfers included")
    lines.append("")
    for name, B, band in CASES:
        per = {}
        for kind in ("band", "dense"):
            rr = rows.get((name, kind), [])
            if not rr:
                continue
            rate = [r["B"] / ((r["fwd_ms"] + r["bwd_ms"]) * 1e-3) for r in rr]
            per[kind] = rate
            lines.append("%-18s B=%-5d %-14s solves/s %s  wall s %s  workspace %d B/instance  (steps %.0f, set-ups %.0f)"
                         % (name, B, "band %s" % (tuple(band),) if kind == "band" else "dense",
                            " ".join("%9.1f" % x for x in rate), " ".join("%6.2f" % r["wall_s"] for r in rr),
                            8 * rr[0]["ws_doubles"], rr[0]["nst"], rr[0]["nsetups"]))
        if "band" in per and "dense" in per:
            mean = lambda v: sum(v) / len(v)        # noqa: E731
            spread = (max(per["dense"]) - min(per["dense"])) / mean(per["dense"])
            ratio = mean(per["band"]) / mean(per["dense"])
            ck = {r["checksum"] for k in ("band", "dense") for r in rows[(name, k)]}
            lines.append("%-18s band / dense = %.2fx; dense run-to-run spread %.2f %%; gain %s 3 x spread; gradient checksums %s"
                         % (name, ratio, 100 * spread, ">" if ratio - 1 > 3 * spread else "NOT >",
                            "identical" if len(ck) == 1 else "DIFFER %s" % sorted(ck)))
        lines.append("")
    if stopped:
        lines.append("session ended early: " + stopped)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text)
    return 1 if stopped and "exit status" in stopped else 0


if __name__ == "__main__":
    sys.exit(main())
