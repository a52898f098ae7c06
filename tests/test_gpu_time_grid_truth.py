"""Per-instance times on the device against the oracle's bits and the truth, on models whose right-hand side reads t.

tests/golden/truth_times_<name>.npz (see tests/test_time_grid_truth.py, which holds the oracle to the same fixtures):
``forcing`` (B-spline input, expit(k (t - t_mid))) and ``misc`` (sin t), rows with t0 < 0, t0 ~ 1e3 / 1e5, the first
output time at t0, repeated output times, spans 10^3 apart in one wavefront, tend strictly inside (t0, tvals[b, 0]).
A kernel that passed another instance's time, the shared scalar or t - t0 to the callbacks is wrong here, where the
autonomous models of tests/test_gpu_time_grids.py cannot tell.

Every case asserts the oracle's bits (outputs, statuses, the CMP / CMP_B counters) and the truth bars: the adjoint
path in every mapping (return_all included), forward sensitivities in the lean lane groups of bdf_wave.hip, bdf_mem.hip
and the register kernel, the plain Solver, Hermite interpolation, every scalar / per-instance mix of t0, tend and tvals
(host and device memory) and the tail-instance guards (B not a multiple of a wavefront's instances, B = 1)."""
import numpy as np
import pytest

from tests.helpers import make_oracle, make_problem
from tests.test_gpu_time_grids import CMP, TOL, _adjoint, _assert_same
from tests.test_time_grid_truth import check_adjoint_truth, check_truth, load_truth, oracle_adjoint, oracle_sens

pytestmark = pytest.mark.gpu

GROUPS = [None, "1", "wave4", "wave8", "wave16", "wave", "mem"]


def _force(group, monkeypatch, name, **kw):
    """SA_FORCE_GROUP=group, or skip where kernel_variant refuses the model in that mapping."""
    from sunode_amd import _native
    if group:
        monkeypatch.setenv("SA_FORCE_GROUP", group)
        try:
            _native.kernel_variant(make_problem(name).native_source(), **kw)
        except _native.NativeBuildError as exc:
            pytest.skip(str(exc))


def _run_adjoint(sol, t):
    return _adjoint(sol, t["y0"], t["ps"], t["pr"], t["t0"], t["tvals"], t["grads"], tend=t["tend"])


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["forcing", "misc"])
def test_adjoint_per_instance_times_vs_oracle_and_truth(name, group, golden_dir, monkeypatch):
    from sunode_amd.solver import AdjointSolver
    _force(group, monkeypatch, name)
    t = load_truth(golden_dir, name)
    sol = AdjointSolver(make_problem(name), **TOL)
    got = _run_adjoint(sol, t)
    _assert_same(got, oracle_adjoint(name, t))             # (lamda_all / quad_all included)
    check_adjoint_truth(t, got[0], got[1], got[3], got[4], got[5])
    sol._engine().close()


@pytest.mark.parametrize("name", ["forcing", "misc"])
def test_single_output_time_and_single_instance(name, golden_dir):
    """n_t = 1 rows (one of them with tvals == t0: no forward step, CV_NO_FWD backward) and B = 1 with [1] / [1, n_t]
    arrays: the tail-instance guards with per-instance times."""
    from sunode_amd.solver import AdjointSolver
    sol = AdjointSolver(make_problem(name), **TOL)
    one = load_truth(golden_dir, name, one=True)
    got = _run_adjoint(sol, one)
    _assert_same(got, oracle_adjoint(name, one))
    check_adjoint_truth(one, got[0], got[1], got[3], got[4], got[5])
    t = load_truth(golden_dir, name)
    want = oracle_adjoint(name, t)
    for b in (2, len(t["t0"]) - 1):                      # (row 2: tend inside (t0, tvals[b, 0]))
        tb = {k: (v[b:b + 1] if k not in ("pr",) else v) for k, v in t.items()}
        _assert_same(_run_adjoint(sol, tb), [w[b:b + 1] for w in want])


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ["forcing", "misc"])
def test_plain_solver_per_instance_times(name, group, golden_dir, monkeypatch):
    """Solver.solve_batch (no trajectory) with per-instance t0 / tvals: oracle bits, truth states."""
    from sunode_amd.solver import Solver
    _force(group, monkeypatch, name)
    t = load_truth(golden_dir, name)
    orc = make_oracle(name)
    cfg = orc.config(rtol=1e-8, atol=1e-8)
    y, st, sc = Solver(make_problem(name), abstol=1e-8, reltol=1e-8).solve_batch(t["t0"], t["tvals"], t["y0"],
                                                                                 t["ps"], t["pr"])
    want = [orc.solve(cfg, t["y0"][b:b + 1], t["ps"][b:b + 1], t["pr"], float(t["t0"][b]), t["tvals"][b])
            for b in range(len(t["t0"]))]
    np.testing.assert_array_equal(y, np.concatenate([w[0] for w in want]))
    np.testing.assert_array_equal(st, np.concatenate([w[1] for w in want]))
    np.testing.assert_array_equal(sc[:, CMP[:8]], np.concatenate([w[2] for w in want])[:, CMP[:8]])
    assert (st == 0).all()
    check_truth(t, y=y)


@pytest.mark.parametrize("mode", ["simultaneous", "staggered"])
@pytest.mark.parametrize("name,group,family", [("forcing", None, ("bdf_wave.hip", 4)),
                                               ("forcing", "mem", ("bdf_mem.hip", 1)),
                                               ("misc", None, ("bdf_kernels.hip", 1))])
def test_forward_sensitivities_per_instance_times(name, group, family, mode, golden_dir, monkeypatch):
    """sa_k_sens_t of the three families: lean lane groups (forcing, n p = 24), memory-resident, register kernel."""
    from sunode_amd import _native
    from sunode_amd.solver import Solver, initial_sensitivities
    _force(group, monkeypatch, name, sens=True)
    prob = make_problem(name)
    assert _native.kernel_variant(prob.native_source(), sens=True) == family
    t = load_truth(golden_dir, name)
    sol = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode=mode)
    y, s, st, sc = sol.solve_sens_batch(t["t0"], t["tvals"], t["y0"], t["ps"], t["pr"], initial_sensitivities(prob))
    yo, so, sto, sco = oracle_sens(name, t, mode)
    np.testing.assert_array_equal(st, sto)
    np.testing.assert_array_equal(y, yo)
    np.testing.assert_array_equal(s, so)
    np.testing.assert_array_equal(sc[:, CMP[:8]], sco[:, CMP[:8]])
    assert (st == 0).all()
    check_truth(t, y=y, sens=s)


@pytest.mark.parametrize("mode", ["simultaneous", "staggered"])
def test_lv_sensitivities_with_edge_rows(mode):
    """The register kernel's sa_k_sens_t on LV with rows starting at t0, t0 repeated and repeated output times."""
    from sunode_amd.solver import Solver, initial_sensitivities
    from tests.test_gpu_time_grids import _lv
    prob, y0, ps, pr, t0, tv, _ = _lv(70, n_t=12, seed=9)
    tv[1::5, :2] = t0[1::5, None]
    tv[2::3, 6] = tv[2::3, 5]
    sens0 = initial_sensitivities(prob)
    y, s, st, sc = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode=mode).solve_sens_batch(t0, tv, y0, ps, pr, sens0)
    orc = make_oracle("lv")
    cfg = orc.config(rtol=1e-8, atol=1e-8)
    want = [orc.solve_sens(cfg, y0[b:b + 1], ps[b:b + 1], pr[b:b + 1], sens0[None], float(t0[b]), tv[b], mode=mode)
            for b in range(70)]
    assert (st == 0).all()
    for got, k in ((y, 0), (s, 1), (st, 2)):
        np.testing.assert_array_equal(got, np.concatenate([w[k] for w in want]))


@pytest.mark.parametrize("variant", [None, "8", "16", "wave4", "wave", "mem"])
def test_hermite_per_instance_times(variant, golden_dir, monkeypatch):
    """AdjointSolver(interpolation="hermite") in the families tests/test_gpu_parity.py's Hermite test runs (register,
    lane groups of 4 / 8 / 16, workgroup, memory-resident): oracle (hermite=True) bits and truth."""
    from sunode_amd.solver import AdjointSolver
    _force(variant, monkeypatch, "forcing", hermite=True)
    t = load_truth(golden_dir, "forcing")
    sol = AdjointSolver(make_problem("forcing"), **TOL, interpolation="hermite")
    got = _run_adjoint(sol, t)
    _assert_same(got, oracle_adjoint("forcing", t, hermite=True))
    check_adjoint_truth(t, got[0], got[1], got[3], got[4], got[5])
    sol._engine().close()


# ---- argument forms: scalar / per-instance mixes of t0, tend and tvals --------------------------------------------
def _forms_data(B=37):
    """forcing with one shared start time (before the spline's support), grid (a repeated time in it) and backward end
    (inside (t0, tvals[0])): every argument form describes the same problem."""
    from tools.problems import forcing_batch
    d = forcing_batch(B)
    t0 = -1.3
    row = t0 + np.array([0.4, 0.9, 1.7, 1.7, 3.2, 5.0, 6.5, 8.0, 9.5])
    tend = t0 + 0.2
    grads = 1.0 + 0.5 * np.cos(np.arange(B * len(row) * 3.0)).reshape(B, len(row), 3)
    return d, t0, row, tend, grads


FWD_FORMS = [(a, b) for a in ("s", "p") for b in ("s", "p")]                       # (t0, tvals)
BWD_FORMS = [(a, b, c) for a in ("s", "p") for b in ("s", "p") for c in ("s", "p")]  # (backward t0, tend, tvals)


def _form(v, kind, B):
    if kind == "s":
        return v
    return np.tile(v, (B, 1)) if np.ndim(v) else np.full(B, v)


def test_every_argument_form_equals_the_broadcast_call():
    """t0 / tvals scalar or per instance forward, t0 / tend / tvals backward, in every combination -- a shared-time
    forward followed by a per-instance backward (s_tinit spread from the forward's t0) and the reverse included: each
    equals the fully broadcast [B] / [B, n_t] call bit for bit (stats slot 15 of the backward pass aside)."""
    from sunode_amd.solver import AdjointSolver
    B = 37
    d, t0, row, tend, grads = _forms_data(B)
    sol = AdjointSolver(make_problem("forcing"), **TOL)

    def run(ff, bf):
        y, st, sc = sol.solve_forward_batch(_form(t0, ff[0], B), _form(row, ff[1], B), d["y0"], d["ps"], d["pr"])
        bw = sol.solve_backward_batch(_form(row[-1], bf[0], B), _form(tend, bf[1], B), _form(row, bf[2], B), grads,
                                      return_all=True)
        return [np.array(a) for a in (y, st, sc) + tuple(bw)]

    ref = run(("p", "p"), ("p", "p", "p"))
    assert (ref[1] == 0).all() and (ref[5] == 0).all()
    for ff in FWD_FORMS:
        for bf in BWD_FORMS:
            got = run(ff, bf)
            try:
                _assert_same(got, ref, stats_cols="solo")
                np.testing.assert_array_equal(got[2], ref[2], err_msg="forward stats")
            except AssertionError as exc:
                raise AssertionError("forward %s, backward %s: %s" % (ff, bf, exc)) from None
    t = {"t0": np.full(B, t0), "tvals": np.tile(row, (B, 1)), "tend": np.full(B, tend), "y0": d["y0"], "ps": d["ps"],
         "pr": d["pr"], "grads": grads}
    _assert_same(ref, oracle_adjoint("forcing", t))


_DEVICE_FORMS_SCRIPT = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from sunode_amd import _native
from sunode_amd.solver import AdjointSolver
from tests.helpers import make_problem
from tests.test_gpu_time_grid_truth import BWD_FORMS, FWD_FORMS, _forms_data, _form
from tests.test_gpu_time_grids import TOL

B = 37
prob = make_problem("forcing")
d, t0, row, tend, grads = _forms_data(B)
sol = AdjointSolver(prob, **TOL)
y, st, sc = sol.solve_forward_batch(np.full(B, t0), np.tile(row, (B, 1)), d["y0"], d["ps"], d["pr"])
ref = [np.array(a) for a in (y, st, sc) + tuple(sol.solve_backward_batch(np.full(B, row[-1]), np.full(B, tend),
                                                                          np.tile(row, (B, 1)), grads))]
eng = AdjointSolver(prob, **TOL)._engine()
dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).reshape(-1).cuda()
z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")
n_t, n, p = len(row), prob.n_states, prob.n_params
_, _, _, prx, stride = sol._batch_inputs(d["y0"], d["ps"], d["pr"])     # (the shared remainder: stride 0)
args = lambda v, kind: (dev(_form(v, kind, B)), 1 if kind == "p" else 0)      # (a shared time: one device element)
for ff in FWD_FORMS + [None]:
    for bf in BWD_FORMS:
        yo, sto, sco = z((B, n_t, n)), z(B, torch.int32), z((B, 16), torch.int64)
        if ff is None:                  # the plain entry point: scalar t0, shared grid
            eng.solve(_native.SA_MEM_DEVICE, B, dev(d["y0"]), dev(d["ps"]), dev(prx), stride, t0, dev(row), n_t,
                      yo, sto, sco, adjoint=True)
        else:
            (t0d, t0s), (tvd, tvs) = args(t0, ff[0]), args(row, ff[1])
            eng.solve(_native.SA_MEM_DEVICE, B, dev(d["y0"]), dev(d["ps"]), dev(prx), stride, t0d, tvd, n_t,
                      yo, sto, sco, adjoint=True, t0_stride=t0s, tvals_stride=n_t if tvs else 0)
        (tbd, tbs), (ted, tes), (tvd, tvs) = args(row[-1], bf[0]), args(tend, bf[1]), args(row, bf[2])
        g, lam, stb, scb = z((B, p)), z((B, n)), z(B, torch.int32), z((B, 16), torch.int64)
        eng.solve_backward(_native.SA_MEM_DEVICE, B, dev(d["ps"]), dev(prx), stride, tbd, ted, tvd, n_t,
                           dev(grads), n_t * n, g, lam, stb, scb, t0_stride=tbs, tend_stride=tes,
                           tvals_stride=n_t if tvs else 0)
        eng.synchronize()
        torch.cuda.synchronize()
        for got, k in ((yo, 0), (sto, 1), (sco, 2), (g, 3), (lam, 4), (stb, 5), (scb, 6)):
            got = got.cpu().numpy()
            if k == 6:
                got, want = got[:, :15], ref[k][:, :15]
            else:
                want = ref[k]
            assert np.array_equal(got, want, equal_nan=True), ("forward", ff, "backward", bf, "output", k)
print("DEVICE_FORMS_OK")
"""


def test_device_tensor_argument_forms():
    """The mixed forms through SA_MEM_DEVICE (a shared time as a one-element device tensor, read back and spread on
    the host side), in a fresh process like bench.py."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _DEVICE_FORMS_SCRIPT, root], capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0 and "DEVICE_FORMS_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
