"""Per-instance start times and output grids of the batch API (t0 / tend [B], tvals [B, n_t]).

The contract: every instance's outputs are bit for bit those of a shared-grid call on that instance alone with its own
t0 / tvals, hence those of the CPU oracle called per instance -- in every mapping, with resident and tiled arenas and
over several handles."""
import numpy as np
import pytest

from tests.helpers import make_oracle, make_problem
from tools.problems import lv_batch, robertson5_batch

pytestmark = pytest.mark.gpu

CMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]            # as tests/test_gpu_parity.py
CMP_B = [0, 1, 2, 3, 4, 5, 6, 9, 10, 12]
TOL = dict(abstol=1e-8, reltol=1e-8, backward_abstol=1e-8, backward_reltol=1e-8, quad_abstol=1e-8, quad_reltol=1e-8)


def _lv(B, n_t=20, seed=3):
    prob = make_problem("lv")
    d = lv_batch(B)
    ps = d["params"][:, prob.params_subset.subset_index]
    pr = d["params"][:, prob.params_subset.remainder_index]
    rng = np.random.default_rng(seed)
    t0 = rng.uniform(0.0, 1.0, B)
    tv = np.sort(t0[:, None] + rng.uniform(0.0, 10.0, (B, n_t)), axis=1)
    tv[::7, 0] = t0[::7]                                   # some rows start exactly at t0
    grads = 1.0 + 0.5 * np.cos(rng.uniform(0, 6, (B, n_t, prob.n_states)))
    return prob, d["y0"], ps, pr, t0, tv, grads


def _r5(B, n_t=6, seed=5):
    prob = make_problem("robertson5")
    d = robertson5_batch(B)
    rng = np.random.default_rng(seed)
    t0 = rng.uniform(0.0, 0.5, B)
    tv = np.sort(t0[:, None] + 10.0 ** rng.uniform(-2, 3, (B, n_t)), axis=1)
    grads = 1.0 + 0.5 * np.sin(rng.uniform(0, 6, (B, n_t, prob.n_states)))
    return prob, d, t0, tv, grads


def _oracle_adjoint(name, y0, ps, pr, t0, tv, grads, tend=None):
    """The oracle instance by instance, each with its own times: y, status, stats, g, lam, status_b, stats_b, la, qa."""
    orc = make_oracle(name)
    cfg = orc.config(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
    rows = []
    for b in range(len(y0)):
        prb = pr[b:b + 1] if pr.ndim == 2 else pr
        y, st, sc = orc.solve_forward(cfg, y0[b:b + 1], ps[b:b + 1], prb, float(t0[b]), tv[b])
        g, lam, stb, scb, la, qa = orc.solve_backward(cfg, tv[b][-1], float(t0[b] if tend is None else tend[b]),
                                                      tv[b], grads[b:b + 1], return_all=True)
        rows.append((y, st, sc, g, lam, stb, scb, la, qa))
    return [np.concatenate(c) for c in zip(*rows)]


def _adjoint(sol, y0, ps, pr, t0, tv, grads, tend=None):
    y, st, sc = sol.solve_forward_batch(t0, tv, y0, ps, pr)
    tb = tv[:, -1] if tv.ndim == 2 else tv[-1]
    g, lam, stb, scb, la, qa = sol.solve_backward_batch(tb, t0 if tend is None else tend, tv, grads, return_all=True)
    return [np.array(a) for a in (y, st, sc, g, lam, stb, scb, la, qa)]


def _assert_same(a, b, stats_cols=True):
    """stats_cols: True -- the counters the oracle keeps (CMP / CMP_B); "solo" -- the 15 per-instance counters (the
    16th, sa_k_backward's iterations of the whole wavefront, depends on which instances share the wave); False: all."""
    for k, (x, y) in enumerate(zip(a, b)):
        if stats_cols is True and k in (2, 6):
            x, y = x[:, CMP if k == 2 else CMP_B], y[:, CMP if k == 2 else CMP_B]
        elif stats_cols == "solo" and k in (2, 6):
            x, y = x[:, :15], y[:, :15]
        np.testing.assert_array_equal(x, y, err_msg="output %d" % k)


def test_lv_forward_backward_per_instance_vs_oracle():
    from sunode_amd.solver import AdjointSolver
    prob, y0, ps, pr, t0, tv, grads = _lv(300)
    got = _adjoint(AdjointSolver(prob, **TOL), y0, ps, pr, t0, tv, grads)
    assert (got[1] == 0).all() and (got[5] == 0).all()
    _assert_same(got, _oracle_adjoint("lv", y0, ps, pr, t0, tv, grads))


@pytest.mark.parametrize("group", [None, "wave4", "wave16", "wave", "mem"])
def test_every_mapping_per_instance_vs_oracle(group, monkeypatch):
    from sunode_amd.solver import AdjointSolver
    if group:
        monkeypatch.setenv("SA_FORCE_GROUP", group)
    prob, d, t0, tv, grads = _r5(20)
    sol = AdjointSolver(prob, **TOL, max_steps=4096)
    got = _adjoint(sol, d["y0"], d["params"], np.zeros(0), t0, tv, grads)
    assert (got[1] == 0).all() and (got[5] == 0).all()
    _assert_same(got, _oracle_adjoint("robertson5", d["y0"], d["params"], np.zeros(0), t0, tv, grads))


def test_forward_solves_and_sensitivities_vs_oracle():
    from sunode_amd.solver import Solver
    prob, y0, ps, pr, t0, tv, _ = _lv(40)
    orc = make_oracle("lv")
    cfg = orc.config(rtol=1e-8, atol=1e-8)
    y, st, sc = Solver(prob, abstol=1e-8, reltol=1e-8).solve_batch(t0, tv, y0, ps, pr)
    want = [orc.solve(cfg, y0[b:b + 1], ps[b:b + 1], pr[b:b + 1], float(t0[b]), tv[b]) for b in range(40)]
    np.testing.assert_array_equal(y, np.concatenate([w[0] for w in want]))
    np.testing.assert_array_equal(st, np.concatenate([w[1] for w in want]))
    np.testing.assert_array_equal(sc[:, CMP[:8]], np.concatenate([w[2] for w in want])[:, CMP[:8]])
    from sunode_amd.solver import initial_sensitivities
    sens0 = initial_sensitivities(prob)
    for mode in ("simultaneous", "staggered"):
        sol = Solver(prob, abstol=1e-8, reltol=1e-8, sens_mode=mode)
        y, s, st, sc = sol.solve_sens_batch(t0, tv, y0, ps, pr, sens0)
        want = [orc.solve_sens(cfg, y0[b:b + 1], ps[b:b + 1], pr[b:b + 1], sens0[None], float(t0[b]), tv[b],
                               mode=mode) for b in range(40)]
        np.testing.assert_array_equal(y, np.concatenate([w[0] for w in want]))
        np.testing.assert_array_equal(s, np.concatenate([w[1] for w in want]))
        np.testing.assert_array_equal(st, np.concatenate([w[2] for w in want]))


def test_identical_rows_equal_the_shared_call():
    from sunode_amd.solver import AdjointSolver
    prob, y0, ps, pr, _, tv, grads = _lv(130)
    row = tv[1]
    shared = _adjoint(AdjointSolver(prob, **TOL), y0, ps, pr, 0.0, row, grads)
    t0s = np.zeros(130)
    per = _adjoint(AdjointSolver(prob, **TOL), y0, ps, pr, t0s, np.tile(row, (130, 1)), grads)
    _assert_same(per, shared, stats_cols=False)                # all 16 counters too


def test_tiled_arena_and_multi_handle():
    from sunode_amd.solver import AdjointSolver
    prob, y0, ps, pr, t0, tv, grads = _lv(200)
    ref = _adjoint(AdjointSolver(prob, **TOL), y0, ps, pr, t0, tv, grads)
    tiled = AdjointSolver(prob, **TOL, arena_gib=3e-3)          # a few MB: several tiles
    _assert_same(_adjoint(tiled, y0, ps, pr, t0, tv, grads), ref, stats_cols=False)
    assert tiled._engine().arena_info()[1] >= 2
    multi = AdjointSolver(prob, **TOL, devices=[0, 0, 0], interleaved=True)
    _assert_same(_adjoint(multi, y0, ps, pr, t0, tv, grads), ref)      # (wave-level diagnostics follow the lanes' mix)


_TORCH_SCRIPT = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from sunode_amd import _native
from sunode_amd.solver import AdjointSolver
from tests.test_gpu_time_grids import TOL, _adjoint, _lv

prob, y0, ps, pr, t0, tv, grads = _lv(200)
ref = _adjoint(AdjointSolver(prob, **TOL), y0, ps, pr, t0, tv, grads)
eng = AdjointSolver(prob, **TOL)._engine()
dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device="cuda")
B, n_t, n = tv.shape[0], tv.shape[1], prob.n_states
stride = prob.n_remainder_native
prx = np.ascontiguousarray(prob.extend_remainder(pr))
yo, st, sc = z((B, n_t, n)), z(B, torch.int32), z((B, 16), torch.int64)
eng.solve(_native.SA_MEM_DEVICE, B, dev(y0), dev(ps), dev(prx), stride, dev(t0), dev(tv), n_t, yo, st, sc,
          adjoint=True, t0_stride=1, tvals_stride=n_t)
g, lam, stb, scb = z((B, prob.n_params)), z((B, n)), z(B, torch.int32), z((B, 16), torch.int64)
eng.solve_backward(_native.SA_MEM_DEVICE, B, dev(ps), dev(prx), stride, dev(tv[:, -1]), dev(t0), dev(tv), n_t,
                   dev(grads), n_t * n, g, lam, stb, scb, t0_stride=1, tend_stride=1, tvals_stride=n_t)
eng.synchronize()
torch.cuda.synchronize()
for got, k in ((yo, 0), (st, 1), (sc, 2), (g, 3), (lam, 4), (stb, 5), (scb, 6)):
    np.testing.assert_array_equal(got.cpu().numpy(), ref[k])
print("TORCH_TIMES_OK")
"""


def test_device_tensors_equal_host_arrays():
    """t0 / tvals (and every other argument) as device tensors through SA_MEM_DEVICE, in a fresh process like bench.py."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _TORCH_SCRIPT, root], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "TORCH_TIMES_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


def test_guard_verifies_a_per_instance_call(monkeypatch):
    from sunode_amd.solver import AdjointSolver
    monkeypatch.setenv("SA_GUARD", "1")
    prob, y0, ps, pr, t0, tv, grads = _lv(150)
    sol = AdjointSolver(prob, **TOL)
    got = _adjoint(sol, y0, ps, pr, t0, tv, grads)
    rep = sol._engine().guard_state()
    assert "adjoint" in rep["verified"] and not rep["differs"], rep
    monkeypatch.setenv("SA_GUARD", "0")
    _assert_same(got, _adjoint(AdjointSolver(prob, **TOL), y0, ps, pr, t0, tv, grads), stats_cols=False)


def test_a_bad_row_fails_alone():
    from sunode_amd.solver import AdjointSolver
    prob, y0, ps, pr, t0, tv, grads = _lv(70)
    bad = tv.copy()
    bad[5, 0] = np.nextafter(t0[5], np.inf)                # first output time one ulp after t0: CV_TOO_CLOSE
    bad[6] = bad[6][::-1]                                  # decreasing (the engine interpolates back, as for a shared grid)
    tend = t0.copy()
    tend[9] = t0[9] - 5.0                                  # backward end outside the forward range
    got = _adjoint(AdjointSolver(prob, **TOL), y0, ps, pr, t0, bad, grads, tend=tend)
    for b in (5, 6, 9):
        solo = _adjoint(AdjointSolver(prob, **TOL), y0[b:b + 1], ps[b:b + 1], pr[b:b + 1], float(t0[b]), bad[b],
                        grads[b:b + 1], tend=float(tend[b]))
        _assert_same([a[b:b + 1] for a in got], solo, stats_cols="solo")
    assert got[1][5] == -27 and got[5][5] != 0              # the forward pass refuses row 5 (CV_TOO_CLOSE) ...
    assert got[1][9] == 0 and got[5][9] != 0               # ... the backward pass instance 9's end time
    ok = np.setdiff1d(np.arange(70), [5, 6, 9])
    ref = _adjoint(AdjointSolver(prob, **TOL), y0[ok], ps[ok], pr[ok], t0[ok], tv[ok], grads[ok])
    _assert_same([a[ok] for a in got], ref, stats_cols="solo")
