"""bench.py's bookkeeping that needs no GPU: the committed counter profile is only used when it describes the build,
batch and record format of the run at hand, the truth-gradient error of the timed batch's first draws,
the number of timed steps, what --dump-outputs writes, and that a plain run measures the headline figure alone
(everything else behind --full)."""
import json
import os

import numpy as np
import pytest


def test_counter_profile_is_withheld_when_it_describes_another_build(monkeypatch):
    import bench
    ctx = {"batch": 65536, "record_bytes": 160, "code_object": "abc", "toolchain": "t1"}
    monkeypatch.setattr(bench, "pmc_profile", lambda w, k: ctx if k == "context" else {"fetch": 1.0, "write": 2.0})
    build = {"code_object": "abc", "toolchain": {"hash": "t1"}}
    assert bench.pmc_context_matches("lv", 65536, 160, build)[0]
    for kw, what in ((dict(B=4096), "batch"), (dict(rec=32), "record_bytes"),
                     (dict(build={"code_object": "zzz", "toolchain": {"hash": "t1"}}), "code_object"),
                     (dict(build={"code_object": "abc", "toolchain": {"hash": "t2"}}), "toolchain")):
        args = dict(B=65536, rec=160, build=build)
        args.update(kw)
        ok, note = bench.pmc_context_matches("lv", args["B"], args["rec"], args["build"])
        assert not ok and what in note
    monkeypatch.setattr(bench, "pmc_profile", lambda w, k: None)
    assert not bench.pmc_context_matches("lv", 65536, 160, build)[0]


def test_truth_gradient_error_of_the_first_draws(golden_dir):
    import bench
    t = np.load(os.path.join(golden_dir, "truth_lv.npz"))
    res = {"head_grads": t["grad_params"] * (1 + 1e-7), "head_lamda": -t["grad_y0"]}
    err = bench.truth_gradient_error("lv", res)
    assert err["draws"] == 16 and 5e-8 < err["dL_dp_max_rel"] < 2e-7 and err["dL_dy0_max_rel"] == 0.0
    assert bench.truth_gradient_error("seir", res) is None


class _CountingEngine:
    """Stand-in for bench.GpuEngine (same interface): counts its steps; every output array holds that count."""

    made = []

    def __init__(self, name, prob, batch, tol, local_rank, arena_bytes=0):
        self.B, self.n_t, self.n = batch["y0"].shape[0], len(batch["tvals"]), prob.n_states
        self.steps = 0
        _CountingEngine.made.append(self)

    def step(self):
        self.steps += 1

    def kernel_ms(self):
        return 1.0, 1.0

    def sync(self):
        pass

    def results(self):
        return dict(failed=0, stats_f=np.ones(16), stats_b=np.ones(16), arena=(0, 0, False))

    def outputs(self):
        return {"y_out": np.full((self.B, self.n_t, self.n), float(self.steps)),
                "st_f": np.full(self.B, self.steps, np.int32), "stats_b": np.full((self.B, 16), self.steps, np.int64)}

    def close(self):
        pass


def test_steps_are_the_timed_steps_and_the_dump_is_the_last_step(tmp_path):
    import bench
    args = bench.parse_args(["--steps", "3", "--warmup", "2", "--batch", "40", "--dump-outputs", str(tmp_path)])
    _CountingEngine.made.clear()
    line = bench.run_rank(args, make_engine=_CountingEngine)
    (eng,) = _CountingEngine.made
    assert eng.steps == 5 and line["steps"] == 3 and line["warmup"] == 2
    assert line["ms_per_step"] > 0 and abs(line["value"] - 40 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert sorted(os.listdir(tmp_path)) == ["instance.npy", "st_f.npy", "stats_b.npy", "y_out.npy"]
    y = np.load(tmp_path / "y_out.npy")
    assert y.dtype == np.float64 and y.shape == (40, 50, 2) and (y == 5.0).all()
    assert (np.load(tmp_path / "st_f.npy") == 5.0).all() and (np.load(tmp_path / "stats_b.npy") == 5.0).all()
    np.testing.assert_array_equal(np.load(tmp_path / "instance.npy"), np.arange(40.0))
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", str(tmp_path)]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def _main_line(bench, monkeypatch, capsys, argv):
    """The line `bench.main(argv)` prints with a counting engine, and the --full parts it ran (in order)."""
    ran = []
    monkeypatch.setattr(bench, "GpuEngine", _CountingEngine)
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: ran.append("cpu_baseline") or {"value": 1.0})
    monkeypatch.setattr(bench, "host_api", lambda *a, **k: ran.append("host_api") or {"solves_per_s": 1.0})
    monkeypatch.setattr(bench, "extra_configs", lambda *a, **k: ran.append("configs") or {})
    monkeypatch.setattr(bench, "first_use", lambda *a, **k: ran.append("first_use") or {})
    monkeypatch.setattr(bench, "truth_gradient_error", lambda *a, **k: ran.append("truth") or {"draws": 16})
    _CountingEngine.made.clear()
    bench.main(argv)
    (text,) = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    return json.loads(text), ran


FULL_ONLY = ("cpu_baseline", "host_api", "configs", "first_use", "truth_gradient_error")


def test_a_plain_run_measures_the_headline_figure_alone(monkeypatch, capsys):
    import bench
    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "40"]
    for extra in ([], ["--no-cpu-baseline"], ["--no-extra-configs"]):
        line, ran = _main_line(bench, monkeypatch, capsys, argv + extra)
        assert ran == [] and not any(k in line for k in FULL_ONLY) and line["full"] is False
        (eng,) = _CountingEngine.made
        assert eng.steps == 5                       # warm-up + timed steps, nothing else stepped an engine
        assert line["unit"] == "solves/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert line["metric"].startswith("fp64 forward+adjoint ODE solves/sec") and line["steps"] == 3
        assert abs(line["value"] - 40 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
        assert {"roofline", "work", "config", "build"} <= set(line)      # (figures of the timed steps themselves stay)


def test_full_runs_every_other_measurement_after_the_timed_steps(monkeypatch, capsys):
    import bench
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "40", "--full"]
    line, ran = _main_line(bench, monkeypatch, capsys, argv)
    assert ran == ["truth", "cpu_baseline", "host_api", "configs", "first_use"]
    assert all(k in line for k in FULL_ONLY) and line["full"] is True
    assert _CountingEngine.made[0].steps == 5 and line["steps"] == 3 and line["warmup"] == 2
    line, ran = _main_line(bench, monkeypatch, capsys, argv + ["--no-cpu-baseline"])
    assert ran == ["truth", "host_api", "configs", "first_use"] and "cpu_baseline" not in line
    line, ran = _main_line(bench, monkeypatch, capsys, argv + ["--no-extra-configs"])
    assert ran == ["truth", "cpu_baseline"]
    line, ran = _main_line(bench, monkeypatch, capsys, argv + ["--workload", "seir"])     # (configs: the headline workload's)
    assert ran == ["truth", "cpu_baseline", "host_api", "first_use"]


def test_dump_outputs_keeps_a_fixed_sample_of_rows_within_the_size_bound(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    B = 5000
    outputs = {"y_out": np.arange(B * 6, dtype=np.float64).reshape(B, 3, 2),
               "st_b": (np.arange(B) % 7 - 3).astype(np.int32), "stats_f": np.arange(B * 16).reshape(B, 16)}
    for d in ("a", "b"):
        bench.dump_outputs(outputs, str(tmp_path / d))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["instance.npy", "st_b.npy", "stats_f.npy", "y_out.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 200_000
    rows = np.load(tmp_path / "a" / "instance.npy")
    assert 1000 < len(rows) < B and (np.diff(rows) > 0).all()
    rows = rows.astype(np.int64)
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b)
        if f != "instance.npy":
            np.testing.assert_array_equal(a, outputs[f[:-4]][rows])
