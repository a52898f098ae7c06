"""The device-memory call path (SA_MEM_DEVICE, torch tensors, a caller's stream -- what bench.py times) and the arena
orchestration behind it, pinned to the host-memory path.

The comparison is always the same: the raw NativeSolver entry points with SA_MEM_DEVICE and torch tensors against a
second handle of the same code object with SA_MEM_HOST and numpy arrays -- every fp64 output bit for bit, every status,
and the counters the suite compares elsewhere (CMP / CMP_B).  The host path is what the rest of the suite pins to the
oracle and to truth; equality carries those pins over.  One case (the guard-on one, smoke()'s inputs) is also held
against tests/golden/truth_lv.npz directly.

Every torch case runs in a fresh child process, like bench.py; the functions the children run live in this module.

Batch L (`batch_l`): lv_batch(200) on linspace(0, 100, 25) at 1e-8 -- between 323 and 851 stored points per instance,
107 of the 200 above the 512 rows of a first resident attempt (measured on the CPU oracle); the children assert those
properties of the host reference before they rely on them.

Measured on an MI355X (the producer queued in front of every default-stream call, against one warm solver call): LV
22.6 ms / 0.64 ms, SEIR 41.8 / 3.85, LV memory-resident 41.2 / 3.84, LV sens 23.2 / 1.98, SEIR sens 827 / 79.6; with
NativeSolver.solve_sens as it was before it called _torch_guard the LV sens case failed at once (all 6700 entries of
y differ: the kernel read the NaN-filled inputs).  DESIGN.md section 2.1, "Device-memory path".
"""
import functools
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMP = [0, 1, 2, 3, 4, 5, 6, 7, 8]            # as tests/test_gpu_fullsize.py
CMP_B = [0, 1, 2, 3, 4, 5, 6, 9, 10, 12]
TOLK = dict(rtol=1e-8, atol=1e-8, rtolB=1e-8, atolB=1e-8, rtolQB=1e-8, atolQB=1e-8)
TOL = dict(abstol=1e-8, reltol=1e-8, backward_abstol=1e-8, backward_reltol=1e-8, quad_abstol=1e-8, quad_reltol=1e-8)
FWD = ("y", "st", "sc")
BWD = ("g", "lam", "stb", "scb", "la", "qa")
SENS = ("y", "s", "st", "sc")
HOST, DEVICE = 0, 1                          # _native.SA_MEM_HOST / SA_MEM_DEVICE
FIRST_ROWS = 512                             # rows of a handle's first resident attempt (csrc/sunode_amd.cpp)


# ------------------------------------------------------------------------------------------------------------------
# cases, handles and the two ways of calling them
# ------------------------------------------------------------------------------------------------------------------
class Case:
    """One batch: inputs as numpy arrays, shared and per-instance forms of every strided argument."""

    def __init__(self, name, B, tvals=None):
        from sunode_amd import _native
        from tests.helpers import make_problem
        from tools import problems
        prob = make_problem(name)
        if name == "lv":
            d = problems.lv_batch(B)
            ps = d["params"][:, prob.params_subset.subset_index]
            pr = d["params"][:, prob.params_subset.remainder_index]      # [B, 2]: a remainder of every instance's own
        else:
            d = getattr(problems, name + "_batch")(B)
            ps, pr = d["ps"], d["pr"]                                    # (seir: one contact matrix for the batch)
        c = lambda a: np.ascontiguousarray(a, dtype=np.float64)          # noqa: E731
        self.name, self.prob, self.src = name, prob, prob.native_source()
        self.B, self.n, self.p, self.r = B, prob.n_states, prob.n_params, prob.n_remainder_native
        self.y0, self.ps, self.pr = c(d["y0"]), c(ps), c(prob.extend_remainder(pr))
        self.tv = c(d["tvals"] if tvals is None else tvals)
        self.n_t = len(self.tv)
        self.grads = c(problems._cotangents(B, self.n_t, self.n))
        rng = np.random.default_rng(11)                                  # per-instance times: own start, own length
        self.t0p = c(rng.uniform(0.0, 1.0, B))
        self.tvp = c(self.t0p[:, None] + self.tv[None, :] * rng.uniform(0.8, 1.0, (B, 1)))
        self.compact = _native.default_compact_trajectory(self.src)      # (reads SA_FORCE_GROUP, like the build)

    def forward_inputs(self, per_instance, times=False):
        """per_instance: every instance's own remainder (where the model has one); times: own t0 / grid as well"""
        pr = self.pr if (per_instance or self.pr.ndim == 1) else np.ascontiguousarray(self.pr[0])
        X = dict(y0=self.y0, ps=self.ps, pr=pr, tvals=self.tvp if times else self.tv)
        if times:
            X["t0"] = self.t0p
        return X

    def backward_inputs(self, per_instance, times=False):
        X = self.forward_inputs(per_instance, times)
        del X["y0"]
        X["grads"] = self.grads if per_instance else np.ascontiguousarray(self.grads[0])
        if times:
            X["tb"], X["tend"] = np.ascontiguousarray(self.tvp[:, -1]), X.pop("t0")
        return X

    def sens0(self):
        from sunode_amd.solver import initial_sensitivities
        return np.ascontiguousarray(np.broadcast_to(initial_sensitivities(self.prob), (self.B, self.p, self.n)))

    def shapes(self):
        B, n_t, n, p = self.B, self.n_t, self.n, self.p
        return dict(y=((B, n_t, n), np.float64), st=((B,), np.int32), sc=((B, 16), np.int64),
                    g=((B, p), np.float64), lam=((B, n), np.float64), stb=((B,), np.int32), scb=((B, 16), np.int64),
                    la=((B, n_t, n), np.float64), qa=((B, n_t, p), np.float64), s=((B, n_t, p, n), np.float64))


def batch_l():
    return Case("lv", 200, np.linspace(0, 100, 25))


def engine(c, **kw):
    from sunode_amd import _native
    kw = dict(TOLK, **kw)
    kw.setdefault("guard", False)
    return _native.NativeSolver(c.src, device=0, n_states=c.n, compact=c.compact and not kw.get("sens"), **kw)


def call_forward(eng, mem, c, X, O, adjoint=True):
    rs = c.r if X["pr"].ndim == 2 else 0
    if "t0" in X:
        eng.solve(mem, c.B, X["y0"], X["ps"], X["pr"], rs, X["t0"], X["tvals"], c.n_t, O["y"], O["st"], O["sc"],
                  adjoint=adjoint, t0_stride=1, tvals_stride=c.n_t)
    else:
        eng.solve(mem, c.B, X["y0"], X["ps"], X["pr"], rs, 0.0, X["tvals"], c.n_t, O["y"], O["st"], O["sc"],
                  adjoint=adjoint)


def call_backward(eng, mem, c, X, O):
    rs = c.r if X["pr"].ndim == 2 else 0
    gs = c.n_t * c.n if X["grads"].ndim == 3 else 0
    if "tb" in X:
        eng.solve_backward(mem, c.B, X["ps"], X["pr"], rs, X["tb"], X["tend"], X["tvals"], c.n_t, X["grads"], gs,
                           O["g"], O["lam"], O["stb"], O["scb"], O["la"], O["qa"], t0_stride=1, tend_stride=1,
                           tvals_stride=c.n_t)
    else:
        eng.solve_backward(mem, c.B, X["ps"], X["pr"], rs, float(c.tv[-1]), 0.0, X["tvals"], c.n_t, X["grads"], gs,
                           O["g"], O["lam"], O["stb"], O["scb"], O["la"], O["qa"])


def call_sens(eng, mem, c, X, O, ism):
    rs = c.r if X["pr"].ndim == 2 else 0
    eng.solve_sens(mem, ism, None, c.B, X["y0"], X["ps"], X["pr"], rs, X["sens0"], 0.0, X["tvals"], c.n_t,
                   O["y"], O["s"], O["st"], O["sc"])


def host_outputs(c, keys):
    return {k: np.zeros(*c.shapes()[k]) for k in keys}


def host_adjoint(eng, c, XF, XB):
    O = host_outputs(c, FWD + BWD)
    call_forward(eng, HOST, c, XF, O)
    call_backward(eng, HOST, c, XB, O)
    return O


def same(got, ref, keys, what, rows=None):
    """bit for bit (fp64 as integers: a NaN equals only the same NaN, -0.0 is not 0.0); counters: CMP / CMP_B"""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if k in ("sc", "scb"):
            cols = CMP if k == "sc" else CMP_B
            a, b = a[:, cols], b[:, cols]
        if rows is not None:
            a, b = a[rows], b[rows]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float64:
            a, b = np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)
        bad = int((a != b).sum())
        assert bad == 0, "%s: %s differs in %d of %d entries" % (what, k, bad, a.size)


# ------------------------------------------------------------------------------------------------------------------
# torch side (children only)
# ------------------------------------------------------------------------------------------------------------------
class Dev:
    """Device tensors, created and filled on torch's current stream."""

    def __init__(self):
        import torch
        self.torch = torch

    def put(self, X):
        return {k: self.torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in X.items()}

    def blank(self, X):
        """inputs of the same shapes, NaN everywhere until a producer has written them"""
        return {k: self.torch.full_like(v, float("nan")) for k, v in X.items()}

    def outputs(self, c, keys):
        tdt = {np.float64: self.torch.float64, np.int32: self.torch.int32, np.int64: self.torch.int64}
        fill = {np.float64: float("nan"), np.int32: -777, np.int64: -1}
        return {k: self.torch.full(c.shapes()[k][0], fill[c.shapes()[k][1]], dtype=tdt[c.shapes()[k][1]], device="cuda")
                for k in keys}

    @staticmethod
    def clone(O, keys):
        return {k: O[k].clone() for k in keys}           # a consumer on the current stream, no synchronisation

    @staticmethod
    def fetch(O):
        return {k: v.cpu().numpy() for k, v in O.items()}


class Producer:
    """A chain of fp64 matrix products on the current stream: the work a caller's inputs are queued behind."""

    def __init__(self, n=2048):
        import torch
        self.torch = torch
        self.a = torch.rand((n, n), dtype=torch.float64, device="cuda") * (2.0 / n)      # (row sums about 1: bounded)
        self.x = torch.rand((n, n), dtype=torch.float64, device="cuda")
        self.y = torch.empty_like(self.x)

    def run(self, reps):
        for _ in range(reps):
            self.torch.mm(self.x, self.a, out=self.y)
            self.x, self.y = self.y, self.x

    def time_ms(self, reps):
        e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run(reps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def size_for(self, warm_ms, label):
        """repetitions whose measured duration is at least ten warm solver calls (and 20 ms: the host needs a moment
        to reach the native call after queueing them)"""
        want = max(10.0 * warm_ms, 20.0)
        self.time_ms(4)                                    # (first launches: library initialisation)
        reps, ms = 16, 0.0
        for _ in range(8):                                 # (short chains are launch-bound: measure, scale, measure)
            ms = self.time_ms(reps)
            if ms >= want:
                break
            reps = int(math.ceil(reps * max(1.5, 1.3 * want / ms)))
        print("%s: producer %d products %.1f ms, warm solver call %.2f ms (host wall time)" % (label, reps, ms, warm_ms))
        assert ms >= want, (ms, warm_ms)
        return reps


def produce(prod, reps, srcs, ins):
    """On the current stream: NaN into the inputs, the long producer, then the real values.  Returns an event behind
    them; the caller checks that it has NOT happened when the native call is entered."""
    import torch
    for v in ins.values():
        v.fill_(float("nan"))
    prod.run(reps)
    for k in ins:
        ins[k].copy_(srcs[k])
    ev = torch.cuda.Event()
    ev.record()
    return ev


def warm_call_ms(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def default_stream_family(name, B, tvals=None, label=None):
    """(a) every kind of call of one kernel family on the library-owned stream (the handle orders itself against
    torch's current stream), every input queued behind the producer, every output consumed by a torch op."""
    label = label or name
    c = Case(name, B, tvals)
    dev, prod = Dev(), Producer()
    H, D = engine(c), engine(c)
    assert H.code_object == D.code_object
    O = dev.outputs(c, FWD + BWD)
    XF = dev.put(c.forward_inputs(True))
    reps = prod.size_for(warm_call_ms(lambda: call_forward(D, DEVICE, c, XF, O, adjoint=False)), label)

    ref = host_outputs(c, FWD)
    call_forward(H, HOST, c, c.forward_inputs(True), ref, adjoint=False)
    assert (ref["st"] == 0).all()
    ins = dev.blank(XF)
    ev = produce(prod, reps, XF, ins)
    assert not ev.query(), "the producer had finished before the call"
    call_forward(D, DEVICE, c, ins, O, adjoint=False)
    same(dev.fetch(dev.clone(O, FWD)), ref, FWD, label + " plain solve")

    for per_instance in (True, False):
        what = "%s adjoint, %s cotangents and remainder" % (label, "per-instance" if per_instance else "shared")
        ref = host_adjoint(H, c, c.forward_inputs(per_instance), c.backward_inputs(per_instance))
        assert (ref["st"] == 0).all() and (ref["stb"] == 0).all()
        XF, XB = dev.put(c.forward_inputs(per_instance)), dev.put(c.backward_inputs(per_instance))
        inF, inB = dev.blank(XF), dev.blank(XB)
        O = dev.outputs(c, FWD + BWD)
        ev = produce(prod, reps, XF, inF)
        assert not ev.query(), "the producer had finished before the call"
        call_forward(D, DEVICE, c, inF, O)
        got = dev.clone(O, FWD)
        ev = produce(prod, reps, XB, inB)
        assert not ev.query(), "the producer had finished before the call"
        call_backward(D, DEVICE, c, inB, O)
        got.update(dev.clone(O, BWD))
        same(dev.fetch(got), ref, FWD + BWD, what)
    H.close()
    D.close()


def default_stream_sens(name, B, tvals=None):
    """(a) forward sensitivities, simultaneous and staggered, on the library-owned stream behind the producer."""
    c = Case(name, B, tvals)
    dev, prod = Dev(), Producer()
    H, D = engine(c, sens=True), engine(c, sens=True)
    X = dict(c.forward_inputs(True), sens0=c.sens0())
    XD = dev.put(X)
    O = dev.outputs(c, SENS)
    reps = prod.size_for(warm_call_ms(lambda: call_sens(D, DEVICE, c, XD, O, 0)), name + " sens")
    for ism in (0, 1):
        ref = host_outputs(c, SENS)
        call_sens(H, HOST, c, X, ref, ism)
        assert (ref["st"] == 0).all()
        ins = dev.blank(XD)
        O = dev.outputs(c, SENS)
        ev = produce(prod, reps, XD, ins)
        assert not ev.query(), "the producer had finished before the call"
        call_sens(D, DEVICE, c, ins, O, ism)
        same(dev.fetch(dev.clone(O, SENS)), ref, SENS, "%s solve_sens ism=%d" % (name, ism))
    H.close()
    D.close()


def check_batch_l_counts(ref):
    """what the 512-row cases rely on, from the host reference's own counters"""
    pts = ref["sc"][:, 8]
    assert (ref["st"] == 0).all() and (ref["stb"] == 0).all()
    assert pts.min() < FIRST_ROWS < pts.max() and not (pts > FIRST_ROWS).all(), (pts.min(), pts.max())
    return pts


def user_stream_steps():
    """(b) bench.py's arrangement: the caller's stream, producers and consumers on it, three steps on one handle
    without any host synchronisation by the caller; then back to the library-owned stream."""
    import torch
    c = batch_l()
    dev = Dev()
    H, D = engine(c), engine(c)
    XFn, XBn = c.forward_inputs(True), c.backward_inputs(True)
    ref = host_adjoint(H, c, XFn, XBn)
    check_batch_l_counts(ref)
    assert H.arena_info()[2]                               # the host handle went the same way: overflow, then tiled
    same(host_adjoint(H, c, XFn, XBn), ref, FWD + BWD, "host path, second step (resident)")
    assert not H.arena_info()[2]

    prod = Producer()
    XF, XB = dev.put(XFn), dev.put(XBn)
    O = dev.outputs(c, FWD + BWD)
    W = engine(c)                                          # (D's first call stays the first adjoint call of its handle)
    reps = prod.size_for(warm_call_ms(lambda: call_forward(W, DEVICE, c, XF, O, adjoint=False)), "batch L")
    W.close()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    D.set_stream(stream.cuda_stream)
    got, info = [], []
    with torch.cuda.stream(stream):
        inF, inB = dev.blank(XF), dev.blank(XB)
        O = dev.outputs(c, FWD + BWD)
        for step in range(3):
            ev = produce(prod, reps, XF, inF)
            for k in inB:
                inB[k].copy_(XB[k])
            assert not ev.query(), "the producer had finished before the call"
            call_forward(D, DEVICE, c, inF, O)
            g = dev.clone(O, FWD)
            call_backward(D, DEVICE, c, inB, O)
            g.update(dev.clone(O, BWD))
            got.append(g)
            info.append(D.arena_info())                    # (settled by the backward call: no synchronisation)
            for v in list(O.values()) + list(inB.values()):
                v.fill_(-1 if not v.is_floating_point() else float("nan"))
        got = [dev.fetch(g) for g in got]                  # the end of the third step: the first wait for the stream
    for step, g in enumerate(got):
        same(g, ref, FWD + BWD, "user stream, step %d" % (step + 1))
    print("batch L arena_info after steps 1-3:", info)
    assert info[0][2] and info[0][1] >= 1                  # step 1: 512 rows overflowed, re-integrated in tiles
    assert not info[1][2] and not info[2][2]               # rows_hint: resident from the second step on
    assert info[1][1] == info[0][1] == info[2][1]          # ... and the tile counter stands still
    D.set_stream(None)
    torch.cuda.synchronize()
    XF, XB = dev.put(XFn), dev.put(XBn)                    # default-stream tensors
    O = dev.outputs(c, FWD + BWD)
    call_forward(D, DEVICE, c, XF, O)
    g = dev.clone(O, FWD)
    call_backward(D, DEVICE, c, XB, O)
    g.update(dev.clone(O, BWD))
    same(dev.fetch(g), ref, FWD + BWD, "back on the library-owned stream")
    H.close()
    D.close()


def lv_record_bytes():
    """bytes of one arena record of the LV code object: a batch whose first call stays resident holds
    512 rows x round64(B) records"""
    c = Case("lv", 64)
    H = engine(c)
    ref = host_adjoint(H, c, c.forward_inputs(True), c.backward_inputs(True))
    assert (ref["st"] == 0).all() and ref["sc"][:, 8].max() < FIRST_ROWS
    nbytes, _, tiled = H.arena_info()
    H.close()
    assert not tiled and nbytes % (FIRST_ROWS * 64 * 8) == 0, (nbytes, tiled)
    return nbytes // (FIRST_ROWS * 64)


def tiled_budget(pts, rec):
    """about one and a half 64-instance groups at the batch's largest point count"""
    return int(1.5 * 64 * int(pts.max()) * rec)


def tiled_device_memory():
    """(c) an arena of a few tiles, device memory, the caller's stream: shared arguments, then every strided argument
    per instance; the forward call's buffers are overwritten before the backward call (the library kept copies)."""
    import torch
    c = batch_l()
    dev = Dev()
    rec = lv_record_bytes()
    H = engine(c)                                          # resident reference (default budget)
    stream = torch.cuda.Stream()
    most = 0                                               # (arena_info: the largest arena of the handle's life)
    for times in (False, True):
        what = "tiled, device memory, %s" % ("every argument per instance" if times else "shared grid / cotangent / remainder")
        XFn, XBn = c.forward_inputs(times, times), c.backward_inputs(times, times)
        ref = host_adjoint(H, c, XFn, XBn)
        assert (ref["st"] == 0).all() and (ref["stb"] == 0).all()
        budget = tiled_budget(ref["sc"][:, 8], rec)
        if not times:
            D = engine(c, arena_bytes=budget)              # (one handle for both runs: shared times, then per instance)
            D.set_stream(stream.cuda_stream)
        else:
            D.set_options(arena_bytes=budget)
        tiles0, most = D.arena_info()[1], max(most, budget)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            XF, XB = dev.put(XFn), dev.put(XBn)            # (the backward call gets tensors of its own)
            O = dev.outputs(c, FWD + BWD)
            call_forward(D, DEVICE, c, XF, O)
            got = dev.clone(O, FWD)
            for k in ("y0", "tvals", "t0"):                # the caller reuses its buffers: garbage on the same stream
                if k in XF:
                    XF[k].fill_(float("nan"))
            O["y"].fill_(float("nan"))
            O["st"].fill_(-12345)
            O["sc"].fill_(-1)
            call_backward(D, DEVICE, c, XB, O)
            got.update(dev.clone(O, BWD))
            got = dev.fetch(got)
        same(got, ref, FWD + BWD, what)
        nbytes, tiles, tiled = D.arena_info()
        print("%s: budget %d bytes, %d tiles, largest tile %d bytes" % (what, budget, tiles - tiles0, nbytes))
        assert tiled and tiles - tiles0 >= 2 and nbytes <= most
    H.close()
    D.close()


def arena_statuses():
    """(d) the two ways an instance leaves the arena, in both memory modes."""
    c = batch_l()
    dev = Dev()
    rec = lv_record_bytes()
    XFn, XBn = c.forward_inputs(True), c.backward_inputs(True)
    H = engine(c)
    ref = host_adjoint(H, c, XFn, XBn)
    H.close()
    pts = check_batch_l_counts(ref)
    R = int(np.sort(pts)[len(pts) // 2])                   # the median: between the shortest and the longest
    assert pts.min() < R < pts.max()
    full = pts > R
    nan = lambda a: bool(np.isnan(a).all())                # noqa: E731

    def both_modes(what, **kw):
        H, D = engine(c, **kw), engine(c, **kw)
        host = host_adjoint(H, c, XFn, XBn)
        XF, XB = dev.put(XFn), dev.put(XBn)
        O = dev.outputs(c, FWD + BWD)
        call_forward(D, DEVICE, c, XF, O)
        got = dev.clone(O, FWD)
        call_backward(D, DEVICE, c, XB, O)
        got.update(dev.clone(O, BWD))
        got = dev.fetch(got)
        same(got, host, FWD + BWD, what + ", device against host memory")
        infos = H.arena_info(), D.arena_info()
        H.close()
        D.close()
        return host, got, infos

    # an instance with more than traj_capacity points: stopped at the bound in the forward call
    for mode, out in zip(("host", "device"), both_modes("traj_capacity", traj_capacity=R)[:2]):
        what = "traj_capacity = %d, %s memory" % (R, mode)
        assert (out["st"][full] == -9001).all() and (out["st"][~full] == 0).all(), what
        assert (out["stb"][full] == -102).all() and (out["stb"][~full] == 0).all(), what
        assert nan(out["y"][full]) and (out["sc"][full, 8] == R).all(), what
        assert nan(out["g"][full]) and nan(out["lam"][full]) and nan(out["la"][full]) and nan(out["qa"][full]), what
        same(out, ref, FWD + BWD, what + ", the other instances", rows=~full)

    # a 64-instance group of R-point trajectories is all the budget holds: longer instances are taken out by the
    # backward call, the forward call does not know yet
    host, got, infos = both_modes("group over budget", arena_bytes=R * 64 * rec)
    for mode, out, info in zip(("host", "device"), (host, got), infos):
        what = "arena of %d rows x 64 instances, %s memory" % (R, mode)
        same(out, ref, FWD, what + ", forward outputs")
        assert (out["stb"][full] == -9001).all() and (out["stb"][~full] == 0).all(), what
        assert nan(out["g"][full]) and nan(out["lam"][full]) and nan(out["la"][full]) and nan(out["qa"][full]), what
        same(out, ref, BWD, what + ", the other instances", rows=~full)
        assert info[2] and info[1] >= 2 and info[0] <= R * 64 * rec, (what, info)
    print("arena statuses: R = %d of %d..%d points, %d of %d instances beyond" % (R, pts.min(), pts.max(), full.sum(), c.B))


def guard_on_device_memory(golden):
    """(e) the handle bench.py builds -- guard on, the adjoint kind, a caller's stream -- with smoke()'s inputs."""
    import torch
    from sunode_amd import _native
    c = Case("lv", 300)
    dev = Dev()
    verdict = _native.guard_verdict_path(_native.code_object_path(c.src, compact=c.compact))
    if os.path.exists(verdict):                            # (a verdict of an earlier process would leave nothing to check)
        os.remove(verdict)
    XFn, XBn = c.forward_inputs(True), c.backward_inputs(True)
    XBn["grads"] = np.ones((c.n_t, c.n))                   # smoke()'s and bench.py's cotangent, shared
    D = engine(c, guard=True, guard_kinds=("adjoint",))
    assert D.guard_report["enabled"] and D.guard_state()["pending"] == ["adjoint"]
    stream = torch.cuda.Stream()
    D.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        XF, XB = dev.put(XFn), dev.put(XBn)
        O = dev.outputs(c, FWD + BWD)
        call_forward(D, DEVICE, c, XF, O)
        got = dev.clone(O, FWD)
        call_backward(D, DEVICE, c, XB, O)
        got.update(dev.clone(O, BWD))
        got = dev.fetch(got)
    state = D.guard_state()
    assert state["verified"] == ["adjoint"] and state["n_sample"]["adjoint"] == 64, state
    assert not state["differs"] and not state["using_conservative"], state
    H = engine(c)                                          # guard off
    same(got, host_adjoint(H, c, XFn, XBn), FWD + BWD, "guard on, device memory, against a guard-off handle")
    assert (got["st"] == 0).all() and (got["stb"] == 0).all()
    t = np.load(os.path.join(golden, "truth_lv.npz"))
    err = np.max(np.abs(got["g"][:16] - t["grad_params"]) / np.abs(t["grad_params"]).max(axis=1, keepdims=True))
    print("guard on, device memory: first 16 gradients against truth %.2e" % err)
    assert err < 4e-6, err                                 # smoke()'s bar
    H.close()
    D.close()


# ------------------------------------------------------------------------------------------------------------------
# the tests: one child process each, one after the other
# ------------------------------------------------------------------------------------------------------------------
_HEAD = r"""
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tools.problems import seir_batch
import tests.test_gpu_device_memory as T
"""

_SCRIPTS = {
    "families": _HEAD + r"""
T.default_stream_family("lv", 67)
T.default_stream_family("seir", 70, seir_batch(1)["tvals"][::5])
os.environ["SA_FORCE_GROUP"] = "mem"
T.default_stream_family("lv", 67, label="lv, memory-resident mapping")
print("DEVICE_MEMORY_OK")
""",
    "sens": _HEAD + r"""
T.default_stream_sens("lv", 67)
T.default_stream_sens("seir", 70, seir_batch(1)["tvals"][::5])
print("DEVICE_MEMORY_OK")
""",
    "user_stream": _HEAD + "T.user_stream_steps()\nprint('DEVICE_MEMORY_OK')\n",
    "tiled": _HEAD + "T.tiled_device_memory()\nprint('DEVICE_MEMORY_OK')\n",
    "statuses": _HEAD + "T.arena_statuses()\nprint('DEVICE_MEMORY_OK')\n",
    "guard": _HEAD + "T.guard_on_device_memory(os.path.join(sys.argv[1], 'tests', 'golden'))\nprint('DEVICE_MEMORY_OK')\n",
}


def _child(key):
    res = subprocess.run([sys.executable, "-c", _SCRIPTS[key], ROOT], capture_output=True, text=True, timeout=300)
    print(res.stdout[-4000:])                              # the measured figures (pytest -s / a failure report)
    assert res.returncode == 0 and "DEVICE_MEMORY_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


def test_every_call_on_the_default_stream_behind_a_producer():
    """(a) plain solve and both adjoint pairs (per-instance and shared cotangents / remainder, lamda_all / quad_all) in
    the one-lane, the lane-group and the memory-resident family."""
    _child("families")


def test_solve_sens_on_the_default_stream_behind_a_producer():
    """(a) solve_sens orders itself against torch's current stream like solve and solve_backward (it did not: with
    its inputs still NaN when the kernel started, every instance failed)."""
    _child("sens")


def test_user_stream_three_steps_on_one_handle():
    """(b) 512-row overflow -> tiled -> rows hint -> resident, step against step."""
    _child("user_stream")


def test_tiled_arena_in_device_memory_with_every_strided_argument():
    _child("tiled")


def test_arena_statuses_in_both_memory_modes():
    """(d) traj_capacity and the 64-instance group that exceeds the budget even alone."""
    _child("statuses")


def test_guard_on_in_device_memory():
    _child("guard")


# -- the same arena cases through AdjointSolver (host memory, no torch: in this process) ---------------------------
@functools.lru_cache(maxsize=None)
def _adjointsolver_reference():
    from sunode_amd.solver import AdjointSolver
    c = batch_l()
    small = Case("lv", 64)
    sol = AdjointSolver(small.prob, **TOL)
    _, st, sc = sol.solve_forward_batch(0.0, small.tv, small.y0, small.ps, small.pr)
    sol.solve_backward_batch(small.tv[-1], 0.0, small.tv, small.grads)
    nbytes, _, tiled = sol._engine().arena_info()
    assert (st == 0).all() and sc[:, 8].max() < FIRST_ROWS and not tiled and nbytes % (FIRST_ROWS * 64 * 8) == 0
    return c, nbytes // (FIRST_ROWS * 64)


def _adjointsolver_run(sol, c, times):
    if times:
        y, st, sc = sol.solve_forward_batch(c.t0p, c.tvp, c.y0, c.ps, c.pr)
        g, lam, stb, scb, la, qa = sol.solve_backward_batch(c.tvp[:, -1], c.t0p, c.tvp, c.grads, return_all=True)
    else:
        y, st, sc = sol.solve_forward_batch(0.0, c.tv, c.y0, c.ps, c.pr)
        g, lam, stb, scb, la, qa = sol.solve_backward_batch(c.tv[-1], 0.0, c.tv, c.grads, return_all=True)
    return {k: np.array(v) for k, v in zip(FWD + BWD, (y, st, sc, g, lam, stb, scb, la, qa))}


def test_tiled_per_instance_arguments_with_all_rows_through_adjointsolver():
    """(c) per-instance times, cotangents and remainder with lamda_all / quad_all, tiled, in host memory."""
    from sunode_amd.solver import AdjointSolver
    c, rec = _adjointsolver_reference()
    ref = _adjointsolver_run(AdjointSolver(c.prob, **TOL), c, True)
    assert (ref["st"] == 0).all() and (ref["stb"] == 0).all()
    tiled = AdjointSolver(c.prob, **TOL, arena_gib=tiled_budget(ref["sc"][:, 8], rec) / 2**30)
    same(_adjointsolver_run(tiled, c, True), ref, FWD + BWD, "AdjointSolver, tiled, every argument per instance")
    assert tiled._engine().arena_info()[1] >= 2


def test_group_over_budget_through_adjointsolver():
    """(d) the 64-instance group that exceeds the budget even alone: RuntimeWarning from the batch call, SolverError
    from the scalar one."""
    from sunode_amd.solver import AdjointSolver, SolverError
    c, rec = _adjointsolver_reference()
    ref = _adjointsolver_run(AdjointSolver(c.prob, **TOL), c, False)
    pts = check_batch_l_counts(ref)
    R = int(np.sort(pts)[len(pts) // 2])
    full = pts > R
    assert full.any() and not full.all()
    gib = (R * 64 * rec + 32 * rec) / 2**30                # (half a row beyond R rows: R whatever the rounding)
    sol = AdjointSolver(c.prob, **TOL, arena_gib=gib)
    y, st, sc = sol.solve_forward_batch(0.0, c.tv, c.y0, c.ps, c.pr)
    with pytest.warns(RuntimeWarning, match="SA_STATUS_ARENA_FULL"):
        g, lam, stb, scb, la, qa = sol.solve_backward_batch(c.tv[-1], 0.0, c.tv, c.grads, return_all=True)
    out = {k: np.array(v) for k, v in zip(FWD + BWD, (y, st, sc, g, lam, stb, scb, la, qa))}
    same(out, ref, FWD, "AdjointSolver, group over budget, forward outputs")
    assert (stb[full] == -9001).all() and (stb[~full] == 0).all()
    assert np.isnan(g[full]).all() and np.isnan(lam[full]).all() and np.isnan(la[full]).all() and np.isnan(qa[full]).all()
    same(out, ref, BWD, "AdjointSolver, group over budget, the other instances", rows=~full)
    # the scalar API on the longest instance
    i = int(np.argmax(pts))
    params = batch_params(c, i)
    one = AdjointSolver(c.prob, **TOL, arena_gib=gib)
    one.set_params_dict(params)
    y_out, grad_out, lamda_out = one.make_output_buffers(c.tv)
    one.solve_forward(0.0, c.tv, c.y0[i], y_out)
    np.testing.assert_array_equal(y_out, ref["y"][i])
    with pytest.warns(RuntimeWarning, match="SA_STATUS_ARENA_FULL"), pytest.raises(SolverError, match="arena budget"):
        one.solve_backward(c.tv[-1], 0.0, c.tv, c.grads[i], grad_out, lamda_out)


def batch_params(c, i):
    from tools.problems import lv_batch
    return dict(zip(("alpha", "beta", "gamma", "delta"), lv_batch(c.B)["params"][i]))
