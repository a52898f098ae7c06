"""Build + ctypes binding of the native engine.

* ``libsunode_amd.so`` (host, C ABI of ``include/sunode_amd.h``) is compiled once with g++
  against the HIP runtime and kept in-tree under ``sunode_amd/_lib/``.
* One gfx950 code object per problem (generated callbacks + ``csrc/bdf_kernels.hip``) is
  compiled on demand and cached by source hash under ``sunode_amd/_cache/``.

The device build is a three-stage pipeline on purpose (see the comment on compile-time loops in
bdf_kernels.hip): clang -O0 -> ``opt always-inline,sroa`` -> clang -O3.  Forcing full inlining
and scalar replacement *before* any other optimisation is what keeps the per-lane integrator
state (about 150 doubles) in VGPRs; the stock -O3 pipeline simplifies the small helpers first
and ends up indexing a scratch copy of the state dynamically.

There is no CPU fallback: if the HIP runtime / a GPU is missing the calls raise.
"""
from __future__ import annotations

import ctypes
import hashlib
import os
import shutil
import subprocess
import tempfile
from typing import Optional

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
_CSRC = os.environ.get("SA_CSRC_DIR") or os.path.join(_PKG, "csrc")      # SA_CSRC_DIR: kernel sources of a scratch tree (tuning)
_LIBDIR = os.path.join(_PKG, "_lib")
_CACHE = os.path.join(_PKG, "_cache")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM_BIN = os.path.join(ROCM, "lib", "llvm", "bin")
ARCH = "gfx950"

SA_MEM_HOST, SA_MEM_DEVICE = 0, 1
N_STATS = 16
STAT_NAMES = ["nst", "nfe", "nsetups", "nje", "nni", "ncfn", "netf", "qlast", "npts", "nfqe", "netfq",
              "ninterp", "nrebuild", "retries", "attempts", "reserved"]


class NativeBuildError(RuntimeError):
    pass


def _run(cmd, **kw):
    res = subprocess.run(cmd, capture_output=True, text=True, **kw)
    if res.returncode != 0:
        raise NativeBuildError("command failed: %s\n%s\n%s" % (" ".join(cmd), res.stdout[-4000:], res.stderr[-4000:]))
    return res


def _hash_files(*paths, extra=b""):
    h = hashlib.sha256(extra)
    for p in paths:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def host_library_path() -> str:
    return os.path.join(_LIBDIR, "libsunode_amd.so")


def build_host_library(force: bool = False) -> str:
    """g++ build of csrc/sunode_amd.cpp -> _lib/libsunode_amd.so (stamp = source hash)."""
    os.makedirs(_LIBDIR, exist_ok=True)
    src = os.path.join(_CSRC, "sunode_amd.cpp")
    deps = [src, os.path.join(_CSRC, "sa_device_abi.h"), os.path.join(_ROOT, "include", "sunode_amd.h")]
    lib = host_library_path()
    stamp = lib + ".stamp"
    want = _hash_files(*deps) if all(os.path.exists(d) for d in deps) else None
    if not force and os.path.exists(lib):
        if want is None:
            return lib
        if os.path.exists(stamp) and open(stamp).read().strip() == want:
            return lib
    if want is None:
        raise NativeBuildError("host library sources missing and no prebuilt %s" % lib)
    # several ranks of one job may get here at once (bench.py --gpus N on a box without the prebuilt files): every
    # process writes its own temporary and publishes it with an atomic rename
    tmp = "%s.tmp%d" % (lib, os.getpid())
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__",
           "-I" + os.path.join(ROCM, "include"), src, "-o", tmp,
           "-L" + os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    _run(cmd)
    os.replace(tmp, lib)
    with open(tmp + ".stamp", "w") as fh:
        fh.write(want)
    os.replace(tmp + ".stamp", stamp)
    return lib


#: Flags of the final clang -O3 stage, all measured on MI355X (same-call A/B blocks in
#: profiles/r03_compact_trajectory.txt).  One lane per instance (bdf_kernels.hip): the iterative ILP scheduler is ~5 %
#: faster than the default for this latency-bound single-wave-per-SIMD kernel; machine LICM off -- the hoisted literal
#: constants otherwise occupy vector registers for the whole kernel (LV backward 370 -> 318 registers, no AGPR
#: shuffling; LV -0.7 %, Robertson backward -1.2 %, Robertson sensitivities -2.5 %).
DEFAULT_CODEGEN_FLAGS = "-mllvm -amdgpu-sched-strategy=iterative-ilp -mllvm -disable-machine-licm"
#: Adjoint builds only: the register allocator splits live ranges for fewer spill instructions (LV backward -0.9 %,
#: SEIR backward -3.4 %, 290 -> 221 spill slots; Robertson / network24 / network100 unchanged); the forward-sensitivity
#: builds lose with it (LV +4 %, Robertson +7 %, SEIR +2 %) and do not get it.
ADJOINT_CODEGEN_FLAGS = "-mllvm -split-spill-mode=size"
#: The lane-group kernels (bdf_wave.hip): plain -O3 scheduling (the ILP strategies are slower there and take several
#: times longer to build at n = 100); adjoint builds: machine LICM and the splitting of critical edges for sinking
#: off (SEIR backward 52.4 -> 51.7 ms, 221 -> 208 spill slots) + the adjoint flag above.
WAVE_CODEGEN_FLAGS = "-mllvm -disable-machine-licm -mllvm -machine-sink-split=0"
#: ... and up to 8 lanes per instance (the lean groups and their neighbours) without memory-operation clustering in the
#: scheduler: SEIR backward 52.0 -> 48.9 ms (291 -> 305 k solves/s), network24 unchanged; the workgroup-per-instance
#: build (network100) loses 0.5 % with it and the sensitivity builds 1 %: not applied there (block 8 of the A/B file)
SMALL_GROUP_CODEGEN_FLAGS = "-mllvm -misched-cluster=0"


#: SIOptimizeVGPRLiveRange -- the AMDGPU pass that shortens VGPR live ranges in divergent if / else regions.  Round 4
#: traced the "parking l[] changes the results" anomaly of the 4-lane forward-sensitivity build to it: with
#: `-disable-machine-licm` and the coefficient vectors parked in LDS the SEIR build differs from the oracle in half of its
#: step counters; the difference survives eight other code-generation variations (no AGPR / SGPR-to-VGPR spilling, no
#: machine CSE, no pre- / post-RA scheduler, no early if-conversion, sink splitting on / off, a hard barrier around the
#: parked values) and disappears with exactly `-amdgpu-opt-vgpr-liverange=0`, with -O1, or when the source reads the
#: parked values once more (which is why it looked like a heisenbug); the machine verifier is silent and the
#: "group-uniform" values are uniform (round 4's diagnostic build).  Reproducer: tools/repro_vgpr_liverange.sh,
#: record: profiles/r04_sens_anomaly.txt.  That configuration is NOT shipped (the sensitivity builds carry neither the
#: parking nor -disable-machine-licm), and every shipped build agrees with the oracle bit for bit (163 GPU tests, all
#: BASELINE batches at full size).  Building everything without the pass costs 10 % (LV) ... 27 % (SEIR) ... 57 %
#: (Robertson sensitivities) -- profiles/r04_vgpr_liverange_ab.txt -- so it stays ON by default and
#: SA_VGPR_LIVERANGE_OPT=0 (or SAFE builds: `sunode_amd._native.SAFE_CODEGEN = True`) turns it off for every
#: register-resident kernel: the conservative build for models nobody has compared with the oracle.
SAFETY_CODEGEN_FLAGS = "-mllvm -amdgpu-opt-vgpr-liverange=0"
SAFE_CODEGEN = False


def all_builds_conservative() -> bool:
    """SA_VGPR_LIVERANGE_OPT=0 (or ``SAFE_CODEGEN = True``): EVERY build is the conservative one."""
    return os.environ.get("SA_VGPR_LIVERANGE_OPT") == "0" or (SAFE_CODEGEN and os.environ.get("SA_VGPR_LIVERANGE_OPT") != "1")


def _safety_flags(safe: bool = False):
    return SAFETY_CODEGEN_FLAGS.split() if (safe or all_builds_conservative()) else []


def _extra_codegen_flags():
    """Extra flags for the final clang -O3 stage (tuning experiments), e.g.
    SA_CLANG_FLAGS="-mllvm -amdgpu-sched-strategy=max-ilp"; part of the cache key."""
    return os.environ.get("SA_CLANG_FLAGS", DEFAULT_CODEGEN_FLAGS).split()


#: systems with more states than this use lane groups (bdf_wave.hip): G lanes per instance
REGISTER_KERNEL_MAX_STATES = 5
#: ... or more differentiated parameters than this (six quadrature Nordsieck columns per parameter in one lane)
REGISTER_KERNEL_MAX_SUB = 8
#: forward sensitivities run in registers while n_states * n_sub stays at or below this
SENS_REGISTER_MAX_NP = 12


def kernel_variant(native_source: str, sens: bool = False, constraints: bool = False, hermite: bool = False,
                   group: Optional[str] = None):
    """(source file, lanes per instance) for a generated problem header.

    ``sens=True`` (forward sensitivities, ``Solver(sens_mode=...)``): the register kernel built with
    ``-DSA_SENS`` while n <= 5 and n * n_sub <= 12, otherwise the memory-resident kernel -- the two
    families carrying the sensitivity corrector.

    n <= 5 states: thread-per-instance, the whole integrator in one lane's registers.
    up to 64: bdf_wave.hip with G lanes per instance (lane_group_size: 4 lanes up to 16 states, 8 up to 21 -- the
        "lean" groups with the LU factors in registers -- then two components per lane, matrix in LDS).
    up to 128: bdf_wave.hip, one 4-wavefront workgroup per instance, Newton matrix / LU resident in LDS.
    larger: memory-resident thread-per-instance kernel (state in an HBM workspace, [element][instance]).
    SA_FORCE_GROUP=<G> or wave<G> forces G lanes per instance (tests run small problems through every mapping);
    SA_FORCE_GROUP=1 forces the register kernel, SA_FORCE_GROUP=wave the workgroup-per-instance one and
    SA_FORCE_GROUP=mem the memory-resident one.  ``group``: the same values as an argument (takes precedence over the
    environment): how ``AdjointSolver`` asks for the small-batch mapping of a model (``small_batch_group``)."""
    import re
    n = int(re.search(r"#define SA_N_STATES (\d+)", native_source).group(1))
    p = int(re.search(r"#define SA_N_SUB (\d+)", native_source).group(1))
    forced = group if group is not None else os.environ.get("SA_FORCE_GROUP")
    # (Hermite interpolation: every family carries it -- since round 2 the register kernel too)
    if sens:
        # forward sensitivities: the register kernel keeps the p sensitivity Nordsieck arrays (14 n p doubles) next
        # to the state's while they fit one lane's register file; everything larger runs memory-resident
        if forced in (None, "1") and n <= REGISTER_KERNEL_MAX_STATES and n * p <= SENS_REGISTER_MAX_NP:
            return "bdf_kernels.hip", 1
        # lean lane groups (sensitivity vectors streamed from the workspace): everything they cover (n <= 21)
        g = int(forced[4:]) if forced and forced.startswith("wave") and forced != "wave" else \
            (None if forced else lane_group_size(n, p))
        if g in (2, 4, 8) and n * ((n + g - 1) // g) <= 64 and 8 * g >= max(n, p) and n >= 1:
            return "bdf_wave.hip", g
        return "bdf_mem.hip", 1
    if forced == "mem" or (not forced and max(n, p) > 128):
        return "bdf_mem.hip", 1
    if forced == "wave" or (not forced and max(n, p) > 64):
        if max(n, p) > 128 or n < 1:
            raise NativeBuildError("the wavefront-per-instance kernel covers 1 <= n_states <= 128, n_sub <= 128")
        return "bdf_wave.hip", 64
    if forced and forced.startswith("wave"):        # "wave16": bdf_wave.hip with 16 lanes per instance
        g = int(forced[4:])
        if 8 * g < max(n, p) or g > 64 or g & (g - 1) or g < 1:
            raise NativeBuildError("bdf_wave.hip group size %d must be a power of two with 8*G >= max(n, p)=%d"
                                   % (g, max(n, p)))
        return "bdf_wave.hip", g
    if forced:                                       # "8" / "16": that many lanes per instance (same as "wave8" / ...)
        g = int(forced)
        if g == 1:
            return "bdf_kernels.hip", 1
        if 8 * g < max(n, p) or g > 64 or g & (g - 1) or g < 2:
            raise NativeBuildError("lane groups need a power of two 2 <= G <= 64 with 8*G >= max(n_states, n_sub) = %d"
                                   % max(n, p))
        return "bdf_wave.hip", g
    if n <= REGISTER_KERNEL_MAX_STATES and p <= REGISTER_KERNEL_MAX_SUB:
        return "bdf_kernels.hip", 1
    return "bdf_wave.hip", lane_group_size(n, p)


def lane_group_size(n: int, p: int) -> int:
    """Lanes per instance of the lane-group kernel for 6 <= max(n, p) <= 64.

    LEAN groups (bdf_wave.hip, SA_LEAN: LU factors in registers, cold state in LDS) exist while a lane's share of the
    matrix, n * ceil(n / G), is at most 64 doubles: G = 4 up to 16 states (16 instances per wavefront: the control
    scalars and the generated callbacks, evaluated redundantly by every lane of a group, cost half of what they
    cost with 8 lanes -- SEIR: 235 k against 191 k solves/s), G = 8 up to 21.  Larger systems keep the matrix in LDS
    with two components per lane (G = next power of two >= max(n, p) / 2)."""
    for g in (4, 8):
        if n * ((n + g - 1) // g) <= 64 and 8 * g >= max(n, p):
            return g
    g = 8
    while 2 * g < max(n, p):
        g *= 2
    return g


def small_batch_group(native_source: str, hermite: bool = False, batch: int = 1) -> Optional[str]:
    """The mapping ``AdjointSolver`` switches to for a SMALL batch (``batch`` = instances on one handle), or None for
    the engine's own choice (``kernel_variant``).

    The chip holds 1 024 wavefronts at one per SIMD -- the occupancy of every backward kernel here.  With G lanes per
    instance a batch of B instances is B G / 64 wavefronts: one lane per instance fills the chip only from 65 536
    instances on, 4-lane groups from 16 384.  Below that, more lanes per instance put more SIMDs to work AND finish an
    instance sooner.  Measured, forward + adjoint (profiles/r06_mapping_by_batch.txt, r06_lanes_by_batch.txt):
      * models the engine maps to ONE lane (n <= 5, p <= 8) with n >= 4 states, 4-lane groups instead, B <= 16 384:
        n = 5, p = 8: +40 ... 55 %; n = 4, p = 8: +30 ... 50 %; n = 4 / 5, p = 2: +8 ... 22 %.  (n = 3: equal, and 7 ...
        15 % slower with transcendental callbacks, which every lane of a group evaluates: not switched); 8 / 16 lanes add
        another +5 ... 23 % up to 4 096 instances (profiles/r06_lanes_small_models.txt);
      * models the engine maps to 4-lane groups (6 <= n <= 16), 16 lanes per instance instead while B <= 4 096: SEIR
        +25 ... 37 %, 12 states +17 ... 28 %, 7 states +13 ... 18 %; 8 lanes while B <= 8 192: SEIR +22 ... 30 % at 4 096.
      * at the next size up (16 384 / 65 536) the engine's own choice wins by 1.5 ... 4x: it stays the large-batch mapping.
    Rule: the largest measured group size whose wavefront count B G / 64 still fits the chip.  Results are
    bit-identical in every mapping.  SA_FORCE_GROUP (a forced mapping) and SA_BATCH_MAPPING=fixed switch this off."""
    import re
    if os.environ.get("SA_FORCE_GROUP") or os.environ.get("SA_BATCH_MAPPING", "auto") == "fixed":
        return None
    n = int(re.search(r"#define SA_N_STATES (\d+)", native_source).group(1))
    fname, g = kernel_variant(native_source, hermite=hermite)
    one_lane = fname == "bdf_kernels.hip" and n >= SMALL_BATCH_MIN_STATES
    if one_lane or (fname == "bdf_wave.hip" and g == 4):
        if batch <= SMALL_BATCH_MAX // 4:
            return "wave16"
        if batch <= SMALL_BATCH_MAX // 2:
            return "wave8"
        if one_lane and batch <= SMALL_BATCH_MAX:
            return "wave4"
    return None


#: a handle's batch up to which 4-lane groups replace one lane per instance (16 384 four-lane instances = one wavefront per
#: SIMD); 8 / 16 lanes replace 4 up to a half / a quarter of it
SMALL_BATCH_MAX = 16384
SMALL_BATCH_MIN_STATES = 4


def default_compact_trajectory(native_source: str, hermite: bool = False, group: Optional[str] = None) -> bool:
    """Arena record format AdjointSolver picks by default: compact {order, t, y[n]} records (table rebuilt by the
    backward kernel) from three states on, in the register-resident kernels -- measured, profiles/
    r03_compact_trajectory.txt: Robertson 73 -> 14 GB and +18 %; SEIR / network24 / network100 the same throughput
    (+-0.5 %) in a sixth of the arena; Lotka-Volterra (n = 2) -4 % -- table records there and in bdf_mem.hip."""
    import re
    n = int(re.search(r"#define SA_N_STATES (\d+)", native_source).group(1))
    return (not hermite) and n >= 3 and \
        kernel_variant(native_source, hermite=hermite, group=group)[0] in ("bdf_kernels.hip", "bdf_wave.hip")


def _size_defines(native_source: str):
    """-D flags of the device build: problem sizes + SA_KERNEL_DEFINES (tuning / profiling builds,
    e.g. SA_KERNEL_DEFINES="-DSA_WAVE_PROFILE"; part of the cache key)."""
    import re
    n = int(re.search(r"#define SA_N_STATES (\d+)", native_source).group(1))
    p = int(re.search(r"#define SA_N_SUB (\d+)", native_source).group(1))
    return ["-DSA_BUILD_NS=%d" % n, "-DSA_BUILD_NQ=%d" % p] + os.environ.get("SA_KERNEL_DEFINES", "").split()


def _band_widths(native_source: str, fname: str, band):
    """(ml, mu) of a band build (``band`` = (lower, upper) bandwidth of the Jacobian), clamped to n - 1, or None: only
    the memory-resident mapping carries the band LU, and a missing kernel is an error."""
    import re
    if band is None:
        return None
    if fname != "bdf_mem.hip":
        raise NativeBuildError("band=%r: only the memory-resident mapping (bdf_mem.hip) has a band LU, this build "
                               "is %s" % (band, fname))
    n = int(re.search(r"#define SA_N_STATES (\d+)", native_source).group(1))
    ml, mu = (int(w) for w in band)
    if ml < 0 or mu < 0:
        raise ValueError("band widths must not be negative: %r" % (band,))
    return min(ml, max(n - 1, 0)), min(mu, max(n - 1, 0))


def code_object_path(native_source: str, sens: bool = False, constraints: bool = False,
                     hermite: bool = False, compact: bool = False, safe: bool = False, group: Optional[str] = None,
                     band=None) -> str:
    """``band`` = (ml, mu): the band build of the memory-resident mapping (-DSA_BAND_ML / -DSA_BAND_MU); the key carries
    a BAND tag only when it is set, so every other build keeps its key."""
    fname, group = kernel_variant(native_source, sens, constraints, hermite, group=group)
    band = _band_widths(native_source, fname, band)
    kern = os.path.join(_CSRC, fname)
    deps = [kern] + [os.path.join(_CSRC, f) for f in ("sa_device_abi.h", "sa_common.h", "bdf_core.h")]
    deps = [d for d in deps if os.path.exists(d)]
    extra = (native_source.encode() + " ".join(_extra_codegen_flags()).encode()
             + (WAVE_CODEGEN_FLAGS + ADJOINT_CODEGEN_FLAGS + SMALL_GROUP_CODEGEN_FLAGS).encode()
             + " ".join(_safety_flags(safe)).encode()
             + b"G%d" % group + fname.encode()
             + os.environ.get("SA_KERNEL_DEFINES", "").encode() + os.environ.get("SA_WAVES_PER_EU", "").encode()
             + (b"SENS" if sens else b"") + (b"CONSTR" if constraints else b"") + (b"HERMITE" if hermite else b"")
             + (b"COMPACT" if compact else b"")
             + (b"BAND%d_%d" % band if band is not None else b""))
    key = _hash_files(*deps, extra=extra) if os.path.exists(kern) else \
        hashlib.sha256(extra).hexdigest()[:16]
    return os.path.join(_CACHE, "sa_%s.hsaco" % key)


def build_code_object(native_source: str, force: bool = False, keep_temps: bool = False,
                      sens: bool = False, constraints: bool = False, hermite: bool = False, compact: bool = False,
                      safe: bool = False, group: Optional[str] = None, band=None) -> str:
    """Compile the integrator kernels for one problem to a gfx950 code object (cached).
    ``constraints=True`` builds the variant that enforces CVodeSetConstraints-style inequality
    constraints (a separate code object: the default build carries no trace of them).
    ``safe=True``: the CONSERVATIVE build -- same source, same defines, same flags, plus SAFETY_CODEGEN_FLAGS
    (SIOptimizeVGPRLiveRange off): the partner of the default build in the differential guard (NativeSolver).
    ``band=(ml, mu)``: band storage and band LU of the Newton matrix in the memory-resident mapping (csrc/bdf_mem.hip,
    SA_BAND_ML / SA_BAND_MU: a separate code object); the caller vouches that the Jacobian has no entry outside it."""
    os.makedirs(_CACHE, exist_ok=True)
    out = code_object_path(native_source, sens, constraints, hermite, compact, safe, group, band)
    if os.path.exists(out) and not force:
        return out
    fname, group = kernel_variant(native_source, sens, constraints, hermite, group=group)
    band = _band_widths(native_source, fname, band)
    band_defines = ["-DSA_BAND_ML=%d" % band[0], "-DSA_BAND_MU=%d" % band[1]] if band is not None else []
    kern = os.path.join(_CSRC, fname)
    hdr = out[:-6] + ".h"
    with open("%s.tmp%d" % (hdr, os.getpid()), "w") as fh:      # (concurrent ranks: private temporaries, atomic renames)
        fh.write(native_source)
    os.replace("%s.tmp%d" % (hdr, os.getpid()), hdr)
    tmp = tempfile.mkdtemp(prefix="sa_build_", dir=_CACHE)
    try:
        bc0, bc1, obj = (os.path.join(tmp, n) for n in ("k0.bc", "k1.bc", "k.o"))
        hipcc = os.path.join(ROCM, "bin", "hipcc")
        _run([hipcc, "--offload-arch=" + ARCH, "--cuda-device-only", "-emit-llvm", "-c", "-O0",
              "-Xclang", "-disable-O0-optnone", "-ffp-contract=off", "-std=c++17",
              "-DSA_PROBLEM_HEADER=\"%s\"" % hdr, "-DSA_GROUP=%d" % group] + _size_defines(native_source)
             + (["-DSA_SENS=1"] if sens else []) + (["-DSA_CONSTRAINTS=1"] if constraints else [])
             + (["-DSA_HERMITE=1"] if hermite else []) + (["-DSA_COMPACT_TRAJ=1"] if compact else []) + band_defines
             + ["-I" + _CSRC, kern, "-o", bc0])
        _run([os.path.join(LLVM_BIN, "opt"), "-passes=always-inline,sroa", bc0, "-o", bc1])
        occupancy = os.environ.get("SA_WAVES_PER_EU")
        if occupancy:
            # tuning: cap the register budget of EVERY function (the noinline callbacks included; the
            # launch-bounds attribute only reaches the kernels) so that `occupancy` waves fit a SIMD
            ll = os.path.join(tmp, "k1.ll")
            _run([os.path.join(LLVM_BIN, "llvm-dis"), bc1, "-o", ll])
            with open(ll) as fh:
                text = fh.read()
            import re
            text = re.sub(r'^(attributes #\d+ = \{.*) \}$',
                          r'\1 "amdgpu-waves-per-eu"="%s,%s" }' % (occupancy, occupancy), text, flags=re.M)
            with open(ll, "w") as fh:
                fh.write(text)
            bc1 = ll            # clang -x ir reads the textual form as well
        base = [os.path.join(LLVM_BIN, "clang"), "-x", "ir", bc1, "-target", "amdgcn-amd-amdhsa",
                "-mcpu=" + ARCH, "-O3", "-ffp-contract=off"]
        # the memory-resident build is dominated by the generated callbacks (10^4 statements at
        # n = 100): default scheduler there, the ILP strategies take several times longer
        extra = _extra_codegen_flags()
        if "SA_CLANG_FLAGS" not in os.environ:
            if fname == "bdf_kernels.hip":
                extra = extra + ([] if sens else ADJOINT_CODEGEN_FLAGS.split())
            elif fname == "bdf_wave.hip":
                extra = ([] if sens else (WAVE_CODEGEN_FLAGS + " " + ADJOINT_CODEGEN_FLAGS
                                          + (" " + SMALL_GROUP_CODEGEN_FLAGS if group <= 8 else "")).split())
            else:
                extra = []
        extra = extra + _safety_flags(safe)          # (also on top of SA_CLANG_FLAGS: the guard's partner of a tuning build)
        try:
            _run(base + extra + ["-c", "-o", obj])
        except NativeBuildError:
            if extra == _safety_flags(safe):
                raise
            # the non-default scheduler strategies crash clang on very large kernels: plain -O3 then
            _run(base + _safety_flags(safe) + ["-c", "-o", obj])
        _run([os.path.join(LLVM_BIN, "ld.lld"), "-shared", obj, "-o", "%s.tmp%d" % (out, os.getpid())])
        os.replace("%s.tmp%d" % (out, os.getpid()), out)
    finally:
        if not keep_temps:
            shutil.rmtree(tmp, ignore_errors=True)
    return out


#: fields of a kernel's code-object notes that the budget (profiles/code_object_budget.json) bounds
NOTE_FIELDS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
               "group_segment_fixed_size")


def code_object_notes(path: str) -> dict:
    """{kernel name: {field: value}} from the AMDGPU metadata notes of a code object (llvm-readelf --notes):
    registers, spill slots, scratch bytes per lane and static LDS of every kernel in it."""
    import re
    text = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", path], capture_output=True, text=True,
                          check=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", "\n" + text)[1:]:
        block = "    .agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        row = {}
        for f in NOTE_FIELDS:
            m = re.search(r"\.%s:\s+(\d+)" % f, block)
            if m:
                row[f] = int(m.group(1))
        out[name.group(1)] = row
    return out


def code_object_meta(path: str) -> dict:
    """The ``sa_meta`` record of a code object, read from the file (no GPU): n_states, n_sub, n_rem, abi, lanes per
    instance and ``ws_doubles``, the per-instance workspace the host library allocates for it."""
    import struct
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:6] != b"\x7fELF\x02\x01":
        raise ValueError("%s is not a little-endian ELF64 file" % path)
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + k * shentsize) for k in range(shnum)]
    for _name, stype, _flags, _addr_, off, size, link, _info, _align, entsize in sections:
        if stype not in (2, 11) or not entsize:           # SHT_SYMTAB / SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for k in range(size // entsize):
            st_name, _st_info, _other, shndx, value, st_size = struct.unpack_from("<IBBHQQ", data, off + k * entsize)
            end = data.index(b"\0", str_off + st_name)
            if data[str_off + st_name:end] == b"sa_meta" and 0 < shndx < shnum and st_size >= 24:
                sec = sections[shndx]
                vals = struct.unpack_from("<6i", data, sec[4] + (value - sec[3]))
                return dict(zip(("n_states", "n_sub", "n_rem", "abi", "lanes", "ws_doubles"), vals))
    raise ValueError("no sa_meta symbol in %s" % path)


def toolchain_id() -> dict:
    """What compiled the code objects: the version banners of hipcc / clang and a short hash of them (bench.py prints
    it next to the counter-traffic source so that a profile taken with another toolchain is detectable)."""
    banners = []
    for exe in (os.path.join(ROCM, "bin", "hipcc"), os.path.join(LLVM_BIN, "clang")):
        try:
            banners.append(subprocess.run([exe, "--version"], capture_output=True, text=True).stdout.strip())
        except OSError:
            banners.append("%s: not found" % exe)
    text = "\n".join(banners)
    first = [ln for ln in text.splitlines() if "version" in ln.lower()]
    return {"hash": hashlib.sha256(text.encode()).hexdigest()[:12], "banner": "; ".join(first[:2])}


def file_hash(path: str) -> str:
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()[:12]


def check_code_object_budget(label: str, path: str, budget: dict) -> list:
    """Violations (strings) of ``budget`` = {kernel: {field: ceiling}} by the code object at ``path``."""
    notes = code_object_notes(path)
    bad = []
    for kernel, limits in budget.items():
        if kernel not in notes:
            bad.append("%s: kernel %s missing from %s" % (label, kernel, os.path.basename(path)))
            continue
        for field, ceiling in limits.items():
            got = notes[kernel].get(field)
            if got is None or got > ceiling:
                bad.append("%s: %s.%s = %s exceeds the budget %s" % (label, kernel, field, got, ceiling))
    return bad


# ----------------------------------------------------------------------------------------------
# differential guard (include/sunode_amd.h: sa_solver_attach_guard)
# ----------------------------------------------------------------------------------------------
#: kinds of batch call the guard checks separately (bit masks of the C ABI)
GUARD_KINDS = {"plain": 1, "adjoint": 2, "sens": 4}
GUARD_RECHECK_OPEN = 0x80000000     # sa_guard_state `pending`: a verified kind may still be re-checked
GUARD_PERSIST_MIN = 16              # smallest sample whose "identical" verdict is written next to the code object


def guard_enabled() -> bool:
    """The guard is ON unless SA_GUARD=0 -- or every build is the conservative one anyway."""
    return os.environ.get("SA_GUARD", "1") != "0" and not all_builds_conservative()


def guard_verdict_path(code_object: str) -> str:
    return code_object[:-len(".hsaco")] + ".guard.json"


def read_guard_verdict(code_object: str, safe_object: str) -> dict:
    """{kind: {"verdict": "identical" | "differs", "n_sample": k}} recorded for this pair of code objects by an
    earlier process (same toolchain), else {}."""
    import json
    try:
        with open(guard_verdict_path(code_object)) as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        return {}
    if doc.get("default") != os.path.basename(code_object) or doc.get("conservative") != os.path.basename(safe_object) \
            or doc.get("toolchain") != toolchain_id()["hash"]:
        return {}
    return doc.get("kinds", {})


def write_guard_verdict(code_object: str, safe_object: str, kinds: dict, detail: str = "") -> None:
    import json
    doc = {"default": os.path.basename(code_object), "conservative": os.path.basename(safe_object),
           "toolchain": toolchain_id()["hash"], "kinds": kinds, "detail": detail,
           "note": "differential guard: first instances of the first batch through both builds, statuses / counters / "
                   "outputs compared bit for bit on the device (include/sunode_amd.h, sa_solver_attach_guard)"}
    import threading
    # (several handles of one solver object report from their own host threads: private temporaries, atomic renames)
    tmp = "%s.tmp%d_%d" % (guard_verdict_path(code_object), os.getpid(), threading.get_ident())
    try:
        with open(tmp, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
        os.replace(tmp, guard_verdict_path(code_object))
    except OSError:
        pass            # a read-only cache: the check simply runs again next time


class _Options(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("device", ctypes.c_int32), ("rtol", ctypes.c_double),
                ("atol", ctypes.POINTER(ctypes.c_double)), ("rtolB", ctypes.c_double), ("atolB", ctypes.c_double),
                ("rtolQB", ctypes.c_double), ("atolQB", ctypes.c_double), ("mxstep", ctypes.c_int32),
                ("max_retries_fwd", ctypes.c_int32), ("max_retries_bwd", ctypes.c_int32),
                ("traj_capacity", ctypes.c_int32), ("constraints", ctypes.POINTER(ctypes.c_double)),
                ("arena_bytes", ctypes.c_int64)]


_LIB: Optional[ctypes.CDLL] = None

_dp = ctypes.c_void_p     # raw addresses: host numpy buffers or device pointers


def load_library() -> ctypes.CDLL:
    """dlopen libsunode_amd.so and declare every symbol of include/sunode_amd.h."""
    global _LIB
    if _LIB is not None:
        return _LIB
    L = ctypes.CDLL(build_host_library())
    i32, i64, dbl, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    L.sa_abi_version.restype = ctypes.c_int
    L.sa_last_error.restype = ctypes.c_char_p
    L.sa_solver_create.argtypes = [ctypes.c_char_p, ctypes.POINTER(_Options), ctypes.POINTER(vp)]
    L.sa_solver_destroy.argtypes = [vp]
    L.sa_solver_destroy.restype = None
    L.sa_solver_set_options.argtypes = [vp, ctypes.POINTER(_Options)]
    L.sa_solver_sizes.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    fwd = [vp, ctypes.c_int, i32, _dp, _dp, _dp, i32, dbl, _dp, i32, _dp, _dp, _dp]
    L.sa_solve_batch.argtypes = fwd
    L.sa_solve_forward_batch.argtypes = fwd
    L.sa_solve_backward_batch.argtypes = [vp, ctypes.c_int, i32, _dp, _dp, i32, dbl, dbl, _dp, i32, _dp, i64,
                                          _dp, _dp, _dp, _dp]
    L.sa_solve_sens_batch.argtypes = [vp, ctypes.c_int, ctypes.c_int, _dp, i32, _dp, _dp, _dp, i32, _dp, dbl, _dp,
                                      i32, _dp, _dp, _dp, _dp]
    L.sa_solve_backward_batch_all.argtypes = [vp, ctypes.c_int, i32, _dp, _dp, i32, dbl, dbl, _dp, i32, _dp, i64,
                                              _dp, _dp, _dp, _dp, _dp, _dp]
    fwd_t = [vp, ctypes.c_int, i32, _dp, _dp, _dp, i32, _dp, i32, _dp, i64, i32, _dp, _dp, _dp]
    L.sa_solve_batch_times.argtypes = fwd_t
    L.sa_solve_forward_batch_times.argtypes = fwd_t
    L.sa_solve_sens_batch_times.argtypes = [vp, ctypes.c_int, ctypes.c_int, _dp, i32, _dp, _dp, _dp, i32, _dp, _dp,
                                            i32, _dp, i64, i32, _dp, _dp, _dp, _dp]
    L.sa_solve_backward_batch_times.argtypes = [vp, ctypes.c_int, i32, _dp, _dp, i32, _dp, i32, _dp, i32, _dp, i64,
                                                i32, _dp, i64, _dp, _dp, _dp, _dp, _dp, _dp]
    L.sa_eval_callbacks.argtypes = [vp, ctypes.c_int, i32] + [_dp] * 11
    L.sa_math_probe.argtypes = [vp, i32] + [_dp] * 5
    L.sa_plan_tiles.argtypes = [i32, _dp, i64, i64, _dp, _dp, ctypes.POINTER(i32), _dp, ctypes.POINTER(i32),
                                ctypes.POINTER(i32)]
    L.sa_arena_info.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32)]
    L.sa_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.sa_device_count.argtypes = [ctypes.POINTER(i32)]
    L.sa_device_memory.argtypes = [i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.sa_set_stream.argtypes = [vp, vp]
    L.sa_synchronize.argtypes = [vp]
    u32 = ctypes.c_uint32
    L.sa_solver_attach_guard.argtypes = [vp, ctypes.c_char_p, i32, u32]
    L.sa_guard_state.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32),
                                 ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_char_p)]
    for name in ("sa_solver_attach_guard", "sa_guard_state", "sa_solver_create", "sa_solver_set_options", "sa_solver_sizes", "sa_solve_batch", "sa_solve_sens_batch",
                 "sa_solve_forward_batch", "sa_solve_backward_batch", "sa_solve_backward_batch_all",
                 "sa_solve_batch_times", "sa_solve_forward_batch_times", "sa_solve_sens_batch_times",
                 "sa_solve_backward_batch_times", "sa_eval_callbacks", "sa_math_probe", "sa_last_kernel_ms", "sa_set_stream", "sa_synchronize",
                 "sa_plan_tiles", "sa_arena_info", "sa_device_count", "sa_device_memory"):
        getattr(L, name).restype = ctypes.c_int
    _LIB = L
    return L


EXPORTED_SYMBOLS = ["sa_abi_version", "sa_last_error", "sa_solver_create", "sa_solver_destroy",
                    "sa_solver_set_options", "sa_solver_sizes", "sa_solve_batch", "sa_solve_sens_batch",
                    "sa_solve_forward_batch",
                    "sa_solve_backward_batch", "sa_solve_backward_batch_all",
                    "sa_solve_batch_times", "sa_solve_forward_batch_times", "sa_solve_sens_batch_times",
                    "sa_solve_backward_batch_times", "sa_eval_callbacks", "sa_math_probe", "sa_plan_tiles",
                    "sa_last_kernel_ms", "sa_arena_info",
                    "sa_set_stream", "sa_synchronize", "sa_device_count", "sa_device_memory",
                    "sa_solver_attach_guard", "sa_guard_state"]


class NativeError(RuntimeError):
    pass


def device_count() -> int:
    """HIP devices visible to the library (include/sunode_amd.h: sa_device_count)."""
    L = load_library()
    n = ctypes.c_int32()
    if L.sa_device_count(ctypes.byref(n)) != 0:
        raise NativeError("sa_device_count: %s" % L.sa_last_error().decode())
    return n.value


def device_memory(device: int):
    """(free, total) bytes of HBM on ``device`` (sa_device_memory)."""
    L = load_library()
    f, t = ctypes.c_int64(), ctypes.c_int64()
    if L.sa_device_memory(int(device), ctypes.byref(f), ctypes.byref(t)) != 0:
        raise NativeError("sa_device_memory: %s" % L.sa_last_error().decode())
    return f.value, t.value


def _addr(x) -> int:
    """Address of a numpy array (host) or pass-through of an int device pointer."""
    if x is None:
        return 0
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if hasattr(x, "data_ptr"):            # torch tensor
        return int(x.data_ptr())
    raise TypeError("unsupported buffer type %r" % type(x))


class NativeSolver:
    """One ``sa_solver`` handle: a problem's code object loaded on one GPU."""

    def __init__(self, native_source: str, *, device: int = 0, rtol=1e-10, atol=1e-10, rtolB=1e-10,
                 atolB=1e-10, rtolQB=1e-10, atolQB=1e-10, mxstep=500, max_retries_fwd=5,
                 max_retries_bwd=50, traj_capacity=500_001, n_states: Optional[int] = None, sens: bool = False,
                 constraints=None, hermite: bool = False, arena_bytes: int = 0, compact: bool = False,
                 guard: Optional[bool] = None, guard_sample: int = 64, guard_kinds=None, group: Optional[str] = None,
                 band=None):
        """``guard`` (default: on, SA_GUARD=0 turns it off): the differential guard -- the conservative build of the
        same source is compiled next to the default one and a sample of the first batch of every kind of call (chosen
        from the batch's own statuses and counters, include/sunode_amd.h) runs through both on the device; any
        difference in statuses, counters or outputs makes the handle use the conservative build (RuntimeWarning), and
        the verdict is kept next to the code object.  ``guard_kinds``: the kinds of call this handle will make
        (``("adjoint",)`` under an AdjointSolver, ``("plain",)`` / ``("sens",)`` under a Solver; default: all) --
        kinds it never runs are not left pending, so the shadow handles go away once the used kind is verified."""
        self.L = load_library()
        build_kw = dict(sens=sens, constraints=constraints is not None, hermite=hermite, compact=compact, group=group)
        if band is not None:        # (ml, mu): the band build; the guard's conservative partner gets the same defines
            build_kw["band"] = tuple(int(w) for w in band)
        self.variant = kernel_variant(native_source, sens, constraints is not None, hermite, group=group)
        self._guard_open = False
        self._guard_safe = None
        self.guard_report = {"enabled": False}
        if guard_enabled() if guard is None else bool(guard):
            todo = [dict(build_kw), dict(build_kw, safe=True)]
            if not all(os.path.exists(code_object_path(native_source, **kw)) for kw in todo):
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(max_workers=2) as pool:          # both builds at once (compiler subprocesses)
                    list(pool.map(lambda kw: build_code_object(native_source, **kw), todo))
            self._guard_fast = build_code_object(native_source, **build_kw)
            self._guard_safe = build_code_object(native_source, **todo[1])
            self._guard_kinds = read_guard_verdict(self._guard_fast, self._guard_safe)
            self.guard_report = {"enabled": True, "default": os.path.basename(self._guard_fast),
                                 "conservative": os.path.basename(self._guard_safe), "kinds": dict(self._guard_kinds),
                                 "using_conservative": False}
        self.code_object = build_code_object(native_source, **build_kw)
        if self._guard_safe and any(v.get("verdict") == "differs" for v in self._guard_kinds.values()):
            import warnings
            warnings.warn("sunode_amd: the default and the conservative build of this model gave different results in "
                          "an earlier run (%s); using the conservative build %s"
                          % (guard_verdict_path(self._guard_fast), os.path.basename(self._guard_safe)),
                          RuntimeWarning, stacklevel=3)
            self.code_object = self._guard_safe
            self.guard_report["using_conservative"] = True
            self._guard_safe = None                 # nothing left to compare
        self._h = ctypes.c_void_p()
        self._user_stream = False
        self._n_hint = n_states
        self._opt_kw = dict(device=device, rtol=rtol, atol=atol, rtolB=rtolB, atolB=atolB, rtolQB=rtolQB,
                            atolQB=atolQB, mxstep=mxstep, max_retries_fwd=max_retries_fwd,
                            max_retries_bwd=max_retries_bwd, traj_capacity=traj_capacity, constraints=constraints,
                            arena_bytes=arena_bytes)
        opt, keep = self._make_options(n_states if n_states is not None else 64)
        rc = self.L.sa_solver_create(self.code_object.encode(), ctypes.byref(opt), ctypes.byref(self._h))
        self._check(rc)
        n, p, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self.L.sa_solver_sizes(self._h, ctypes.byref(n), ctypes.byref(p), ctypes.byref(r)))
        self.n, self.p, self.r = n.value, p.value, r.value
        self.set_options()
        if self._guard_safe:
            used = set(GUARD_KINDS) if guard_kinds is None else set(guard_kinds)
            if not used <= set(GUARD_KINDS):
                raise ValueError("guard_kinds must be some of %s" % sorted(GUARD_KINDS))
            verified = sum(bit for kind, bit in GUARD_KINDS.items()
                           if self._guard_kinds.get(kind, {}).get("verdict") == "identical")
            unused = sum(bit for kind, bit in GUARD_KINDS.items() if kind not in used)
            self.guard_report["checked_kinds"] = sorted(used)
            self._check(self.L.sa_solver_attach_guard(self._h, self._guard_safe.encode(), int(guard_sample),
                                                      verified | unused))
            self._guard_unused = unused
            self._guard_seen = (verified | unused, 0)
            self._guard_open = True
            self._guard_poll()

    def _make_options(self, n):
        kw = self._opt_kw
        atol = np.ascontiguousarray(np.broadcast_to(np.asarray(kw["atol"], dtype=np.float64), (max(n, 1),)))
        opt = _Options()
        opt.struct_size = ctypes.sizeof(_Options)
        opt.device = kw["device"]
        opt.rtol = float(kw["rtol"])
        opt.atol = atol.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        opt.rtolB, opt.atolB = float(kw["rtolB"]), float(kw["atolB"])
        opt.rtolQB, opt.atolQB = float(kw["rtolQB"]), float(kw["atolQB"])
        opt.mxstep, opt.max_retries_fwd = int(kw["mxstep"]), int(kw["max_retries_fwd"])
        opt.max_retries_bwd, opt.traj_capacity = int(kw["max_retries_bwd"]), int(kw["traj_capacity"])
        opt.arena_bytes = int(kw.get("arena_bytes") or 0)
        cons = None
        if kw.get("constraints") is not None:
            cons = np.ascontiguousarray(np.broadcast_to(np.asarray(kw["constraints"], dtype=np.float64), (max(n, 1),)))
            opt.constraints = cons.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        return opt, (atol, cons)

    def set_options(self, **kw):
        self._opt_kw.update(kw)
        opt, keep = self._make_options(self.n)
        self._check(self.L.sa_solver_set_options(self._h, ctypes.byref(opt)))

    def _check(self, rc):
        if rc != 0:
            raise NativeError("sunode_amd native call failed (%d): %s" % (rc, self.L.sa_last_error().decode()))

    def guard_state(self):
        """dict(pending, verified, differs: lists of kind names; using_conservative; n_sample {kind: k}; detail)."""
        u32, i32 = ctypes.c_uint32, ctypes.c_int32
        pend, ver, dif, safe = u32(), u32(), u32(), i32()
        ns = (i32 * 3)()
        detail = ctypes.c_char_p()
        self._check(self.L.sa_guard_state(self._h, ctypes.byref(pend), ctypes.byref(ver), ctypes.byref(dif),
                                          ctypes.byref(safe), ns, ctypes.byref(detail)))
        names = lambda m: [k for k, bit in GUARD_KINDS.items() if m & bit]          # noqa: E731
        unused = getattr(self, "_guard_unused", 0)
        return dict(pending=names(pend.value), verified=names(ver.value & ~unused), differs=names(dif.value),
                    using_conservative=bool(safe.value), n_sample=dict(zip(GUARD_KINDS, list(ns))),
                    recheck_open=bool(pend.value & GUARD_RECHECK_OPEN),
                    detail=(detail.value or b"").decode(), _masks=(ver.value, dif.value))

    def _guard_poll(self):
        """After a batch call while checks are pending: persist new verdicts, warn about a difference."""
        if not self._guard_open:
            return
        st = self.guard_state()
        if st["_masks"] != self._guard_seen:
            self._guard_seen = st["_masks"]
            for kind in st["verified"]:
                if st["n_sample"][kind]:          # (kinds verified by an earlier process keep their record)
                    self._guard_kinds[kind] = {"verdict": "identical", "n_sample": st["n_sample"][kind]}
            for kind in st["differs"]:
                self._guard_kinds[kind] = {"verdict": "differs", "n_sample": st["n_sample"][kind]}
            # on disk: a difference always; "identical" only from a sample of at least GUARD_PERSIST_MIN instances
            # (a verdict from three batches of one draw stays with this process -- ADVICE r5)
            keep = {k: v for k, v in self._guard_kinds.items()
                    if v["verdict"] == "differs" or v.get("n_sample", 0) >= GUARD_PERSIST_MIN}
            if keep:
                write_guard_verdict(self._guard_fast, self._guard_safe, keep, st["detail"])
            self.guard_report.update(kinds=dict(self._guard_kinds), using_conservative=st["using_conservative"],
                                     detail=st["detail"])
            if st["differs"]:
                import warnings
                warnings.warn("sunode_amd differential guard: %s -- this solver now runs the conservative build (a "
                              "difference found in a backward pass repeats this batch's forward pass internally; "
                              "forward outputs already returned to the caller came from the default build and are "
                              "not recomputed); the verdict is recorded in %s"
                              % (st["detail"], guard_verdict_path(self._guard_fast)), RuntimeWarning, stacklevel=4)
                self.code_object = self._guard_safe
        if not st["pending"] and not st["recheck_open"]:
            self._guard_open = False

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.L.sa_solver_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- stream ordering (include/sunode_amd.h): the handle launches on its own non-blocking stream unless the caller
    #    hands it one with set_stream().  When torch tensors come in and no stream was set, the safe default is to
    #    order by synchronising: torch's current stream before the launch, the solver's stream after it.
    def _torch_guard(self, *arrays):
        if self._user_stream or not any(getattr(a, "is_cuda", False) for a in arrays):
            return None
        import torch
        torch.cuda.current_stream().synchronize()
        return self.synchronize

    # -- raw entry points (addresses or numpy arrays; shapes are the caller's responsibility) --
    # Time arguments: a Python number / 0-d array t0 (tend) and a 1-d grid go through the shared-grid entry points as
    # before; ``t0_stride`` / ``tend_stride`` / ``tvals_stride`` not None select the per-instance entry points
    # (include/sunode_amd.h sa_*_batch_times) with t0 (tend, tvals) an array or device pointer and that stride.
    @staticmethod
    def _time_arg(x, stride, mem):
        """(buffer, stride) of one time argument of a per-instance entry point: a number becomes a one-element host
        array (stride 0) -- the caller keeps the buffer alive across the call."""
        if stride is None:
            if mem != SA_MEM_HOST:
                raise ValueError("a shared time of a device-memory call must be a one-element device array (stride 0)")
            return np.asarray([x], dtype=np.float64), 0
        if isinstance(x, (np.ndarray, int, np.integer)) or hasattr(x, "data_ptr"):
            return x, int(stride)
        raise TypeError("a per-instance time argument must be an array, a tensor or a device pointer")

    def solve(self, mem, B, y0, ps, pr, rem_stride, t0, tvals, n_t, y_out, status, stats, adjoint=False,
              t0_stride=None, tvals_stride=None):
        done = self._torch_guard(y0, ps, pr, tvals, y_out, status, stats, t0)
        if t0_stride is None and tvals_stride is None:
            fn = self.L.sa_solve_forward_batch if adjoint else self.L.sa_solve_batch
            rc = fn(self._h, mem, B, _addr(y0), _addr(ps), _addr(pr), rem_stride, float(t0), _addr(tvals),
                    n_t, _addr(y_out), _addr(status), _addr(stats))
        else:
            fn = self.L.sa_solve_forward_batch_times if adjoint else self.L.sa_solve_batch_times
            t0b, t0s = self._time_arg(t0, t0_stride, mem)
            rc = fn(self._h, mem, B, _addr(y0), _addr(ps), _addr(pr), rem_stride, _addr(t0b), t0s,
                    _addr(tvals), int(tvals_stride or 0), n_t, _addr(y_out), _addr(status), _addr(stats))
        self._check(rc)
        if done:
            done()
        if self._guard_open:
            self._guard_poll()

    def solve_backward(self, mem, B, ps, pr, rem_stride, t0, tend, tvals, n_t, grads, grads_stride, grad_out,
                       lamda_out, status, stats, lamda_all=None, quad_all=None, t0_stride=None, tend_stride=None,
                       tvals_stride=None):
        done = self._torch_guard(ps, pr, tvals, grads, grad_out, lamda_out, status, stats, t0, tend)
        if t0_stride is None and tend_stride is None and tvals_stride is None:
            rc = self.L.sa_solve_backward_batch_all(
                self._h, mem, B, _addr(ps), _addr(pr), rem_stride, float(t0), float(tend), _addr(tvals), n_t,
                _addr(grads), int(grads_stride), _addr(grad_out), _addr(lamda_out), _addr(lamda_all), _addr(quad_all),
                _addr(status), _addr(stats))
        else:
            t0b, t0s = self._time_arg(t0, t0_stride, mem)
            teb, tes = self._time_arg(tend, tend_stride, mem)
            rc = self.L.sa_solve_backward_batch_times(
                self._h, mem, B, _addr(ps), _addr(pr), rem_stride, _addr(t0b), t0s, _addr(teb), tes,
                _addr(tvals), int(tvals_stride or 0), n_t, _addr(grads), int(grads_stride),
                _addr(grad_out), _addr(lamda_out), _addr(lamda_all), _addr(quad_all), _addr(status), _addr(stats))
        self._check(rc)
        if done:
            done()
        if self._guard_open:
            self._guard_poll()

    def solve_sens(self, mem, ism, scaling, B, y0, ps, pr, rem_stride, sens0, t0, tvals, n_t, y_out, sens_out,
                   status, stats, t0_stride=None, tvals_stride=None):
        done = self._torch_guard(y0, ps, pr, sens0, tvals, y_out, sens_out, status, stats, t0)
        if t0_stride is None and tvals_stride is None:
            rc = self.L.sa_solve_sens_batch(self._h, mem, int(ism), _addr(scaling), B, _addr(y0), _addr(ps),
                                            _addr(pr), rem_stride, _addr(sens0), float(t0), _addr(tvals), n_t,
                                            _addr(y_out), _addr(sens_out), _addr(status), _addr(stats))
        else:
            t0b, t0s = self._time_arg(t0, t0_stride, mem)
            rc = self.L.sa_solve_sens_batch_times(self._h, mem, int(ism), _addr(scaling), B, _addr(y0), _addr(ps),
                                                  _addr(pr), rem_stride, _addr(sens0), _addr(t0b), t0s,
                                                  _addr(tvals), int(tvals_stride or 0), n_t,
                                                  _addr(y_out), _addr(sens_out), _addr(status), _addr(stats))
        self._check(rc)
        if done:
            done()
        if self._guard_open:
            self._guard_poll()

    def eval_callbacks(self, t, y, lam, ps, pr):
        npts = len(t)
        n, p, r = self.n, self.p, self.r
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (t, y, lam, ps, pr)]
        rhs = np.zeros((npts, n)); jac = np.zeros((npts, n * n)); adj = np.zeros((npts, n))
        quad = np.zeros((npts, p)); adjjac = np.zeros((npts, n * n)); codes = np.zeros((npts, 5), np.int32)
        self._check(self.L.sa_eval_callbacks(self._h, SA_MEM_HOST, npts, *[_addr(a) for a in arrs], _addr(rhs),
                                             _addr(jac), _addr(adj), _addr(quad), _addr(adjjac), _addr(codes)))
        return dict(rhs=rhs, jac=jac.reshape(npts, n, n).transpose(0, 2, 1).copy(), adj=adj, quad=quad,
                    adjjac=adjjac.reshape(npts, n, n).transpose(0, 2, 1).copy(), codes=codes)

    def math_probe(self, x, y):
        x = np.ascontiguousarray(x, np.float64); y = np.ascontiguousarray(y, np.float64)
        out = [np.zeros_like(x) for _ in range(3)]
        self._check(self.L.sa_math_probe(self._h, len(x), _addr(x), _addr(y), *[_addr(o) for o in out]))
        return out

    def last_kernel_ms(self):
        f, b = ctypes.c_float(), ctypes.c_float()
        self._check(self.L.sa_last_kernel_ms(self._h, ctypes.byref(f), ctypes.byref(b)))
        return f.value, b.value

    def arena_info(self):
        """(bytes of the largest trajectory-arena allocation used, tiles re-integrated so far, last batch tiled?)"""
        b, t, f = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        self._check(self.L.sa_arena_info(self._h, ctypes.byref(b), ctypes.byref(t), ctypes.byref(f)))
        return b.value, t.value, bool(f.value)

    def set_stream(self, stream_ptr):
        """Launch on the caller's HIP stream (e.g. ``torch.cuda.Stream().cuda_stream``); 0 / None: back to the
        library-owned stream."""
        self._check(self.L.sa_set_stream(self._h, ctypes.c_void_p(stream_ptr or 0)))
        self._user_stream = bool(stream_ptr)

    def synchronize(self):
        self._check(self.L.sa_synchronize(self._h))
