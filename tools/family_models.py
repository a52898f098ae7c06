"""The integrated models of the function families: one record per model, read by ``__graft_entry__.build()`` (which
code objects to compile), tools/make_golden_truth.py (which truth fixtures to write) and the GPU tests (which mappings to
force) -- so a mapping that is tested is a mapping that is built.  Kept out of tests/: the build must not import the
test package.
"""
import functools
from typing import Callable, NamedTuple, Optional, Tuple

from tools import problems as P


class FamilyModel(NamedTuple):
    name: str
    batch: Callable                     # batch(B) -> the model's B-draw batch (tools/problems.py)
    truth_draws: Optional[int]          # draws of tests/golden/truth_<name>.npz; None: no truth fixture
    conservative: bool = False          # the differential guard's conservative partner is built
    sens: bool = False                  # a forward-sensitivity build (Solver(sens_mode=...)) is needed
    hermite: bool = False               # a Hermite-interpolation build is needed
    mappings: Tuple[str, ...] = ()      # the values of SA_FORCE_GROUP the tests force, next to the engine's own mapping


def _threshold_sir(M):
    return FamilyModel("threshold_sir%d" % M, functools.partial(P.threshold_sir_batch, M=M), 8 if M == 8 else None,
                       mappings={4: ("wave8",), 8: ("wave",), 16: ("wave", "mem")}[M])


FAMILY_MODELS = (
    # transcendental right-hand sides / the reference's helper functions (tests/test_gpu_transcendental.py)
    FamilyModel("forcing", P.forcing_batch, 8, conservative=True, sens=True, mappings=("wave4", "wave16", "wave", "mem")),
    FamilyModel("logistic_switch", P.logistic_switch_batch, 8, conservative=True, mappings=("mem",)),
    FamilyModel("misc", P.misc_batch, 8, conservative=True, mappings=("wave8",)),
    # inverse trigonometric / hyperbolic functions, erf / erfc; gamma family; Bessel functions (tests/test_gpu_inverse_erf.py,
    # test_gpu_gamma.py, test_gpu_bessel.py)
    FamilyModel("probit_gate", P.probit_gate_batch, 16, conservative=True, sens=True, mappings=("wave4", "wave", "mem")),
    FamilyModel("gamma_delay", P.gamma_delay_batch, 16, conservative=True, sens=True, mappings=("wave4", "wave", "mem")),
    FamilyModel("bessel_ring", P.bessel_ring_batch, 16, conservative=True, sens=True, mappings=("wave4", "wave", "mem")),
    # erfinv / erfcinv / incomplete gamma functions (tests/test_gpu_prob.py)
    FamilyModel("quantile_delay", P.quantile_delay_batch, 16, conservative=True, sens=True, mappings=("wave4", "wave", "mem")),
    # non-smooth right-hand sides (tests/test_gpu_nonsmooth.py)
    FamilyModel("kinked", P.kinked_batch, 8, sens=True, hermite=True, mappings=("wave4", "wave8", "wave", "mem")),
    _threshold_sir(4), _threshold_sir(8), _threshold_sir(16),
)
FAMILY = {model.name: model for model in FAMILY_MODELS}
