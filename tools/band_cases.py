"""The band builds (``linear_solver="band"``, csrc/bdf_mem.hip under SA_BAND_ML / SA_BAND_MU) that tests/test_band.py and
tests/test_gpu_band.py run: ``__graft_entry__.build()`` pre-compiles them, with the dense memory-resident builds they are
compared with, the differential guard's conservative partner and the oracle libraries of the new models.

(model, SA_FORCE_GROUP or None, build_code_object keywords): small models reach the memory-resident mapping through
``SA_FORCE_GROUP=mem``; ``chain256`` and ``brusselator1d_65`` (130 states) get there by themselves."""

BAND_BUILDS = [
    # brusselator1d(6), n = 12, (ml, mu) = (2, 2): band and dense, over-declared, Hermite, the guard's partner
    ("brusselator1d_6", "mem", {}),
    ("brusselator1d_6", "mem", {"band": (2, 2)}),
    ("brusselator1d_6", "mem", {"band": (2, 2), "safe": True}),
    ("brusselator1d_6", "mem", {"band": (3, 4)}),
    ("brusselator1d_6", "mem", {"hermite": True}),
    ("brusselator1d_6", "mem", {"hermite": True, "band": (2, 2)}),
    # row exchanges inside a tridiagonal band / a nearly full band
    ("pivoting_band", "mem", {"band": (1, 1)}),
    ("pivoting", "mem", {"band": (5, 1)}),
    # Solver: plain solves and forward sensitivities
    ("brusselator1d_3", "mem", {"band": (2, 2)}),
    ("brusselator1d_3", "mem", {"band": (2, 2), "sens": True}),
    # the natural path
    ("chain256", None, {"band": (1, 0)}),
    ("brusselator1d_65", None, {"band": (2, 2)}),
]

#: models whose oracle library the tests need and no other part of the build compiles
BAND_ORACLES = ["brusselator1d_3", "brusselator1d_6", "brusselator1d_65", "pivoting_band"]
