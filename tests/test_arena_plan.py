"""The trajectory-arena plan of a batch that is not resident (csrc/sunode_amd.cpp plan_tiles, through the test hook
sa_plan_tiles) against a plain Python reference: which instances are taken out, where the tile cuts fall.

The plan decides how many records every tile's launch may write into the arena, so an off-by-one at a group boundary
or an over-budget tile is an out-of-bounds arena write on the device; this is its integer arithmetic alone, on the CPU.

Budgets are at least two rows of one 64-instance group (2 * 64 * record bytes): every store-mode launch has two rows,
so below that no plan can fit and the property "every tile fits" has no meaning."""
import ctypes
import itertools

import numpy as np
import pytest

SIZES = [1, 63, 64, 65, 128, 129, 200, 1000]


def _round64(v):
    return (v + 63) // 64 * 64


def plan(counts, rec, budget):
    """sa_plan_tiles: (counts with the taken-out instances zeroed, their indices, cuts, balanced?)"""
    from sunode_amd import _native
    L = _native.load_library()
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    B = len(counts)
    out = np.full(B, -7, np.int32)
    full = np.full(max(B, 1), -7, np.int32)
    cuts = np.full(max((B + 63) // 64, 1) + 1, -7, np.int64)        # (one guard element behind the documented size)
    n_full, n_cuts, bal = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = L.sa_plan_tiles(B, counts.ctypes.data, int(rec), int(budget), out.ctypes.data, full.ctypes.data,
                         ctypes.byref(n_full), cuts.ctypes.data, ctypes.byref(n_cuts), ctypes.byref(bal))
    assert rc == 0, L.sa_last_error().decode()
    assert 0 <= n_cuts.value <= (B + 63) // 64 and cuts[-1] == -7
    assert bal.value in (0, 1)
    return out, full[:n_full.value].tolist(), cuts[:n_cuts.value].tolist(), bool(bal.value)


def _need(lo, hi, kept, rec):
    """bytes of the tile [lo, hi): whole 64-instance groups of its largest count, at least two rows"""
    return _round64(hi - lo) * max(2, int(kept[lo:hi].max(initial=0))) * rec


def _fewest_tiles(B, kept, rec, budget):
    """fewest tiles over ALL contiguous partitions on group boundaries (dynamic programme over the groups)"""
    G = (B + 63) // 64
    best = [0] + [None] * G
    for j in range(1, G + 1):
        hi = min(64 * j, B)
        cands = [best[i] + 1 for i in range(j) if best[i] is not None and _need(64 * i, hi, kept, rec) <= budget]
        best[j] = min(cands) if cands else None
    return best[G]


def _reference_cuts(B, kept, rec, budget):
    """the documented choice: greedy over the groups; the equal-sized alternative when every tile of it fits"""
    cuts, lo = [], 0
    while lo < B:
        hi = min(lo + 64, B)
        while hi < B and _need(lo, min(hi + 64, B), kept, rec) <= budget:
            hi = min(hi + 64, B)
        cuts.append(hi)
        lo = hi
    if len(cuts) > 1:
        per = _round64(-(-B // len(cuts)))
        even = [min(lo + per, B) for lo in range(0, B, per)]
        if len(even) <= len(cuts) and all(_need(lo, hi, kept, rec) <= budget for lo, hi in zip([0] + even, even)):
            return even, True
    return cuts, False


def check(counts, rec, budget):
    counts = np.asarray(counts, dtype=np.int32)
    B = len(counts)
    assert budget >= 2 * 64 * rec
    kept, full, cuts, balanced = plan(counts, rec, budget)
    # taken out: exactly the instances that do not fit a 64-instance group of their own
    want_full = np.flatnonzero(counts > budget // (64 * rec))
    assert full == want_full.tolist()
    want_kept = counts.copy()
    want_kept[want_full] = 0
    np.testing.assert_array_equal(kept, want_kept)
    # cuts: strictly increasing, on group boundaries, ending at B
    assert cuts and cuts[-1] == B
    assert all(a < b for a, b in zip([0] + cuts, cuts))
    assert all(c % 64 == 0 for c in cuts[:-1])
    # every tile fits (the balanced ones as well), and no partition has fewer
    for lo, hi in zip([0] + cuts, cuts):
        assert _need(lo, hi, kept, rec) <= budget, (lo, hi, _need(lo, hi, kept, rec), budget)
    assert len(cuts) == _fewest_tiles(B, kept, rec, budget)
    want_cuts, want_balanced = _reference_cuts(B, kept, rec, budget)
    assert (cuts, balanced) == (want_cuts, want_balanced)
    if balanced:
        sizes = {hi - lo for lo, hi in zip([0] + cuts, cuts[:-1])}
        assert len(sizes) == 1 and cuts[-1] - cuts[-2] <= next(iter(sizes))
    return kept, full, cuts, balanced


@pytest.mark.parametrize("B", SIZES)
def test_seeded_counts(B):
    rng = np.random.default_rng(1000 + B)
    for rec in (24, 160):                               # (compact n = 2, table n = 2: 8 * (8 + 6n))
        for spread in (1.05, 2.0, 20.0):
            counts = np.round(300 * spread ** rng.uniform(-1, 1, B)).astype(np.int32)
            one_group = 64 * rec * int(counts.max())
            for budget in (one_group // 3, one_group - 1, one_group, one_group + 1, int(1.5 * one_group),
                           int(3.3 * one_group), 40 * one_group):
                check(counts, rec, max(budget, 2 * 64 * rec))


@pytest.mark.parametrize("B", SIZES)
def test_all_equal_and_the_exact_boundary(B):
    rec, c = 160, 37
    counts = np.full(B, c, np.int32)
    whole = _round64(B) * c * rec
    kept, full, cuts, _ = check(counts, rec, whole)             # exactly what ONE tile needs: "<=" holds
    assert cuts == [B] and not full
    if B > 64:
        kept, full, cuts, _ = check(counts, rec, whole - 1)     # one byte less: two tiles
        assert len(cuts) == 2 and not full
    one = 64 * c * rec
    kept, full, cuts, _ = check(counts, rec, one)               # exactly one group: a tile per group, nobody taken out
    assert len(cuts) == (B + 63) // 64 and not full
    kept, full, cuts, _ = check(counts, rec, one - 1)           # one byte less: nobody fits
    assert full == list(range(B)) and not kept.any()


@pytest.mark.parametrize("B", [128, 129, 200, 1000])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_long_group(B, where):
    """A group of long trajectories beside short ones: the greedy cuts isolate it; the equal-sized alternative would
    put short groups beside it at its row count and must be refused when that exceeds the budget."""
    rec = 160
    G = (B + 63) // 64
    g = {"first": 0, "middle": G // 2, "last": G - 1}[where]
    counts = np.full(B, 100, np.int32)
    counts[64 * g + 3:64 * g + 9] = 1000
    for budget in (64 * 1000 * rec, 64 * 1000 * rec + 64 * 100 * rec, 128 * 1000 * rec - 1, 128 * 1000 * rec,
                   64 * 999 * rec, 64 * 100 * rec):
        kept, full, cuts, balanced = check(counts, rec, budget)
        if budget < 64 * 1000 * rec:                    # below one group of the longest instances: they are taken out
            assert full == list(range(64 * g + 3, min(64 * g + 9, B)))
    if B == 200 and where == "first":
        # 64 * 1000 records: the long group alone, then the rest -- two tiles; two equal tiles of 128 do not fit
        kept, full, cuts, balanced = check(counts, rec, 64 * 1000 * rec)
        assert cuts == [64, 200] and not balanced


@pytest.mark.parametrize("B", SIZES)
def test_counts_of_at_most_two(B):
    """Failed and trivial instances (0, 1, 2 points): every tile still has the two rows of a store-mode launch."""
    rng = np.random.default_rng(B)
    counts = rng.integers(0, 3, B).astype(np.int32)
    for groups in (1, 2, 3, 100):
        kept, full, cuts, _ = check(counts, 24, 2 * 64 * 24 * groups)
        assert not full and len(cuts) == -(-((B + 63) // 64) // groups)


def test_balanced_alternative_is_taken_when_it_fits():
    rec = 24
    counts = np.full(200, 50, np.int32)                 # 4 groups; 3 groups per tile fit: greedy [192, 200]
    kept, full, cuts, balanced = check(counts, rec, 192 * 50 * rec)
    assert balanced and cuts == [128, 200]
    counts = np.full(1000, 50, np.int32)                # 16 groups, 5 per tile: greedy 320/320/320/40 -> 4 x 256 (last 232)
    kept, full, cuts, balanced = check(counts, rec, 320 * 50 * rec)
    assert balanced and cuts == [256, 512, 768, 1000]


def test_every_small_case_exhaustively():
    """Three groups, every combination of four row counts per group, budgets around every tile's need."""
    rec = 8
    levels = (2, 5, 9, 30)
    for B in (129, 192):
        for combo in itertools.product(levels, repeat=3):
            counts = np.repeat(np.array(combo, np.int32), 64)[:B]
            needs = {_round64(n) * r * rec for n in (64, 128, 192) for r in levels}
            for budget in sorted({b + d for b in needs for d in (-1, 0, 1)}):
                if budget >= 2 * 64 * rec:
                    check(counts, rec, budget)


def test_argument_checks():
    from sunode_amd import _native
    L = _native.load_library()
    a = np.zeros(4, np.int32)
    n = ctypes.c_int32()
    assert L.sa_plan_tiles(4, a.ctypes.data, 0, 100, a.ctypes.data, a.ctypes.data, ctypes.byref(n), a.ctypes.data,
                           ctypes.byref(n), None) != 0
    assert L.sa_plan_tiles(4, None, 8, 100, a.ctypes.data, a.ctypes.data, ctypes.byref(n), a.ctypes.data,
                           ctypes.byref(n), None) != 0
