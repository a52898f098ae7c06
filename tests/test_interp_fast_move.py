"""The one-index move of the backward interpolation as straight-line code (csrc/bdf_kernels.hip interp_y,
SA_INTERP_FAST_MOVE).

`CVAfindIndex` walks from the last bracketing index one stored point at a time.  Nearly every move of the one-lane
adjoint kernel is ONE index to the left, and for that move everything the walk looks at is in registers: t[ilast-1]
(tlo) and t[ilast-2] (tlo2).  The device classifies a call as such a move when

    (t - tlo) < 0   and   ilast >= 2   and   not (t - tlo2) <= 0

and then sets indx = ilast - 1, ilast = indx, thi = tlo, tlo = tlo2, newpoint = 1 with selects; every other call runs
the walk.  Checked here on a host transcription of BOTH forms of the index part of interp_y (no GPU; the device code is
compared with the oracle's plain walk and with the -DSA_INTERP_FAST=0 build by tests/test_gpu_interp_fast.py): the
stored times increase strictly, the walk's first comparison is the classification's first, its second look is the
classification's third, so after every call of every query sequence indx, ilast, tlo / thi / tlo2, newpoint and the
return code agree, and the walk text is entered only where the classification does not hold."""
import numpy as np

UROUND = 2.220446049250313e-16
FUZZ_FACTOR_ADJ = 1000000.0
CV_SUCCESS, CV_GETY_BADT = 0, -107


class State:
    """The fields of Cv<BWD> the index part of interp_y reads and writes."""

    def __init__(self, T):
        self.T = T
        self.np = len(T)
        self.tfinal = T[-1]
        self.ilast, self.newdata, self.have_last, self.last_t = 0, 1, 0, 0.0
        self.tlo = self.thi = self.tlo2 = 0.0
        self.cur_idx = 0
        self.n_interp = self.n_rebuild = 0
        self.walks = 0                  # calls that ran the walk text
        self.moves1 = 0                 # calls the straight-line form served as a one-index move

    def fields(self):
        return (self.ilast, self.newdata, self.have_last, self.last_t, self.tlo, self.thi, self.tlo2, self.cur_idx,
                self.n_interp, self.n_rebuild)


def record_t2(T, indx):
    """T[2] of the table record of index indx: t[indx-2]; the forward kernel's point history starts at zero"""
    return T[indx - 2] if indx >= 2 else 0.0


def walk_text(m, t, newpoint):
    """interp_y from `if (m.newdata)` to the end of the move to the right: returns (code or None, indx, newpoint)"""
    T = m.T
    m.walks += 1
    if m.newdata:
        m.ilast = m.np - 1; newpoint = 1; m.newdata = 0
        m.tlo = T[m.ilast - 1]; m.thi = T[m.ilast]
        m.tlo2 = T[m.ilast - 2] if m.ilast >= 2 else m.tlo
    ilast = m.ilast
    to_left = (t - m.tlo) < 0.0
    to_right = (t - m.thi) > 0.0
    indx = ilast
    if to_left:
        newpoint = 1
        tprev, tcur = m.tlo, m.thi
        while True:
            if indx == 0:
                break
            if (t - tprev) <= 0.0:
                indx -= 1
                tcur = tprev
                if indx > 0:
                    tprev = m.tlo2 if indx == ilast - 1 else T[indx - 1]
            else:
                break
        m.ilast = 1 if indx == 0 else indx
        if indx == 0:
            m.tlo = tcur; m.thi = T[1]
            if abs(t - m.tlo) > FUZZ_FACTOR_ADJ * UROUND:
                return CV_GETY_BADT, indx, newpoint
        else:
            m.tlo = tprev; m.thi = tcur
    elif to_right:
        newpoint = 1
        tcur, tprev = m.thi, m.tlo
        while True:
            if indx >= m.np - 1:
                break
            if (t - tcur) > 0.0:
                indx += 1
                tprev = tcur
                tcur = T[indx]
            else:
                break
        m.ilast = indx
        m.tlo = tprev; m.thi = tcur
        if (t - m.thi) > FUZZ_FACTOR_ADJ * UROUND * (abs(m.tfinal) + 1.0):
            return CV_GETY_BADT, indx, newpoint
    return None, indx, newpoint


def interp_index(m, t, fast):
    """The index part of interp_y up to the evaluation: (return code, indx, newpoint); indx / newpoint are None where
    the function returns before it has them."""
    if m.have_last and t == m.last_t:
        return CV_SUCCESS, None, None
    m.n_interp += 1
    newpoint = 0
    if fast:
        move1 = (not m.newdata) and (t - m.tlo) < 0.0 and m.ilast >= 2 and not ((t - m.tlo2) <= 0.0)
        walk = bool(m.newdata) or (not move1 and ((t - m.tlo) < 0.0 or (t - m.thi) > 0.0))
        assert not (move1 and walk)
        m.moves1 += 1 if move1 else 0
        tlo_old = m.tlo
        indx = m.ilast - (1 if move1 else 0)
        m.ilast = indx
        m.thi = tlo_old if move1 else m.thi
        m.tlo = m.tlo2 if move1 else tlo_old
        newpoint = 1 if move1 else 0
        if walk:
            code, indx, newpoint = walk_text(m, t, newpoint)
            if code is not None:
                return code, indx, newpoint
    else:
        code, indx, newpoint = walk_text(m, t, newpoint)
        if code is not None:
            return code, indx, newpoint
    m.have_last = 1
    m.last_t = t
    if indx == 0:
        return CV_SUCCESS, indx, newpoint
    if newpoint:
        m.n_rebuild += 1
        m.cur_idx = indx
        if indx == m.ilast:
            m.tlo2 = record_t2(m.T, indx)
    return CV_SUCCESS, indx, newpoint


def run_both(T, queries):
    """Every query through both forms, each on its own state; returns the calls the fast form served without the walk"""
    a, b = State(T), State(T)
    for k, t in enumerate(queries):
        ra = interp_index(a, t, fast=False)
        rb = interp_index(b, t, fast=True)
        assert ra == rb, (k, t, ra, rb)
        assert a.fields() == b.fields(), (k, t, a.fields(), b.fields())
    return len(queries) - b.walks, b


def grids():
    rng = np.random.default_rng(20261018)
    for n in (2, 3, 4, 7, 64, 300):
        for kind in ("uniform", "geometric", "random"):
            if kind == "uniform":
                T = np.linspace(0.0, 10.0, n)
            elif kind == "geometric":
                T = np.r_[0.0, np.cumsum(1e-6 * 1.07 ** np.arange(n - 1))]
            else:
                T = np.r_[0.25, 0.25 + np.cumsum(rng.uniform(1e-9, 1.0, n - 1))]
            assert (np.diff(T) > 0).all()
            yield T, rng


def near(T, k, rng):
    """a stored time, its two neighbours in the floating-point numbers, or a point inside the interval to its left"""
    lo = T[k - 1] if k > 0 else T[0] - 1.0
    return [T[k], np.nextafter(T[k], -np.inf), np.nextafter(T[k], np.inf), rng.uniform(lo, T[k])][int(rng.integers(0, 4))]


def test_backward_sweeps_agree_and_take_the_straight_line_path():
    """What the adjoint kernel asks for: t decreasing in steps short against the stored intervals (moves by 0 and 1),
    a rejected attempt stepping back to the right now and then."""
    for T, rng in grids():
        t, qs = T[-1], []
        while t > T[0]:
            qs.append(t)
            if rng.uniform() < 0.1 and len(qs) > 2:
                qs.append(qs[-2])                     # the retry of a rejected attempt: back to the right
            k = max(int(np.searchsorted(T, t)), 1)    # a thirteenth of the stored interval around t, more or less
            t -= (T[k] - T[k - 1]) / 13.0 * rng.uniform(0.2, 2.0)
        qs.append(T[0])
        served, m = run_both(T, qs)
        if len(T) >= 64:
            # nearly every move is one index to the left, served without the walk
            assert m.n_rebuild > len(T) // 2 and served > 0.9 * len(qs)


def test_moves_by_zero_one_two_and_many_in_both_directions():
    for T, rng in grids():
        n = len(T)
        for _ in range(60):
            qs = [near(T, int(rng.integers(0, n)), rng)]
            k = int(rng.integers(0, n))
            for _ in range(40):
                d = [0, 0, 1, -1, 2, -2, int(rng.integers(-n, n + 1))][int(rng.integers(0, 7))]
                k = min(max(k + d, 0), n - 1)
                qs.append(near(T, k, rng))
                if rng.uniform() < 0.2:
                    qs.append(qs[-1])                 # the same t again: evaluated once
            run_both(T, qs)


def test_stored_times_themselves():
    """t equal to a stored time, walked down and up: the <= of the walk's comparison decides the index"""
    for T, _ in grids():
        down = list(T[::-1])
        run_both(T, down + list(T) + down[::2] + list(T[::3]))


def test_arrival_at_index_zero_and_both_ends():
    for T, rng in grids():
        n = len(T)
        fuzz_l = FUZZ_FACTOR_ADJ * UROUND
        fuzz_r = FUZZ_FACTOR_ADJ * UROUND * (abs(T[-1]) + 1.0)
        ends = [T[0], T[0] - 0.5 * fuzz_l, T[0] - 2.0 * fuzz_l, T[0] - 1.0,          # left end: inside / outside the fuzz
                T[-1], T[-1] + 0.5 * fuzz_r, T[-1] + 2.0 * fuzz_r, T[-1] + 1.0]     # right end
        for e in ends:
            for start in (n - 1, n // 2, 1, 0):
                # from fresh data, from a bracket in the middle, from the first intervals; then on after the call
                qs = [near(T, start, rng), e, near(T, min(1, n - 1), rng), e, near(T, n - 1, rng), e, T[0], e]
                run_both(T, qs)
        # one index at a time down to index 0 (the last one-index move ends at index 1: ilast >= 2 no longer holds)
        mids = [0.5 * (T[k - 1] + T[k]) for k in range(n - 1, 0, -1)]
        served, m = run_both(T, mids + [T[0]])
        assert m.ilast == 1 and m.walks == 1 and served == n - 1      # (only the first call, on fresh data, walks)


def test_two_and_three_stored_points():
    """np = 2: ilast is always 1, every call runs the walk; np = 3: one possible one-index move"""
    rng = np.random.default_rng(7)
    for n in (2, 3):
        T = np.r_[0.0, np.cumsum(rng.uniform(0.1, 1.0, n - 1))]
        moves1 = 0
        for _ in range(200):
            qs = [rng.uniform(T[0] - 0.1, T[-1] + 0.1) if rng.uniform() < 0.7 else near(T, int(rng.integers(0, n)), rng)
                  for _ in range(12)]
            moves1 += run_both(T, qs)[1].moves1
        if n == 2:
            # ilast >= 2 never holds: no call is a one-index move (calls inside the bracket need no walk either)
            assert moves1 == 0
            m = State(T)
            assert interp_index(m, 0.5 * (T[0] + T[1]), fast=True)[2] == 1 and m.walks == 1
        else:
            # the one possible move, from the bracket [t1, t2] to [t0, t1], is taken by the straight-line form
            assert moves1 > 0
            served, m = run_both(T, [T[2], 0.5 * (T[0] + T[1])])
            assert m.walks == 1 and m.moves1 == 1 and served == 1 and (m.ilast, m.tlo, m.thi) == (1, T[0], T[1])
