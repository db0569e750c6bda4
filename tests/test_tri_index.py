"""CPU: the address recurrences of the no-wrap form of the compact direction's triangular products
(csrc/lbfgs_device.h: lb_cmp_tri_nowrap) restated in plain Python and checked against lb_tri.

While the live window does not wrap round the ring (head + n <= 100) the no-wrap form replaces the general form's
per-column ring arithmetic by running registers: a packed index that advances by a constant (backward product) or by a
running second difference (forward product), and vector elements at a base plus constant offsets.  It must visit exactly
what the general form visits: lane q of row a takes the live columns b = q (mod 4) in ascending order, the packed entry
{slot(a), slot(b)} and the vector element slot(b) - for every head and window length, with and without a freshly
inserted pair (which the forward product leaves out: it is the newest column).  And every address it forms, the masked
columns of a lane's last batch and the aliased dead rows included, must lie inside the arrays."""
import functools

import pytest

LB_HIST = 100
LB_RPACK = (LB_HIST * (LB_HIST + 1) // 2 + 3) // 4 * 4
LB_TRI_B = 8                       # columns per lane and batch (4 in a short last batch)
WORK = 128                         # elements of the work vectors (LbWork::bvec, gnew, zv)


def lb_tri(r, c):
    hi, lo = max(r, c), min(r, c)
    return hi * (hi + 1) // 2 + lo


def wave_trips(n, nE, a, fwd):
    """Column steps of the longest lane of row a's wave (16 rows, first row a0): uniform, it picks the batch sizes."""
    a0 = a & ~15
    return (nE - a0 + 3) >> 2 if fwd else (min(a0 + 15, n - 1) + 4) >> 2


def lane_columns(head, n, nE, a, q, fwd):
    """The column loop of one lane as the kernel runs it.  Returns (executed, loaded): the (packed index, vector index) of
    the columns whose product enters the sum, in order, and of every column whose operands are loaded."""
    # (what the loop does depends on n through the aliased row and the wave's trip count alone, the backward product not on nE)
    return _lane_columns(head, min(a, n - 1), nE if fwd else 0, q, fwd, wave_trips(n, nE, a, fwd))


@functools.lru_cache(maxsize=None)
def _lane_columns(head, ar, nE, q, fwd, trips):
    if fwd:
        b0 = ar + ((q - ar) & 3)
        cnt = (nE - b0 + 3) >> 2
        S = head + b0
        R = ((S * (S + 1)) >> 1) + head + ar
    else:
        b0 = q
        cnt = (ar - q + 4) >> 2
        S = head + b0
        R = lb_tri(head + ar, head + q)
    assert cnt <= trips
    xp = head + b0
    S4 = 4 * S
    executed, loaded = [], []
    k0 = 0
    while k0 < trips:
        rem = cnt - k0
        B = LB_TRI_B if trips - k0 > 4 else 4    # the last batch is a short one where four columns cover the wave's rest
        if rem > 0:                              # (a lane that has run out of columns sits the batch out)
            A = R
            for j in range(B):
                cj = 8 * j * j + 2 * j if fwd else 4 * j
                at = (min(A, LB_RPACK - 1 - cj) + cj, xp + 4 * j)
                loaded.append(at)
                if j < rem:
                    executed.append(at)
                if fwd:
                    A += S4
            xp += 4 * B
            if fwd:
                R += B * S4 + (4 * B) * (4 * B + 1) // 2
                S4 += 16 * B
            else:
                R += 4 * B
        k0 += B
    return executed, loaded


@functools.lru_cache(maxsize=None)
def check_lane(head, ar, nE, q, fwd, live, trips):
    """One lane of row ar (a live row, or the alias a dead row runs as): addresses in bounds; for a live row, the columns
    that enter the sum are the live ones with b = q (mod 4), ascending, at the entries lb_tri names."""
    executed, loaded = _lane_columns(head, ar, nE, q, fwd, trips)
    for idx, xi in loaded:
        assert 0 <= idx < LB_RPACK and 0 <= xi < WORK, (head, ar, nE, q, fwd, idx, xi)
    if live:
        cols = [b for b in (range(ar, nE) if fwd else range(0, ar + 1)) if b % 4 == q]
        assert executed == [(lb_tri(head + ar, head + b), head + b) for b in cols], (head, ar, nE, q, fwd)
    return len(executed)


def check_window(head, n, inserted, fwd):
    nE = n - 1 if (fwd and inserted) else n
    for a in range(LB_HIST):
        if (a & ~15) >= n:                       # the wave's first row is dead: the wave does not enter the column loop
            continue
        # (a dead row's sum is discarded: only its addresses matter)
        total = sum(check_lane(head, min(a, n - 1), nE if fwd else 0, q, fwd, a < n, wave_trips(n, nE, a, fwd)) for q in range(4))
        if a < n:                                # the four lanes' columns are disjoint (b mod 4): none is skipped
            assert total == (max(nE - a, 0) if fwd else a + 1), (head, n, inserted, fwd, a)


@pytest.mark.parametrize('heads', [range(0, 8), range(8, 20), range(20, 36), range(36, 100)])
@pytest.mark.parametrize('product', ['forward', 'forward_inserted', 'backward'])
def test_nowrap_recurrences_visit_what_lb_tri_says(product, heads):
    for head in heads:
        for n in range(1, LB_HIST - head + 1):
            check_window(head, n, product == 'forward_inserted', product != 'backward')


def test_batches_of_the_longest_row():
    """A 64-pair window takes two batches (the general form takes three batches of 4 columns per lane at 48 pairs), the
    typical 42-pair window 8 + 4 column steps for its 11 columns per lane."""
    for n, steps in ((64, [8, 8]), (42, [8, 4]), (16, [4]), (17, [8])):
        for fwd, a in ((True, 0), (False, n - 1)):
            loaded = max(len(lane_columns(0, n, n, a, q, fwd)[1]) for q in range(4))
            assert loaded == sum(steps), (n, fwd, loaded)
