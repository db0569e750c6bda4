"""CPU: the lane map and the cross-lane sum of the compact direction's register-form mat-vec (csrc/lbfgs_device.h:
lb_mv_chunk, lb_cmp_matvec_row), restated in plain Python.

512 threads: lane & 15 is the row class c (history rows c, c + 16, ...), lb_mv_chunk(tid) the four-element chunk.  Checked:
the map is a bijection onto (chunk place, class) that covers every live chunk of ld = 88 and ld = 52 and every chunk that has to
be stored (up to LB_D / 4) with the sixteen classes of a chunk in one DPP row; the DPP sequence of the device code, run on
symbols, leaves ((((((P_0 + P_1) + P_2) + P_3) + P_4) + P_5) + P_6) + P_7 with P_w = A_2w + A_2w+1 of the row's own chunk in
the storing lane; the 16-byte loads of a history row chunk are free of LDS bank conflicts at ld = 88 and at most two-way at
ld = 52."""
import pytest

NT, LB_D, LB_HIST = 512, 96, 100
# lanes served together by one LDS cycle of a 16-byte read (64 banks of 4 bytes: sixteen 16-byte units)
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]


def mv_chunk(tid):
    return 2 * (tid >> 6) + ((tid >> 4) & 1) + 16 * ((tid >> 5) & 1)


def test_the_map_is_a_bijection_with_a_chunk_per_dpp_row():
    seen = {}
    for tid in range(NT):
        seen.setdefault((mv_chunk(tid), tid & 15), []).append(tid)
    assert len(seen) == NT and all(len(v) == 1 for v in seen.values())
    assert {cl for cl, _ in seen} == set(range(32))
    for cl in range(32):
        rows = {seen[(cl, c)][0] >> 4 for c in range(16)}
        assert len(rows) == 1, (cl, rows)                               # the sixteen classes of a chunk: one DPP row of one wave


@pytest.mark.parametrize('ld', [88, 52])
def test_every_live_element_and_every_stored_chunk_has_its_lanes(ld):
    live = {(mv_chunk(tid), (tid & 15) + 16 * i) for tid in range(NT) for i in range(7) if 4 * mv_chunk(tid) < ld and (tid & 15) + 16 * i < LB_HIST}
    assert live == {(cl, r) for cl in range(ld // 4) for r in range(LB_HIST)}
    stored = sorted(mv_chunk(tid) for tid in range(NT) if (tid & 15) == 0 and mv_chunk(tid) < LB_D // 4)
    assert stored == list(range(LB_D // 4))


def test_the_dpp_sequence_adds_the_eight_pair_sums_in_ascending_order():
    for wave in range(NT // 64):
        acc = [('A', mv_chunk(64 * wave + l), l & 15) for l in range(64)]
        xor1 = lambda v: [v[l ^ 1] for l in range(64)]                           # quad_perm [1,0,3,2]
        bcast = lambda v, n: [v[(l & ~15) + n] for l in range(64)]               # row_newbcast:n
        add = lambda a, b: [('+', x, y) for x, y in zip(a, b)]
        p = add(acc, xor1(acc))
        s = add(bcast(p, 0), bcast(p, 2))
        for n in (4, 6, 8, 10, 12, 14):
            s = add(s, bcast(p, n))
        for row in range(4):
            cl = mv_chunk(64 * wave + 16 * row)
            pw = [('+', ('A', cl, 2 * w), ('A', cl, 2 * w + 1)) for w in range(8)]
            want = ('+', pw[0], pw[1])
            for w in range(2, 8):
                want = ('+', want, pw[w])
            assert s[16 * row] == want, (wave, row)


@pytest.mark.parametrize('ld, worst', [(88, 1), (52, 2)])
def test_lds_banks_of_the_row_loads(ld, worst):
    nch = ld // 4
    most = 0
    for wave in range(NT // 64):
        for i in range(7):
            for grp in B128_GROUPS:
                units = {}
                for l in grp:
                    tid = 64 * wave + l
                    r = min((tid & 15) + 16 * i, LB_HIST - 1)
                    cl = mv_chunk(tid)
                    unit = r * nch + (cl if cl < nch else cl & 1)               # 16-byte units from the start of the rows (dead chunk: 0 / 1)
                    units.setdefault(unit % 16, set()).add(unit)                # (equal addresses broadcast)
                most = max(most, max(len(v) for v in units.values()))
    assert most <= worst, most
