"""CPU: who owns which item of the forward basis stream, and which thread writes which word in E1 (csrc/model_layout.h:
fwd_item_owner and the E1_* constants; csrc/closure_device.h: pose_prep_elems, sparse_forward), restated in plain Python.

E2 streams pd_sub as 8 k-slices x nc_pad / 4 float4 column groups = items.  Stream thread t (thread 64 + t, waves 1-7) owns the
items t and t + 448 that exist; the threads of waves 5-7 (t >= 256), which have no work in E1, load their item there, one
barrier early.  Checked for the three model sizes (a skeleton model, the LSP regressor, top4): every item has exactly one
owner, the early items are exactly those of 256 <= t < 448 that exist, the counts the design quotes.  E1: 305 workers on the
threads below 320, every word of coef, R, Mj and J written exactly once.  The constants of the mirror are read back from the
header, and the header's function is compared as text, so that an edit there fails here."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mvsmplfitting_amd', 'csrc')
NT, NJ, KROWS = 512, 24, 224
FWD_SLICES, FWD_THREADS, FWD_EARLY_T0 = 8, 448, 256
E1_POSE_T, E1_NPOSE, E1_WORKERS, E1_IDLE_T0 = 288, 207, 305, 320


def fwd_item_owner(nc_pad, t):
    """(first item, number of items, first one loaded early) of stream thread t: model_layout.h"""
    nitems = (nc_pad >> 2) * FWD_SLICES
    n = 0 if t >= nitems else (2 if t + FWD_THREADS < nitems else 1)
    return t, n, n > 0 and t >= FWD_EARLY_T0


def owners(nc_pad):
    """item -> [(t, early)] over the stream threads"""
    out = {}
    for t in range(FWD_THREADS):
        first, n, early = fwd_item_owner(nc_pad, t)
        for k in range(n):
            out.setdefault(first + k * FWD_THREADS, []).append((t, early and k == 0))
    return out


def test_the_mirror_has_the_headers_constants_and_function():
    txt = open(os.path.join(CSRC, 'model_layout.h')).read()
    const = lambda name: re.search(r'\b%s = ([^;,]+)[;,]' % name, txt).group(1).strip()
    assert const('NJ') == '24' and const('KROWS') == '224' and const('FWD_SLICES') == '8'
    assert const('E1_POSE_T') == 'NJ * 12' and const('E1_NPOSE') == '(NJ - 1) * 9'
    assert const('E1_WORKERS') == 'E1_POSE_T + (KROWS - E1_NPOSE)' and const('E1_IDLE_T0') == '320'
    assert const('FWD_THREADS') == '512 - 64' and const('FWD_EARLY_T0') == 'E1_IDLE_T0 - 64'
    body = re.search(r'constexpr FwdOwner fwd_item_owner\(int nc_pad, int t\) \{(.*?)\n\}', txt, re.S).group(1)
    assert [l.strip() for l in body.strip().split('\n')] == [
        'const int nitems = (nc_pad >> 2) * FWD_SLICES;',
        'const int n = t >= nitems ? 0 : (t + FWD_THREADS < nitems ? 2 : 1);',
        'return FwdOwner{t, n, n > 0 && t >= FWD_EARLY_T0};']
    assert (E1_POSE_T, E1_NPOSE, E1_WORKERS) == (NJ * 12, (NJ - 1) * 9, NJ * 12 + KROWS - (NJ - 1) * 9)
    assert FWD_THREADS == NT - 64 and FWD_EARLY_T0 == E1_IDLE_T0 - 64


@pytest.mark.parametrize('nc_pad', [16, 208, 264])
def test_every_item_has_one_owner_and_the_early_ones_are_waves_5_to_7(nc_pad):
    nitems = (nc_pad >> 2) * FWD_SLICES
    own = owners(nc_pad)
    assert sorted(own) == list(range(nitems))
    assert all(len(v) == 1 for v in own.values())
    early = sorted(item for item, v in own.items() if v[0][1])
    assert early == [t for t in range(FWD_EARLY_T0, FWD_THREADS) if t < nitems]
    for item, ((t, e),) in own.items():
        assert item in (t, t + FWD_THREADS)
        assert e == (item == t and 64 + t >= E1_IDLE_T0)                  # early <=> first item of a thread of waves 5-7
    # the in-slot waves of the shipped form (threads 64..319) own exactly the rest
    rest = sorted(item for item, v in own.items() if not v[0][1])
    assert rest == sorted(t + k * FWD_THREADS for t in range(FWD_EARLY_T0) for k in range(fwd_item_owner(nc_pad, t)[1]))


def test_the_counts_of_the_three_models():
    count = lambda nc_pad: (len(owners(nc_pad)), sum(v[0][1] for v in owners(nc_pad).values()))
    assert count(16) == (32, 0)                                           # a skeleton model: no early item
    assert count(208) == (416, 160)                                       # the LSP regressor
    assert all(fwd_item_owner(208, t)[1] == 0 for t in range(416, 448))   # threads 416..447 own nothing
    assert all(fwd_item_owner(208, t)[1] == 1 for t in range(416))
    assert count(264) == (528, 192)                                       # top4
    assert [t for t in range(FWD_THREADS) if fwd_item_owner(264, t)[1] == 2] == list(range(80))
    assert not any(fwd_item_owner(264, t)[2] for t in range(80))          # both items of such a thread are in-slot
    # an early thread never owns a second item, whatever the model (NC_MAX = 288 columns)
    assert all(fwd_item_owner(nc_pad, t)[1] <= 1 for nc_pad in range(4, 292, 4) for t in range(FWD_EARLY_T0, FWD_THREADS))


def e1_writes(tid):
    """the words thread tid writes in E1: pose_prep_elems"""
    if tid >= E1_IDLE_T0:
        return []
    if tid >= E1_POSE_T:
        p = E1_NPOSE + tid - E1_POSE_T
        return [('coef', p)] if p < KROWS else []
    j, e = divmod(tid, 12)
    if e < 9:
        w = [('R', j, e), ('Mj', j, 4 * (e // 3) + e % 3)]
        if e < 3:
            w.append(('rod', j, e))
        if j >= 1:
            w.append(('coef', 9 * (j - 1) + e))
        return w
    return [('J', j, e - 9), ('Mj', j, 4 * (e - 9) + 3)]


def test_e1_has_305_workers_below_thread_320_and_writes_every_word_once():
    workers = [tid for tid in range(NT) if e1_writes(tid)]
    assert len(workers) == E1_WORKERS == 305 and max(workers) < E1_IDLE_T0 and workers == list(range(305))
    assert sum(1 for tid in workers if ('R', tid // 12, tid % 12) in e1_writes(tid)) == 216
    assert sum(1 for tid in workers if e1_writes(tid)[0][0] == 'J') == 72
    assert sum(1 for tid in workers if e1_writes(tid) == [('coef', E1_NPOSE + tid - E1_POSE_T)]) == 17
    written = [w for tid in range(NT) for w in e1_writes(tid)]
    assert len(written) == len(set(written))
    want = {('coef', p) for p in range(KROWS)} | {('R', j, e) for j in range(NJ) for e in range(9)}
    want |= {('Mj', j, e) for j in range(NJ) for e in range(12)} | {('J', j, a) for j in range(NJ) for a in range(3)}
    want |= {('rod', j, e) for j in range(NJ) for e in range(3)}
    assert set(written) == want
    # the pose feature's word p = 9 (j - 1) + e comes from the thread that owns R[j][e]
    for p in range(E1_NPOSE):
        j, e = 1 + p // 9, p % 9
        assert ('coef', p) in e1_writes(12 * j + e) and ('R', j, e) in e1_writes(12 * j + e)
