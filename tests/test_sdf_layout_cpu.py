"""The byte layouts of the SDF term's two workspaces (csrc/sdf_layout.h) on the CPU, built for the host (tests/
sdf_layout_host_shim.cpp, ROCm's clang++): the regions are ordered, aligned, disjoint and inside the allocation, and a launch
that covers fewer problems than the buffers were allocated for - a non-final sub-batch of a service tail - addresses the first
slices of the ALLOCATION's regions, tickets and bin counters included: the words that were zeroed when the buffer was made.

The expected offsets are worked out here from the documented order of the regions (sdf_layout.h) and the record sizes, not
read back from the header.  A launcher that derives the layout from its grid (96 problems inside buffers for 165) puts the
tickets inside the entry lists of problems the allocation's layout gives to others: test_a_sub_batch_addresses_... fails on
that arithmetic."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS = [1, 37, 96, 165]
NVS = [6890, 431]                     # SMPL's (even) and an odd count
FS = [512, 13776]                     # the smallest face-list term and all of SMPL's faces
NS, NC, NBINS, OFFS_LD, CAP = 8, 16, 256 * 256 + 64 ** 3, 256 * 256 + 64 ** 3 + 4, 64
ENTRY, ADJ, CHUNK, TRI = 16, (4 + 24 * 12 + 224) * 4, 48, 128


def up(x):
    return (x + 255) // 256 * 256


@pytest.fixture(scope='module')
def shim():
    so = os.path.join(tempfile.mkdtemp(), 'libsdf_layout_host.so')
    subprocess.run(['/opt/rocm/llvm/bin/clang++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'sdf_layout_host_shim.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.sdf_layout_work.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.sdf_layout_cull.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.sdf_layout_launch_work.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.sdf_layout_launch_cull.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.sdf_layout_constants.argtypes = [C.c_void_p]
    for f in (lib.sdf_layout_work, lib.sdf_layout_cull, lib.sdf_layout_constants):
        f.restype = None
    return lib


def work(lib, B, nv, grid=None):
    """{'off': [entries, part, chunks, tickets], 'bytes', 'stride': [...]} of a work area for B problems (as a launch over
    `grid` problems addresses it)"""
    o = np.zeros(9, np.int64)
    if grid is None:
        lib.sdf_layout_work(B, nv, o.ctypes.data)
    else:
        assert lib.sdf_layout_launch_work(grid, B, nv, o.ctypes.data) == 1
    return dict(off=[int(x) for x in o[:4]], bytes=int(o[4]), stride=[int(x) for x in o[5:9]])


def cull(lib, B, F, grid=None):
    """{'off': [tri, offs, cnt, ent, flag], 'bytes', 'stride': [...], 'zeroed': bytes of the counters the allocation clears}"""
    o = np.zeros(12, np.int64)
    if grid is None:
        lib.sdf_layout_cull(B, F, o.ctypes.data)
    else:
        assert lib.sdf_layout_launch_cull(grid, B, F, o.ctypes.data) == 1
    return dict(off=[int(x) for x in o[:5]], bytes=int(o[5]), stride=[int(x) for x in o[6:11]], zeroed=int(o[11]))


def check_regions(L, B, aligns):
    """ordered, aligned, disjoint, inside the allocation: region i holds B slices of stride[i] bytes"""
    ends = [o + B * s for o, s in zip(L['off'], L['stride'])]
    assert L['off'][0] == 0
    for i, (o, a) in enumerate(zip(L['off'], aligns)):
        assert o % a == 0, (i, o, a)
        if i:
            assert o >= ends[i - 1], (i, o, ends[i - 1])
    assert ends[-1] <= L['bytes']


def test_constants(shim):
    out = np.zeros(9, np.int64)
    shim.sdf_layout_constants(out.ctypes.data)
    assert [int(x) for x in out] == [NS, NC, NBINS, OFFS_LD, CAP, ENTRY, ADJ, CHUNK, TRI]


@pytest.mark.parametrize('nv', NVS)
@pytest.mark.parametrize('B', BS)
def test_work_area(shim, B, nv):
    L = work(shim, B, nv)
    assert L['stride'] == [nv * ENTRY, NS * ADJ, NC * CHUNK, 4]
    part = up(B * nv * ENTRY)
    chunks = part + B * NS * ADJ
    tickets = up(chunks + B * NC * CHUNK)
    assert L['off'] == [0, part, chunks, tickets] and L['bytes'] == tickets + 4 * B
    # float4 entries, 16-byte blocks of the adjoint records, doubles in the chunk records, ticket words
    check_regions(L, B, [16, 16, 8, 4])


@pytest.mark.parametrize('F', FS)
@pytest.mark.parametrize('B', BS)
def test_face_list_workspace(shim, B, F):
    L = cull(shim, B, F)
    assert L['stride'] == [F * TRI, OFFS_LD * 4, NBINS * 4, CAP * F * 8, 4]
    offs = up(B * F * TRI)
    cnt = offs + up(B * OFFS_LD * 4)
    ent = cnt + up(B * NBINS * 4)
    flag = ent + up(B * CAP * F * 8)
    assert L['off'] == [0, offs, cnt, ent, flag] and L['bytes'] == flag + up(4 * B)
    # the scan kernel reads counters and writes offsets as int4; list entries are int2
    check_regions(L, B, [16, 16, 16, 8, 4])
    # what the allocation clears covers every problem's counters and nothing of the lists behind them
    assert B * NBINS * 4 <= L['zeroed'] and L['off'][2] + L['zeroed'] <= L['off'][3]


@pytest.mark.parametrize('nv', NVS)
def test_a_sub_batch_addresses_the_first_slices_of_the_allocations_regions(shim, nv):
    """a grid of 96 problems inside buffers allocated for 165: problem b < 96 has, in every region, the bytes problem b has in the
    layout of 165 - tickets and bin counters among them, so the words the allocation zeroed are the ones the launch uses"""
    full, sub = work(shim, 165, nv), work(shim, 165, nv, grid=96)
    assert sub == full
    for i, (o, s) in enumerate(zip(sub['off'], sub['stride'])):
        for b in (0, 95):
            assert (o + b * s, o + (b + 1) * s) == (full['off'][i] + b * full['stride'][i], full['off'][i] + (b + 1) * full['stride'][i])
        nxt = full['off'][i + 1] if i + 1 < len(full['off']) else full['bytes']
        assert o + 96 * s <= nxt
    # the tickets the launch takes are the first 96 of the 165 words cleared at sdf_ticket_offset(165, nv)
    assert sub['off'][3] == up(up(165 * nv * ENTRY) + 165 * NS * ADJ + 165 * NC * CHUNK)
    # ... and not where a layout of 96 problems has them: inside the 165 layout's entry lists (for SMPL's nv), which a round overwrites
    own = work(shim, 96, nv)
    assert own['off'][3] != full['off'][3] and own['off'][1] != full['off'][1] and own['off'][2] != full['off'][2]
    if nv == 6890:
        assert own['off'][3] + 96 * 4 <= full['off'][1]
    for F in FS:
        cfull, csub = cull(shim, 165, F), cull(shim, 165, F, grid=96)
        assert csub == cfull
        cown = cull(shim, 96, F)
        assert all(cown['off'][i] != cfull['off'][i] for i in range(1, 5))
        # the 96 problems' counters lie inside what the allocation cleared; a layout of 96 has some of them in front of it
        lo, hi = cfull['off'][2], cfull['off'][2] + cfull['zeroed']
        assert lo <= csub['off'][2] and csub['off'][2] + 96 * csub['stride'][2] <= hi
        assert cown['off'][2] < lo


def test_a_grid_larger_than_the_allocation_is_refused(shim):
    o = np.zeros(12, np.int64)
    assert shim.sdf_layout_launch_work(166, 165, 6890, o.ctypes.data) == 0
    assert shim.sdf_layout_launch_cull(166, 165, 512, o.ctypes.data) == 0
    assert shim.sdf_layout_launch_work(165, 165, 6890, o.ctypes.data) == 1
    assert shim.sdf_layout_launch_work(-1, 165, 6890, o.ctypes.data) == 0
