"""Which kernel a per-round vertex pass runs, asked of csrc/fit_plan.cpp:plan_pass_launch itself: the host build of the plan
(tests/fit_plan_host_shim.cpp, ROCm's clang++, no HIP) is compiled once per process and queried, so the table pinned in
tests/test_fit_plan_cpu.py and the names in the ids of tests/test_gpu_vertex_pass_matrix.py come from the code the launcher
switches on."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT, SPLIT, SPLIT_LOOP, PIPE = range(4)                # fit_plan.h: PassKernel
KERNELS = ('lbs_vertex_pass_kernel', 'lbs_vertex_pass_split_kernel', 'lbs_vertex_pass_split_loop_kernel',
           'lbs_vertex_pass_pipe_kernel')
SHORT = ('exact', 'split', 'loop', 'pipe')


def build_shim():
    so = os.path.join(tempfile.mkdtemp(), 'libfit_plan_host.so')
    subprocess.run(['/opt/rocm/llvm/bin/clang++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'fit_plan_host_shim.cpp'),
                    os.path.join(ROOT, 'mvsmplfitting_amd', 'csrc', 'fit_plan.cpp'), '-o', so], check=True)
    lib = C.CDLL(so)
    lib.fit_plan_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    lib.fit_plan_nsets.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.fit_plan_constants.argtypes = [C.c_void_p]
    lib.fit_plan_pass_launch.argtypes = [C.c_int] * 5 + [C.c_void_p]
    lib.fit_plan_pass_launch.restype = None
    return lib


@functools.lru_cache(maxsize=None)
def shim():
    return build_shim()


def pass_launch(split_basis, sparse_skinning, nv_even, chunks, pass_kernel, lib=None):
    """(kernel, sparse, grid_y) of a launch over `chunks` 32-problem chunks"""
    out = np.zeros(3, np.int32)
    (lib or shim()).fit_plan_pass_launch(int(split_basis), int(sparse_skinning), int(nv_even), int(chunks), int(pass_kernel),
                                         out.ctypes.data)
    return int(out[0]), int(out[1]), int(out[2])


def kernel_name(kernel, sparse):
    """the instantiation as the source names it"""
    if kernel == PIPE:
        return KERNELS[kernel]
    return '%s<%s>' % (KERNELS[kernel], 'true' if sparse else 'false')


def short_name(split_basis, sparse_skinning, nv_even, B, pass_kernel):
    """for test ids: the kernel of a launch over all of B problems, e.g. 'pipe', 'split_sparse', 'loop_dense'"""
    k, sp, _ = pass_launch(split_basis, sparse_skinning, nv_even, (B + 31) // 32, pass_kernel)
    return SHORT[k] if k == PIPE else '%s_%s' % (SHORT[k], 'sparse' if sp else 'dense')
