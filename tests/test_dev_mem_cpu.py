"""The owners of the library's device and pinned memory (csrc/dev_mem.h) on the CPU: tests/dev_mem_host_main.cpp defines the
HIP allocation calls over malloc and a table of live pointers, runs the pool and the grow-only buffer through scope ends,
releases, failing allocations, zero-fills, growth (free before allocate) and moves, and exits non-zero at the first check
that fails.  Built for the host with ROCm's clang++, without the HIP runtime."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_and_grow_only_buffer_own_what_they_allocate():
    exe = os.path.join(tempfile.mkdtemp(), 'dev_mem_host')
    subprocess.run(['/opt/rocm/llvm/bin/clang++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-D__HIP_PLATFORM_AMD__',
                    '-I/opt/rocm/include', os.path.join(ROOT, 'tests', 'dev_mem_host_main.cpp'), '-o', exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', (r.returncode, r.stdout, r.stderr)
