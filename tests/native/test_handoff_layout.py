"""Host check of the blocked hand-off layout's index math (native/kernels/handoff_layout.h).

The header's constexpr functions are compiled with a host compiler into a stand-alone program
(tests/native/handoff_layout_check.cpp) that, for the LeNet shapes, checks that the weight-gradient
tile receives every (feature, sample) in exactly the lane and element of the plain ``[F][M]``
addressing (LDS-DMA path at M = 1024, global-load path at M = 8 / 40 / 520 / 1024), that the DMA
image and the fragment reads are inverse maps, that no pad feature is read as live and no source
chunk leaves its tensor, and that a model of the LDS lane groups (``ds_read_b64`` and the merged
``ds_read2_b64`` form the compiler emits for most of the reads) shows the conflict degree the header
states.

The compiler is g++ or clang++ from PATH, else the ROCm toolchain's clang++ the project is built
with; the test does not skip."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = os.path.join(os.path.dirname(os.path.dirname(HERE)), "rocket_amd", "native", "kernels")


def _host_cxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (shutil.which("g++"), shutil.which("clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"),
              os.path.join(rocm, "llvm", "bin", "clang++")):
        if c and os.path.exists(c):
            return c
    raise AssertionError("no host C++ compiler (g++, clang++ or the ROCm toolchain's clang++)")


def test_handoff_layout_index_math(tmp_path):
    exe = str(tmp_path / "handoff_layout_check")
    cmd = [_host_cxx(), "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{KERNELS}",
           os.path.join(HERE, "handoff_layout_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "handoff layout: ok" in run.stdout, run.stdout
    assert "ds_read_b64 conflict degree: 1 (stated: 1)" in run.stdout, run.stdout
    assert "ds_read2_b64 conflict degree: 1 (stated: 1)" in run.stdout, run.stdout
