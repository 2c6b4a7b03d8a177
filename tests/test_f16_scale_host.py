"""The fp16 operand scale (surfh_amd/csrc/f16_split.h: f16x2_scale, the one definition the gather, the ymat16 kernels and the GEMM
share) on the host: tests/native/f16_scale_test.cpp is a stand-alone program that compares it with the frexp / ldexp formula of
gemm_f16x2_scale on every fp32 exponent, and checks the zero / negative / NaN inputs and the values that need no reference.  It is
compiled here with a plain host compiler and run.  No GPU, no HIP header: f16_split.h includes none under such a compiler."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "f16_scale_test.cpp")


def _compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    pytest.fail("no host C++ compiler found (c++, g++, clang++)")


def test_f16_scale_program(tmp_path):
    exe = str(tmp_path / "f16_scale_test")
    build = subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout
