"""The device-buffer owner and the lazy-set helper (surfh_amd/csrc/dev_buf.h) on the host: tests/native/dev_buf_test.cpp is a
stand-alone program with its own allocator (malloc, a live count, a refusal at the k-th call); it is compiled here with the
address and undefined-behaviour sanitizers and run.  No GPU, no HIP header: dev_buf.h includes none."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "dev_buf_test.cpp")


def _compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    pytest.fail("no host C++ compiler found (c++, g++, clang++)")


def test_dev_buf_program(tmp_path):
    exe = str(tmp_path / "dev_buf_test")
    base = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", SRC, "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:
        # no sanitizer runtimes on this machine: the program's own checks still run, and the output says which build ran
        print("sanitizer build failed, building without:\n" + san.stderr[-2000:])
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout and "none live" in run.stdout
