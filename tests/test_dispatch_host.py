"""csrc/dispatch.h on its own: the value lists and the variadic dispatcher every kernel launch site
picks its instantiation with.  Host C++17 only, so it builds with any compiler and needs no GPU:
tests/dispatch_host.cpp walks a three-selector dispatch (a lane list, a flag, a list without a
fallback) and checks the constants delivered, the fallback to the last entry, the unmatched case
(no call, false) and has()."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = cxx and shutil.which(cxx)
        if path:
            return path
    return None


def test_dispatch_header_standalone(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path / "dispatch_host")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "hybrid-gmres_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dispatch_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("dispatch ok"), run.stdout
