"""The per-stream registry of the library's host-side queues (ig-gcn_amd/csrc/pending.h) under sanitizers, on the CPU.

tests/host/pending_check.cpp is a stand-alone program: it includes pending.h and nothing of HIP, checks the queue contract
on fabricated stream handles and runs eight threads against two of them.  Here it is built twice with the host C++
compiler — address + undefined-behaviour, and thread sanitizer — and each build runs as a child process of its own.
Nothing is preloaded; neither libigcn.so nor Python code is involved.
"""
import os
import shutil
import subprocess

import pytest
from conftest import ROOT, has_gpu

SRC = os.path.join(ROOT, "tests", "host", "pending_check.cpp")
MODES = {"asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}


def _compiler():
    for c in ("g++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c)
        if path:
            return path
    return None


@pytest.mark.parametrize("mode", sorted(MODES))
def test_pending_registry_is_clean_under_sanitizers(mode, tmp_path):
    if has_gpu():
        pytest.skip("sanitizer runs belong on the CPU machine")
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ or the ROCm clang++)")
    exe = str(tmp_path / f"pending_check_{mode}")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", *MODES[mode], SRC, "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, f"{cxx} {mode}:\n{cc.stderr[-4000:]}"
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, f"{mode}: exit {run.returncode}\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}"
    assert "all checks passed" in run.stdout and "FAIL" not in run.stdout
