"""The IGCN_* switch table (igcn_amd/switches.py) against the code that reads the environment, the library's option bits,
INTEGRATION §4 and the GPU tests that flip each switch.  No GPU: nothing here loads the library."""
import ast
import glob
import os
import re

import pytest

from conftest import ROOT
from igcn_amd import switches

PKG = os.path.join(ROOT, "ig-gcn_amd")
READ = re.compile(r'(?:environ\.get\(|environ\[|getenv\()\s*"(IGCN_[A-Z0-9_]+)"')
BUILD_TIME = {"IGCN_HIPCC_EXTRA"}           # build.py's extra hipcc flags: part of the build digest, not a runtime switch


def _sources():
    for path in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True) + glob.glob(os.path.join(PKG, "csrc", "*"))):
        with open(path) as f:
            yield os.path.relpath(path, PKG), f.read()


def test_every_environment_read_is_in_the_table():
    reads = {}
    for rel, text in _sources():
        for name in READ.findall(text):
            reads.setdefault(name, set()).add(rel)
    assert "IGCN_DEBUG_SYNC" in reads                        # (the pattern sees the reads that are there)
    assert set(reads) - BUILD_TIME <= switches.ALL, sorted(set(reads) - BUILD_TIME - switches.ALL)
    # outside the table module, only _lib.py (IGCN_DEBUG_SYNC at import) and build.py read the environment themselves
    assert set().union(*reads.values()) <= {"_lib.py", "build.py"}, reads


def test_library_bits_match_common_h():
    with open(os.path.join(PKG, "csrc", "common.h")) as f:
        macros = re.findall(r"#define\s+IGCN_OPT_([A-Z0-9_]+)\s+(\d+)u", f.read())
    assert [("IGCN_" + name, int(bit)) for name, bit in macros] == \
        [(name, 1 << k) for k, (name, _) in enumerate(switches.LIBRARY)]


def test_every_entry_is_documented_once():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = text[text.index("## 4."):text.index("## 5.")]
    counts = {name: len(re.findall(rf"\b{name}\b", section)) for name in sorted(switches.ALL)}
    assert all(n == 1 for n in counts.values()), {k: n for k, n in counts.items() if n != 1}


def test_library_mask_reads_only_1_as_on():
    names = [name for name, _ in switches.LIBRARY]
    assert switches.library_mask({}) == 0
    assert switches.library_mask({n: "0" for n in names}) == 0
    assert switches.library_mask({n: "" for n in names}) == 0
    assert switches.library_mask({n: "1" for n in names}) == (1 << len(names)) - 1
    assert switches.library_mask({"IGCN_PROPAGATE_NO_LDS": "1", "IGCN_NO_TILED_LISTS": "0",
                                  "IGCN_ATTN_EXACT_FP32": "1", "IGCN_NO_DEFER": "1"}) == 2 | 128
    assert switches.knob("IGCN_GEMM_BN", {}) == 0 and switches.knob("IGCN_GEMM_BN", {"IGCN_GEMM_BN": ""}) == 0
    assert switches.knob("IGCN_ATTN_CHUNK", {"IGCN_ATTN_CHUNK": "64"}) == 64


def test_host_switch_reads_only_1_as_on(monkeypatch):
    monkeypatch.setenv("IGCN_NO_DEFER", "0")
    assert not switches.on("IGCN_NO_DEFER")
    monkeypatch.setenv("IGCN_NO_DEFER", "1")
    assert switches.on("IGCN_NO_DEFER")
    with pytest.raises(KeyError):
        switches.on("IGCN_NO_DEFFER")
    with pytest.raises(KeyError):
        switches.on("IGCN_PROPAGATE_NO_LDS")                # a library bit: read once, at load, never per use


def test_every_switch_is_flipped_by_a_gpu_test():
    texts = {}
    for path in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")):
        with open(path) as f:
            texts[os.path.basename(path)] = f.read()
    flipped = set()
    for text in texts.values():
        flipped |= set(re.findall(r'setenv\("(IGCN_[A-Z0-9_]+)", "1"\)', text))
        flipped |= set(re.findall(r'"(IGCN_[A-Z0-9_]+)": "1"', text))
    # the train-step test takes every host switch from the table, less those it names as not reached by that step
    model = texts["test_gpu_model.py"]
    assert "sorted(set(switches.HOST) - set(_NOT_IN_THE_TRAIN_STEP))" in model
    not_reached = next(ast.literal_eval(node.value) for node in ast.parse(model).body if isinstance(node, ast.Assign)
                       and getattr(node.targets[0], "id", None) == "_NOT_IN_THE_TRAIN_STEP")
    flipped |= set(switches.HOST) - set(not_reached)
    want = (set(switches.HOST) | {n for n, _ in switches.LIBRARY}) - switches.EXEMPT
    assert want <= flipped, sorted(want - flipped)
