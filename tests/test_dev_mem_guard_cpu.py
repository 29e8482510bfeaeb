"""The guard mode of the handle's device memory (pauxy_amd/csrc/dev_guard.h, dev_mem.h; AFQ_DEBUG_GUARD) without a GPU: a
stand-alone program (tests/dev_mem_guard_main.cpp, built here with the host compiler under AddressSanitizer and UBSan) runs
the allocation, fill, check and free logic over a host shim of the five runtime calls it uses (tests/dev_mem_shim.h), so the
sanitizers see every byte the logic touches.  No Python process runs under a sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

from pauxy_amd import _lib as L
from tests import between_steps_cases as bs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

CHECKS = [
    "untouched-mode1", "untouched-mode2", "aligned-mode1", "aligned-mode2", "poison-typed",
    "byte-before", "byte-behind", "byte-front-far", "byte-back-far", "byte-behind-odd-size", "byte-back-far-odd-size",
    "complex-store-past-end", "reported-at-replace", "reported-at-release", "reported-at-scope-exit", "devtemp-untouched",
    "mode0-exact", "environment", "nothing-left-live",
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("dev_mem_guard") / "dev_mem_guard_main")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DAFQ_DEV_MEM_HOST_SHIM", "-I", HERE,
                           os.path.join(HERE, "dev_mem_guard_main.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("AFQ_DEBUG_GUARD")}
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert not out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert all(re.match(r"(ok|FAIL) \S+", ln) for ln in lines), out.stdout
    got = {ln.split()[1].rstrip(":"): ln for ln in lines}
    assert len(got) == len(lines)
    assert out.returncode == (1 if any(ln.startswith("FAIL") for ln in lines) else 0)
    return got


@pytest.mark.parametrize("name", CHECKS)
def test_guard_logic_on_the_host(verdicts, name):
    assert verdicts.get(name) == "ok " + name, verdicts.get(name)


def test_the_program_ran_nothing_this_list_does_not_name(verdicts):
    assert sorted(verdicts) == sorted(CHECKS)


def test_guard_headers_reach_the_runtime_through_the_shim_switch_only():
    for name in ("dev_guard.h", "dev_mem.h"):
        text = open(os.path.join(ROOT, "pauxy_amd", "csrc", name)).read()
        assert text.count("hip/hip_runtime.h") == (1 if name == "dev_guard.h" else 0)
    guard = open(os.path.join(ROOT, "pauxy_amd", "csrc", "dev_guard.h")).read()
    assert re.search(r'#ifdef AFQ_DEV_MEM_HOST_SHIM\n#include "dev_mem_shim.h"\n#else\n#include <hip/hip_runtime.h>\n#endif', guard)
    # the handle's blocks are allocated and freed in one place each
    mem = open(os.path.join(ROOT, "pauxy_amd", "csrc", "dev_mem.h")).read()
    assert "hipMalloc(" not in mem and "hipFree(" not in mem
    ueg = open(os.path.join(ROOT, "pauxy_amd", "csrc", "k_ueg.hip")).read()
    assert "hipMalloc(" not in ueg and "hipFree(" not in ueg


def test_entry_points_are_declared_bound_and_classified():
    text = open(os.path.join(ROOT, "include", "afqmc_hip.h")).read()
    assert re.search(r"^int afq_debug_guard_check\(afq_handle \*h\);", text, re.M)
    assert re.search(r"^int afq_debug_guard_report\(char \*buf, int n\);", text, re.M)
    assert re.search(r"^void afq_debug_guard_reset\(void\);", text, re.M)
    for name in ("afq_debug_guard_check", "afq_debug_guard_report", "afq_debug_guard_reset"):
        assert name in L.SIGNATURES and name in bs.EXEMPT
    lib = L.load()
    assert int(lib.afq_debug_guard_check(None)) == L.AFQ_EINVAL
    import ctypes
    lib.afq_debug_guard_reset()
    buf = ctypes.create_string_buffer(64)
    assert int(lib.afq_debug_guard_report(buf, 64)) == 0 and buf.value == b""
    assert int(lib.afq_debug_guard_report(None, 0)) == 0


def test_benchmark_never_selects_the_mode():
    assert "AFQ_DEBUG_GUARD" not in open(os.path.join(ROOT, "bench.py")).read()
