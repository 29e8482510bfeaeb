"""The host side of the far route (AFQ_THERMAL_FAR) without a GPU: a stand-alone program
(tests/thermal_far_sizes_main.cpp, built here with the project's compiler and AddressSanitizer and UBSan on the host side)
runs the LDS and scratch size functions of pauxy_amd/csrc/thermal_wide.h, the bound they leave and th_screen_bound with
the far kernels, on a handle that holds nothing but M.  No device is touched, no kernel is launched, and no Python
process runs under a sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

CHECKS = [
    "lds-is-the-vectors", "lds-is-the-wide-kernels-less-its-matrix", "scratch-is-four-buffers-and-w", "scratch-at-123",
    "scratch-in-size_t", "scratch-bytes-of-256-walkers", "bound-is-128", "screen-passes-to-128", "screen-refuses-129-sites",
    "screen-refuses-171-plane-waves", "screen-refuses-a-million", "screen-names-bytes-of-a-kernel-that-does-not-fit",
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("thermal_far_sizes") / "thermal_far_sizes_main")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Wno-unused-value", "-Wno-unused-result", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "thermal_far_sizes_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert not out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert all(re.match(r"(ok|FAIL) \S+", ln) for ln in lines), out.stdout
    got = {ln.split()[1].rstrip(":"): ln for ln in lines}
    assert len(got) == len(lines)
    assert out.returncode == (1 if any(ln.startswith("FAIL") for ln in lines) else 0)
    return got


@pytest.mark.parametrize("name", CHECKS)
def test_far_sizes_and_bound_on_the_host(verdicts, name):
    assert verdicts.get(name) == "ok " + name, verdicts.get(name)


def test_the_program_ran_nothing_this_list_does_not_name(verdicts):
    assert sorted(verdicts) == sorted(CHECKS)
