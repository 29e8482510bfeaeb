"""The host side of the quad route (AFQ_THERMAL_QUAD) without a GPU: a stand-alone program
(tests/thermal_quad_sizes_main.cpp, built here with the project's compiler and AddressSanitizer and UBSan on the host side)
runs the quad LDS and scratch size functions of pauxy_amd/csrc/thermal_wide.h, the bound they leave and th_screen_bound
with the quad kernels and, unchanged, with the 128 columns of two per lane, on a handle that holds nothing but M.  No
device is touched, no kernel is launched, and no Python process runs under a sanitizer."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

CHECKS = [
    "lds-is-the-vectors-at-256", "lds-is-twice-the-far-kernels", "lds-fits-a-work-group", "scratch-is-the-far-routes",
    "scratch-at-147-and-256", "scratch-bytes-of-256-walkers-in-size_t", "bound-is-256", "far-bound-is-still-128",
    "screen-passes-to-256", "screen-refuses-257-sites", "screen-refuses-305-plane-waves", "screen-refuses-a-million",
    "screen-words-128-columns-as-before", "screen-words-64-lanes-as-before",
]


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("thermal_quad_sizes") / "thermal_quad_sizes_main")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function",
                           "-Wno-unused-value", "-Wno-unused-result", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           os.path.join(HERE, "thermal_quad_sizes_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert not out.stderr, out.stderr[-4000:]
    lines = out.stdout.splitlines()
    assert all(re.match(r"(ok|FAIL) \S+", ln) for ln in lines), out.stdout
    got = {ln.split()[1].rstrip(":"): ln for ln in lines}
    assert len(got) == len(lines)
    assert out.returncode == (1 if any(ln.startswith("FAIL") for ln in lines) else 0)
    return got


@pytest.mark.parametrize("name", CHECKS)
def test_quad_sizes_and_bound_on_the_host(verdicts, name):
    assert verdicts.get(name) == "ok " + name, verdicts.get(name)


def test_the_program_ran_nothing_this_list_does_not_name(verdicts):
    assert sorted(verdicts) == sorted(CHECKS)
