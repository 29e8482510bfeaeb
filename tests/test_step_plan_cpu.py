"""The launch plan of the fused propagator (pauxy_amd/csrc/step_plan.h) computed on the host, without a GPU: a stand-alone
program (tests/step_plan_main.cpp, built here with the host compiler under AddressSanitizer and UBSan) walks the cases of
tests.test_gpu_step_plan and prints, per step, the instantiation the plan names and plan_issued_flops.  Both must equal
what the library launched and counted on the device with the build before the plan -- the literals of that file: the
benchmark's frac < frac_issued gate rests on this count agreeing with the launch."""
import os
import shutil
import subprocess

import pytest

from tests.test_gpu_step_plan import BEFORE, CASES, KINDS, ORDER, TRACES

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def facts_line(c):
    """The facts the handle would hold for tests.test_gpu_step_plan.population: a real trial, closed where na == nb; psi^H B
    and B B exist for such a trial and one real one-body matrix; the force bias contracts the spin sum -- the kind of step
    whose Green's function can ride -- with more than 32 walkers of a closed trial (k_fb_use_sum)."""
    M, na, nb, nw = c['M'], c['na'], c['nb'], c['nw']
    same_b, b_real = c['onebody'] != 'spin-real', c['onebody'] != 'same-complex'
    closed = na == nb
    nmax = max(na, nb)
    tail_lds = 16 * (2 * (nmax * nmax + 2 * nmax) + ((2 * nmax + 3) // 4 + 1) + M * (na + nb))       # greens_fill's size
    switch = lambda key, default: default if c[key] is None else c[key]
    vals = [M, na, nb, nw, ORDER, same_b, b_real, switch('closed_form', 0), switch('fusion', 2), switch('scope', 0),
            switch('overlap', 1), switch('handover', 1), closed and nw > 32, True, closed, closed and same_b and b_real,
            tail_lds, len(KINDS)] + [how == 'announced' for how in KINDS]
    return " ".join(str(int(v)) for v in vals)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("step_plan") / "step_plan_main")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(HERE, "step_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe], input="\n".join(facts_line(c) for c in CASES) + "\n", capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(CASES) * len(KINDS)
    return {c['name']: lines[i * len(KINDS):(i + 1) * len(KINDS)] for i, c in enumerate(CASES)}


@pytest.mark.parametrize("name", [c['name'] for c in CASES])
def test_plan_names_and_counts_the_launch_the_device_made(plans, name):
    for line, (trace, _c3, _c9, per_walker, total, _sha) in zip(plans[name], BEFORE[name]):
        variant, flops, fields = line.split("|")
        launched = [n for n, _count in TRACES[trace] if 'prop_fused_kernel' in n]
        assert "REFUSED" not in fields
        if not variant:                             # (not a shape of the fused propagator: the GEMM chain ran)
            assert "supported 0" in fields and launched == []
            continue
        assert launched == [variant], (line, launched)
        o, c, t = (float(x) for x in flops.split())
        assert (o, c) == per_walker and t == total, (line, per_walker, total)


def test_plan_header_is_plain_cxx():
    text = open(os.path.join(HERE, "..", "pauxy_amd", "csrc", "step_plan.h")).read()
    assert "#include <cstddef>" in text and text.count("#include") == 1
