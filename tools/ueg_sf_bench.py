#!/usr/bin/env python3
"""Cost of back-propagated UEG energies + structure factor at the C2 sizes (UEG(2.0, 7, 7, 4.0): 93 plane waves, 750
momentum transfers, 256 walkers), per 40-step back-propagation window.  Prints one JSON line.

For the reference's index lists (first nup plane waves) and the complete ones (full_lists=True):
  off     afq_bp_update with neither option (the path this work leaves unchanged)
  on      afq_bp_update_ext with evaluate_energy and the structure factor
  extra   on - off (medians), next to the library's own per-launch event pairs (afq_launch_trace) for the new kernels
Timed from the host around the call, stream synchronised before and after; 5 warm-up + 20 timed windows, median and
the run-to-run spread (min, max).  Every window is preceded by its 40 propagation steps (not timed).

  python tools/ueg_sf_bench.py [--windows 20] [--warmup 5]
  python tools/ueg_sf_bench.py --parent-library /path/to/libafqmc_hip.so    adds 'off' measured with that build of the
                                                                           library (a child process; older builds
                                                                           lack the new entry points: 'off' only)
  rocprofv3 --kernel-trace --stats -- python tools/ueg_sf_bench.py --profile full
                                                                           only the 'on' windows of one list kind,
                                                                           for a kernel trace (no counters)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pauxy_amd import _lib as L                                    # noqa: E402

if os.environ.get("AFQ_LIBRARY"):
    # another build of the library: keep the entry points it has (an older one lacks the newest)
    _probe = ctypes.CDLL(os.environ["AFQ_LIBRARY"])
    for _name in [n for n in L.SIGNATURES if not hasattr(_probe, n)]:
        del L.SIGNATURES[_name]

from pauxy_amd import systems, trial as trial_mod                  # noqa: E402
from pauxy_amd.device import AfqDevice                             # noqa: E402
from pauxy_amd.propagation import setup                            # noqa: E402

NW, NBP, DT = 256, 40, 0.005
NEW_KERNELS = ('ueg_pair_kernel', 'ueg_pair_finish_kernel', 'ueg_sf_wsum_kernel')


def device(full):
    s = systems.UEG(2.0, 7, 7, 4.0, **({'full_lists': True} if full else {}))
    t = trial_mod.hartree_fock_ueg(s)
    BH1, mf = setup.ueg_propagator_arrays(s, t, DT)
    H1diag = numpy.array([numpy.diag(s.H1[0]).real, numpy.diag(s.H1[1]).real])
    dev = AfqDevice(0)
    dev.set_system_ueg(s.iA, s.iB, s.ikpq_i, s.ikpq_kpq, s.ipmq_i, s.ipmq_pmq, s.vqvec, s.vol, H1diag, s.ecore, 7, 7)
    dev.set_trial(t.psi)
    dev.set_propagator(BH1, mf, DT)
    dev.walkers_alloc(NW)
    rng = numpy.random.RandomState(1)
    M, ne = s.nbasis, 14
    dev.set(L.F_PHI, numpy.array([t.psi + 0.05 * (rng.rand(M, ne) + 1j * rng.rand(M, ne)) for _ in range(NW)]))
    dev.set(L.F_OT, dev.calc_overlap())
    dev.bp_configure(NBP)
    lens = [len(a) * len(b) for a, b in zip(s.ikpq_i, s.ipmq_i)]
    info = {'M': M, 'nq': len(s.qvecs), 'longest_list': int(max(len(a) for a in s.ikpq_i)),
            'empty_q': int(sum(1 for x in lens if x == 0)), 'pairs_per_spin_and_G': int(sum(lens))}
    return dev, t.psi, rng, info


def windows(dev, psi, rng, n, on):
    out = []
    for _ in range(n):
        for i in range(NBP):
            dev.propagate(rng.normal(size=(NW, dev.K)), 0.0)
            if i % 10 == 9:
                dev.reortho(fetch=False)
        dev.sync()
        t0 = time.perf_counter()
        if on:
            dev.bp_update(psi, 10, None, True, reset=True, two_rdm=True)
        else:
            dev.bp_update(psi, 10, None, False, reset=True)
        dev.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stats(ms):
    return {'median_ms': round(float(numpy.median(ms)), 4), 'min_ms': round(float(min(ms)), 4),
            'max_ms': round(float(max(ms)), 4)}


def run(full, nwin, warmup, off_only=False):
    dev, psi, rng, info = device(full)
    row = dict(info)
    windows(dev, psi, rng, warmup, False)
    row['off'] = stats(windows(dev, psi, rng, nwin, False))
    if not off_only:
        dev.bp_observables(two_rdm='structure_factor')
        windows(dev, psi, rng, warmup, True)
        row['on'] = stats(windows(dev, psi, rng, nwin, True))
        row['extra_ms'] = round(row['on']['median_ms'] - row['off']['median_ms'], 4)
        dev.launch_trace(True)
        windows(dev, psi, rng, 5, True)
        tr = dev.launch_trace_get()
        dev.launch_trace(False)
        row['new_kernels_us_per_window'] = {k: round(v[1] * 1e3 / 5, 2) for k, v in tr.items()
                                            if k.startswith(NEW_KERNELS)}
        row['window_kernels_us_total'] = round(sum(v[1] for k, v in tr.items()) * 1e3 / 5, 1)
    dev.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--off-only', action='store_true')
    ap.add_argument('--parent-library', default=None)
    ap.add_argument('--profile', choices=['truncated', 'full'], default=None)
    a = ap.parse_args()
    if a.profile:
        dev, psi, rng, _ = device(a.profile == 'full')
        dev.bp_observables(two_rdm='structure_factor')
        windows(dev, psi, rng, 3, True)
        dev.close()
        return
    out = {'config': 'C2 UEG(2.0, 7, 7, 4.0)', 'nw': NW, 'window_steps': NBP, 'windows': a.windows, 'warmup': a.warmup,
           'timing': 'host clock around afq_bp_update(_ext), stream synchronised before and after'}
    for tag, full in (('truncated_lists', False), ('full_lists', True)):
        if a.off_only and full and 'full_lists' not in systems.UEG.__init__.__code__.co_varnames:
            continue
        out[tag] = run(full, a.windows, a.warmup, a.off_only)
    if a.parent_library:
        env = dict(os.environ, AFQ_LIBRARY=a.parent_library)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--off-only', '--windows', str(a.windows),
                            '--warmup', str(a.warmup)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            out['parent_library_error'] = r.stderr[-400:]
        else:
            p = json.loads(r.stdout.strip().splitlines()[-1])
            for tag in ('truncated_lists', 'full_lists'):
                if tag in p:
                    out[tag]['off_parent_library'] = p[tag]['off']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
