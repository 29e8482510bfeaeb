#!/usr/bin/env python3
"""Same-build comparison of afq_set_step_handover on the C3 headline: ONE population and one handle, the switch flipped
between timed regions (on, off, on, off, ...), each region --steps batched steps bracketed by a device synchronise.
   python tools/step_handover_ab.py [--steps 100] [--warmup 20] [--repeats 3]
afq_counters_ext [9] is asserted per region: walker steps start from the hand-over with the switch on and never with it off.
Prints one JSON line: ms per step of every region, the share of walker steps that consumed, the medians, spreads, gain and
whether it counts (gain > 3 x the larger spread)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from pauxy_amd.qmc.afqmc import AFQMC
    system, trial = bench.build_inputs()
    options = {
        'qmc': {'timestep': bench.DT, 'num_steps': bench.NSTEPS_BLOCK, 'blocks': 10 ** 6, 'stabilise_freq': bench.NSTBLZ,
                'pop_control_freq': bench.NPOP, 'num_walkers': bench.NW_PER_GPU, 'rng_seed': 7},
        'propagator': {'device_rng': True, 'rng_seed': 7, 'rng_stream': 0},
        'estimators': {'mixed': {'verbose': False}, 'write_file': False},
    }
    afqmc = AFQMC(comm=None, options=options, system=system, trial=trial)
    dev = afqmc.psi.dev
    t_heat = time.perf_counter()
    while time.perf_counter() - t_heat < 0.3:
        dev.greens(want_G=False, fetch=False)
        for _ in range(8):
            dev.local_energy(fetch=False)
        dev.sync()
    eshift = afqmc.run_batched(args.warmup, first_step=1, eshift=0.0)
    dev.sync()
    first = args.warmup + 1
    ms = {1: [], 0: []}
    dev.counters(reset=True, n=10)
    share = []
    for _ in range(args.repeats):
        for on in (1, 0):
            dev.set_step_handover(on)
            before = int(dev.counters(n=10)[9])
            t0 = time.perf_counter()
            eshift = afqmc.run_batched(args.steps, first_step=first, eshift=eshift)
            dev.sync()
            ms[on].append(1e3 * (time.perf_counter() - t0) / args.steps)
            first += args.steps
            took = int(dev.counters(n=10)[9]) - before
            assert (took > 0) == bool(on), (on, took)
            if on:
                share.append(took / float(args.steps * bench.NW_PER_GPU))

    def med(v):
        return sorted(v)[(len(v) - 1) // 2]

    spread = max(max(v) - min(v) for v in ms.values())
    gain = med(ms[0]) - med(ms[1])
    print(json.dumps({"steps": args.steps, "ms_per_step_on": ms[1], "ms_per_step_off": ms[0], "median_on": med(ms[1]),
                      "median_off": med(ms[0]), "consuming_share_on": share, "larger_spread": spread, "gain_ms_per_step": gain,
                      "counts": gain > 3.0 * spread}))


if __name__ == "__main__":
    main()
