#!/usr/bin/env python3
"""Time of one population-control event, by hipEvent on the handle's stream: afq_popcontrol_pair_branch next to
afq_popcontrol_comb on the same handle, C3-size walkers (M = 100, 25 + 25 electrons, K = 500), 256 and 2048 walkers,
120 events each after 5 that are not counted.  Every event starts from fresh log-normal weights (sigma 0.5) with a few
strays, is enqueued without read-back, and includes the upload of its uniforms.  A second pass (20 events of each kind
under afq_launch_trace) gives the time of every kernel of an event.

Usage:  python tools/pair_branch_event_time.py [--out profiles/pair_branch_event_time.json]
"""
import ctypes
import json
import os
import sys

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import afqmc_ref as ref
from pauxy_amd import _lib as L
from pauxy_amd.systems import synthetic_generic
from pauxy_amd.trial import rhf_trial_generic
from pauxy_amd.propagation.setup import generic_propagator_arrays
from tests.helpers import make_device

M, K, N, NEV = 100, 500, 25, 120
system = synthetic_generic(M, K, (N, N), seed=7)
trial = rhf_trial_generic(system)
BH1, mf_shift = generic_propagator_arrays(system, trial, 0.005)
model = ref.RefModel('generic', M, N, N, trial.psi, BH1, mf_shift, 0.005, hs_pot=system.hs_pot, rchol=trial._rchol,
                     H1=system.H1.astype(complex), ecore=system.ecore)
out = {'M': M, 'K': K, 'nelec': [N, N], 'events': NEV, 'cases': []}
for nw in (256, 2048):
    dev = make_device(model, nw)
    hip = dev.lib
    stream = ctypes.c_void_p()
    assert hip.afq_stream(dev.h, ctypes.byref(stream)) == 0
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    rng = numpy.random.RandomState(nw)
    phi = trial.psi[None] + 0.01 * (rng.rand(nw, M, 2 * N) + 1j * rng.rand(nw, M, 2 * N))
    dev.set(L.F_PHI, phi)
    dev.set(L.F_OT, dev.calc_overlap())
    res = {}
    for kind in ('pair_branch', 'comb'):
        ms = []
        for ev in range(NEV + 5):
            # a population a long run sees between events: log-normal weights, sigma 0.5, plus a few strays
            w = numpy.exp(0.5 * rng.normal(size=nw))
            w[rng.randint(0, nw, nw // 32)] *= rng.choice([0.02, 6.0], nw // 32)
            dev.set(L.F_WEIGHT, w)
            u = rng.rand(nw // 2)
            assert hip.hipEventRecord(e0, stream) == 0
            if kind == 'comb':
                dev.popcontrol_comb(float(u[0]), nw, fetch=False)
            else:
                dev.popcontrol_pair_branch(u, nw, 0.1, 4.0, fetch=False)
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
            t = ctypes.c_float()
            assert hip.hipEventElapsedTime(ctypes.byref(t), e0, e1) == 0
            if ev >= 5:
                ms.append(t.value)
        ms = numpy.array(ms)
        res[kind] = {'median_us': float(numpy.median(ms) * 1e3), 'mean_us': float(ms.mean() * 1e3),
                     'min_us': float(ms.min() * 1e3), 'max_us': float(ms.max() * 1e3)}
    # where an event's time goes: a separate pass with an event pair around every launch (the events themselves add
    # to the stream, so these are per-kernel times, not a second measurement of the whole event)
    dev.launch_trace(True)
    for ev in range(40):
        w = numpy.exp(0.5 * rng.normal(size=nw))
        w[rng.randint(0, nw, nw // 32)] *= rng.choice([0.02, 6.0], nw // 32)
        dev.set(L.F_WEIGHT, w)
        u = rng.rand(nw // 2)
        if ev % 2:
            dev.popcontrol_comb(float(u[0]), nw, fetch=False)
        else:
            dev.popcontrol_pair_branch(u, nw, 0.1, 4.0, fetch=False)
    dev.sync()
    res['kernels_us'] = {name: {'launches': n, 'mean_us': 1e3 * ms / n} for name, (n, ms) in dev.launch_trace_get().items() if n}
    dev.launch_trace(False)
    res['nw'] = nw
    out['cases'].append(res)
    print(json.dumps(res), flush=True)
    dev.close()
path = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'pair_branch_event_time.json')
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, 'w') as f:
    json.dump(out, f, indent=1)
