"""Mixed estimator on the device, behind PAUXY's ``Mixed`` surface.

Mirrors pauxy/estimators/mixed.py:33-371 (``Mixed``: ``update``, ``print_step``,
``get_shift``, ``names``, ``estimates``) and the free function
``local_energy`` (:383-437).  ``update`` accumulates the ten estimators of
:460-469 with one device launch (plus the batched Green's function + local
energy launches on energy steps) instead of a Python loop over walkers.

Output: the per-block rows are kept in ``self.blocks`` (and printed when
``verbose``); when the container was given a file name the root rank also pushes
them to ``basic/energies/<block>`` with ``basic/headers`` (mixed.py:278,368-371;
layout in pauxy_amd/estimators/utils.py).

``two_rdm: 'structure_factor'`` (UEG, importance sampling): every update that evaluates the energy also accumulates
sum_w weight_w Re two_rdm[G_w] on the device, two_rdm[2, 2, nq] being what local_energy_ueg(system, G, two_rdm=...)
fills.  Per block the root pushes ``basic/two_rdm/<block>`` = (the accumulator summed over ranks) / (the block's global
EDenom) and keeps it in ``self.two_rdm``: the energy's own estimator per momentum transfer, so that
1 / (2 vol) * vqvec . two_rdm.sum((0, 1)) of a block is that block's E2Body.  (The reference's non-thermal branch never
hands its two_rdm array to the energy call, mixed.py:214, and writes zeros; this normalisation is this package's.)

Thermal walkers (``qmc.beta``) with ``Mixed(..., thermal_sweep=True)`` -- what ``ThermalAFQMC`` passes; without the
keyword the three options are refused as before -- take ``one_rdm: True``, ``two_rdm: 'structure_factor'`` (UEG) and
``average_gf: True`` (mixed.py:180-233): the library's afq_thermal_estimates makes every walker's sums in one call.
Per block ``basic/one_rdm/<block>`` = sum_w weight_w Re G_w / nsteps / Weight [2, M, M] and ``basic/two_rdm/<block>`` =
sum_w weight_w Re two_rdm[P_w] / nsteps / Weight [2, 2, nq] with P_w = I - G_w^T: for thermal walkers this is the
reference's normalisation (mixed.py:279-287), not the ground state's / EDenom above.
One deliberate deviation: with ``average_gf`` EDenom accumulates the walkers' weights.  The reference's ``average_gf``
branch (mixed.py:182-199) has no EDenom line, so its ETotal, E1Body and E2Body columns are +-inf or NaN; the numerators
(ENumer and the raw one- and two-body sums), Nav, Weight and the RDMs are the reference's.
"""
import time

import numpy


class _Enum(dict):
    __getattr__ = dict.__getitem__


def get_estimator_enum(thermal=False):
    keys = ['uweight', 'weight', 'enumer', 'edenom', 'eproj', 'e1b', 'e2b', 'ehyb', 'ovlp']
    if thermal:
        keys.append('nav')                                              # mixed.py:463-464
    keys.append('time')
    return _Enum((k, v) for v, k in enumerate(keys))


class Mixed(object):
    calc_two_rdm = None
    structure_factor = False
    _sf_armed = False
    thermal = False             # set with a finite-temperature run (qmc.beta, mixed.py:87-92): the Nav column

    average_gf = False          # thermal, with thermal_sweep: energies and Nav averaged over the stack_length Green's functions

    def __init__(self, mixed, system, root, filename, qmc, trial, dtype=complex, thermal_sweep=False):
        if getattr(qmc, 'beta', None) is not None:
            self.thermal = True
            if not thermal_sweep:
                if mixed.get('average_gf', False):
                    raise NotImplementedError("mixed estimator: average_gf is not supported with a thermal trial "
                                              "(Mixed(..., thermal_sweep=True), which ThermalAFQMC passes, takes it)")
                if mixed.get('one_rdm', False) or mixed.get('two_rdm', None) is not None:
                    raise NotImplementedError("mixed estimator: one_rdm / two_rdm are not supported with a thermal trial "
                                              "(Mixed(..., thermal_sweep=True), which ThermalAFQMC passes, takes them)")
            self.average_gf = bool(mixed.get('average_gf', False))
        self.eval_energy = mixed.get('evaluate_energy', True)
        self.calc_one_rdm = mixed.get('one_rdm', False)
        two = mixed.get('two_rdm', None)
        if two is not None:
            if not (isinstance(two, str) and two == 'structure_factor' and system.name == "UEG"):
                raise NotImplementedError("mixed two_rdm: only 'structure_factor' on a UEG system")
            # (set only with the option: without it the instance holds what it held before)
            self.calc_two_rdm = two
            self.structure_factor = True
            self.sf_acc = numpy.zeros((2, 2, len(system.qvecs)))
            self.two_rdm = []                                           # per block, as pushed to 'two_rdm'
        self.G = numpy.zeros((2, system.nbasis, system.nbasis))          # mixed.py:99
        self.rdm_acc = numpy.zeros_like(self.G)
        self.one_rdm = []                                               # per block, as pushed to 'one_rdm'
        self._rdm_armed = False
        self.energy_eval_freq = mixed.get('energy_eval_freq', None)
        if self.energy_eval_freq is None:
            self.energy_eval_freq = qmc.nsteps                      # mixed.py:78-80
        self.verbose = mixed.get('verbose', True)
        self.nsteps = qmc.nsteps
        self.header = ['Iteration', 'WeightFactor', 'Weight', 'ENumer', 'EDenom', 'ETotal', 'E1Body',
                       'E2Body', 'EHybrid', 'Overlap', 'Time']
        if self.thermal:
            self.header.insert(len(self.header) - 1, 'Nav')
        self.nreg = len(self.header[1:])
        self.dtype = dtype
        self.names = get_estimator_enum(self.thermal)
        self.estimates = numpy.zeros(self.nreg, dtype=dtype)
        self.estimates[self.names.time] = time.time()
        self.global_estimates = numpy.zeros(self.nreg, dtype=dtype)
        self.eshift = numpy.array([0, 0])
        self.key = {                                                    # mixed.py:113-126
            'Iteration': "Simulation iteration. iteration*dt = tau.",
            'WeightFactor': "Rescaling Factor from population control.",
            'Weight': "Total walker weight.",
            'E_num': "Numerator for projected energy estimator.",
            'E_denom': "Denominator for projected energy estimator.",
            'ETotal': "Projected energy estimator.",
            'E1Body': "Mixed one-body energy estimator.",
            'E2Body': "Mixed two-body energy estimator.",
            'EHybrid': "Hybrid energy.",
            'Overlap': "Walker average overlap.",
            'Nav': "Average number of electrons.",
            'Time': "Time per processor to complete one iteration.",
        }
        self.blocks = []
        self.root = root
        self.flush_every = mixed.get('flush_every', None)
        self.output = None
        if root and filename is not None:
            self.setup_output(filename)

    def update(self, system, qmc, trial, psi, step, free_projection=False):
        """mixed.py:133-233: importance-sampling branch (:210-225) or, when the propagator was
        built with free_projection, the complex wfac = weight*ot*phase accumulation of :151-175
        (the device handle knows which from afq_set_propagator)."""
        if self.thermal:
            return self.update_thermal(psi)
        if self.structure_factor and free_projection:
            raise NotImplementedError("mixed two_rdm: 'structure_factor' with free projection")
        psi._end_sweep()
        psi._flush()
        dev = psi.dev
        self.arm_rdm(dev)
        do_energy = (step % self.energy_eval_freq == 0)
        if do_energy and not self.eval_energy:
            # E, T, V = 0 but the denominator still accumulates (mixed.py:215-221)
            dev.estimates_update(False)
            est = dev.estimates_get(zero=True)
            est[self.names.edenom] += est[self.names.weight]
        else:
            dev.estimates_update(do_energy)
            est = dev.estimates_get(zero=True)
        self.estimates[:self.names.time] += est[:self.names.time]
        if self.calc_one_rdm:
            self.rdm_acc += dev.estimates_rdm_get(zero=True)            # mixed.py:226-229
        if self.structure_factor and do_energy and self.eval_energy:
            self.sf_acc += dev.estimates_sf_get(zero=True)
        if do_energy:
            psi._greens_version = psi.phi_version           # the launch refreshed Ghalf

    def update_thermal(self, psi):
        """mixed.py:200-209,222-225 for a population of thermal walkers: G rebuilt from every walker's stack at its
        current time slice (the end of the path), the energies and particle numbers from the device, the weighted
        sums -- once per path -- here."""
        if self.average_gf or self.calc_one_rdm or self.structure_factor:
            return self.update_thermal_sweep(psi)
        ns, es = self.names, self.estimates
        psi.recompute_greens_function(None)
        E, nav = psi.dev.thermal_energy()
        from pauxy_amd import _lib as L
        w = psi.dev.get(L.F_WEIGHT)
        uw = psi.dev.get(L.F_UNSCALED_WEIGHT)
        for i in range(len(w)):                                         # (walker order, as the reference sums)
            es[ns.nav] += w[i] * nav[i]
            es[ns.enumer] += w[i] * E[i, 0]
            es[ns.e1b:ns.e2b + 1] += w[i] * E[i, 1:3]
            es[ns.edenom] += w[i]
            es[ns.uweight] += uw[i]
            es[ns.weight] += w[i]
            es[ns.ovlp] += w[i] * 1.0                                   # walker.ot stays 1 (walkers/walker.py)
            es[ns.ehyb] += w[i] * 0.0                                   # walker.hybrid_energy stays 0

    def update_thermal_sweep(self, psi):
        """mixed.py:180-233 with ``average_gf``, ``one_rdm`` or ``two_rdm`` (``Mixed(..., thermal_sweep=True)``): one
        call of the library (afq_thermal_estimates) for the whole population.  With ``average_gf`` every walker's
        energies and particle number are summed over the Green's functions at slice_ix = ts * stack_size,
        ts = 0 .. stack_length - 1, multiplied by the weight and divided by stack_length (mixed.py:195-199); the RDMs
        then are the last of those Green's functions', as in the reference, whose loop leaves it on the walker."""
        from pauxy_amd import _lib as L
        ns, es = self.names, self.estimates
        if self.average_gf and getattr(psi, 'delayed_updates', False):         # (before the device is configured)
            raise NotImplementedError("mixed estimator: average_gf is not supported on a population with delayed_updates "
                                      "(the sweep kernels are the resident engine's; M <= 64 without the key)")
        psi.ensure_configured()
        if psi.dev.thermal_state()[0] != psi.time_slice:                # (the library evaluates at ITS slice counter)
            raise RuntimeError("mixed estimator: the population's time slice and the library's differ")
        res = psi.dev.thermal_estimates(average_gf=self.average_gf, one_rdm=bool(self.calc_one_rdm),
                                        two_rdm=self.structure_factor)
        cols = res['cols']
        w = psi.dev.get(L.F_WEIGHT)
        uw = psi.dev.get(L.F_UNSCALED_WEIGHT)
        nb = psi.stack_length
        for i in range(len(w)):                                         # (walker order, as the reference sums)
            if self.average_gf:
                es[ns.nav] += w[i] * cols[i, 3] / nb
                es[ns.enumer] += w[i] * cols[i, 0] / nb
                es[ns.e1b:ns.e2b + 1] += w[i] * cols[i, 1:3] / nb
            else:
                es[ns.nav] += w[i] * cols[i, 3]
                es[ns.enumer] += w[i] * cols[i, 0]
                es[ns.e1b:ns.e2b + 1] += w[i] * cols[i, 1:3]
            es[ns.edenom] += w[i]                                       # (with average_gf: this package's, see the module)
            es[ns.uweight] += uw[i]
            es[ns.weight] += w[i]
            es[ns.ovlp] += w[i] * 1.0                                   # walker.ot stays 1, walker.hybrid_energy 0
        if self.calc_one_rdm:
            self.rdm_acc += res['one_rdm']                              # mixed.py:226-229
        if self.structure_factor:
            self.sf_acc += res['two_rdm']                               # mixed.py:230-233

    def arm_rdm(self, dev):
        """one_rdm: True -> the device accumulates weight * walker.G.real with every estimator update."""
        if self.calc_one_rdm and not self._rdm_armed:
            dev.estimates_rdm(True)
            self._rdm_armed = True
        if self.structure_factor and not self._sf_armed:
            dev.estimates_sf(True)          # (the library refuses a free-projection propagator)
            self._sf_armed = True

    def print_step(self, comm, nprocs, step, nsteps=None, free_projection=False):
        """mixed.py:235-289."""
        if step % self.nsteps != 0:
            return
        if nsteps is None:
            nsteps = self.nsteps
        es = self.estimates
        ns = self.names
        es[ns.time] = (time.time() - es[ns.time]) / (1 if getattr(comm, 'already_reduced', False) else nprocs)
        es[ns.uweight:ns.weight + 1] /= nsteps
        es[ns.ehyb:ns.time + 1] /= nsteps
        comm.Reduce(es, self.global_estimates, op=None)
        gs = self.global_estimates
        # torch.distributed has no rooted reduce worth its latency: TorchComm.Reduce leaves the sums on every
        # rank, so every rank derives the shift itself and the broadcast of mixed.py:273 is not needed
        everywhere = getattr(comm, 'reduce_is_allreduce', False)
        if comm.rank == 0 or everywhere:
            gs[ns.eproj] = gs[ns.enumer]
            # A block without an energy evaluation (energy_eval_freq larger than the block) has edenom = 0: the reference
            # divides all the same (mixed.py:268: a RuntimeWarning and a NaN row).  The row is the same NaN here -- the
            # file stays comparable with the reference's -- without the warning
            with numpy.errstate(divide='ignore', invalid='ignore'):
                gs[ns.eproj:ns.e2b + 1] = gs[ns.eproj:ns.e2b + 1] / gs[ns.edenom]
            gs[ns.ehyb] /= gs[ns.weight]
            gs[ns.ovlp] /= gs[ns.weight]
            eshift = numpy.array([gs[ns.ehyb], gs[ns.eproj]])
            if self.thermal:
                gs[ns.nav] = gs[ns.nav] / gs[ns.weight]                 # mixed.py:271-272
        else:
            eshift = numpy.array([0, 0])
        if not everywhere:
            eshift = comm.bcast(eshift, root=0)
        self.eshift = eshift
        if self.calc_one_rdm and comm.size > 1 and not getattr(comm, 'already_reduced', False):
            # the RDM sums are part of the reference's one estimates vector (mixed.py:261); here they are a second buffer
            red = numpy.zeros_like(self.rdm_acc)
            comm.Reduce(self.rdm_acc, red, op=None, root=0)
            self.rdm_acc[...] = red
        if self.structure_factor and comm.size > 1 and not getattr(comm, 'already_reduced', False):
            red = numpy.zeros_like(self.sf_acc)
            comm.Reduce(self.sf_acc, red, op=None, root=0)
            self.sf_acc[...] = red
        if comm.rank == 0:
            row = [step] + list(gs[:ns.time + 1])
            self.blocks.append(numpy.array(row))
            if self.structure_factor:
                # the energy's estimator per momentum transfer: the block's sums over its (global) energy denominator
                # (thermal: the reference's own rdm / nsteps / Weight, mixed.py:284-287)
                with numpy.errstate(divide='ignore', invalid='ignore'):
                    self.two_rdm.append(self.sf_acc / nsteps / gs[ns.weight].real if self.thermal
                                        else self.sf_acc / gs[ns.edenom].real)
            if self.calc_one_rdm:                               # mixed.py:279-283
                rdm = self.rdm_acc / nsteps / gs[ns.weight].real
                self.one_rdm.append(rdm)
            if self.output is not None:
                self.output.push(row, 'energies')               # mixed.py:278
                if self.calc_one_rdm:
                    self.output.push(self.one_rdm[-1], 'one_rdm')
                if self.structure_factor:
                    self.output.push(self.two_rdm[-1], 'two_rdm')
                self.output.increment()
            if self.verbose:
                print(" ".join("{: .10e}".format(x) for x in numpy.array(row).real))
        self.zero()

    def get_shift(self, hybrid=True):
        """mixed.py:345-360."""
        return self.eshift[0].real if hybrid else self.eshift[1].real

    def projected_energy(self):
        return (self.estimates[self.names.enumer] / self.estimates[self.names.edenom]).real

    def zero(self):
        self.rdm_acc[:] = 0
        if self.structure_factor:
            self.sf_acc[:] = 0
        self.estimates[:] = 0
        self.global_estimates[:] = 0
        self.estimates[self.names.time] = time.time()

    def print_key(self, eol='', encode=False):
        """mixed.py:290-310: what the output columns are (same keys and texts, so logs read alike)."""
        header = eol + '# Explanation of output column headers:\n' + '# -------------------------------------' + eol
        print(header.encode('utf-8') if encode else header)
        for k, v in self.key.items():
            line = '# %s : %s' % (k, v) + eol
            print(line.encode('utf-8') if encode else line)

    def print_header(self, eol='', encode=False):
        print(" ".join("{:>17s}".format(x) for x in self.header) + eol)

    def setup_output(self, filename):
        """mixed.py:368-371."""
        from pauxy_amd.estimators.utils import H5EstimatorHelper
        from pauxy_amd.utils import io as _io
        with _io.h5.File(filename, 'a') as fh5:
            fh5['basic/headers'] = numpy.array(self.header).astype('S')
        self.output = H5EstimatorHelper(filename, 'basic', flush_every=self.flush_every)


def local_energy(system, G, Ghalf=None, two_rdm=None, rchol=None, eri=None, C0=None, ecoul0=None,
                 exxa0=None, exxb0=None, UVT=None, device=None):
    """pauxy.estimators.mixed.local_energy (mixed.py:383-437) for ONE Green's
    function, evaluated by the device energy kernels: ``Ghalf`` (half-rotated form) or, without it, the
    full ``G`` is used for Generic; ``G`` for Hubbard and the UEG.  ``two_rdm`` (UEG only, ignored elsewhere as in the
    reference): an array [2, 2, nq] that receives the pair sums per momentum transfer (estimators/ueg.py:71-80), with the
    system's index lists and for any ``G``.  Call-compatible with the reference:
    the device is the handle ``pauxy_amd.context`` already holds for ``system`` (the one the propagator,
    walkers and estimators of that system share); ``device=`` names another one.  The evaluation uses a
    scratch handle when the shared one carries a population (its walkers are not disturbed)."""
    from pauxy_amd import _lib as L
    from pauxy_amd import context
    if device is None:
        device = context.scratch_device(system)
    if device.nw < 1:
        device.walkers_alloc(1)
    if device.kind == 'ueg' and two_rdm is not None:
        # estimators/ueg.py:71-80: the per-q pair sums of this G go to the caller's two_rdm[2, 2, nq]
        E, two = device.ueg_pair_sums(numpy.asarray(G, dtype=numpy.complex128)[None])
        two_rdm[...] = two[0]
        return (complex(E[0, 0]), complex(E[0, 1]), complex(E[0, 2]))
    if device.kind == 'ueg':
        device.set(L.F_G, numpy.asarray(G, dtype=numpy.complex128), 0)
    else:
        if Ghalf is None:
            # estimators/generic.py:398-434 (local_energy_generic_cholesky): full-G form
            E = device.local_energy_full_g(numpy.asarray(G, dtype=numpy.complex128)[None])[0]
            return (complex(E[0]), complex(E[1]), complex(E[2]))
        device.set(L.F_GHALF, numpy.concatenate([Ghalf[0], Ghalf[1]]).astype(numpy.complex128), 0)
    E = device.local_energy()[0]
    return (complex(E[0]), complex(E[1]), complex(E[2]))
