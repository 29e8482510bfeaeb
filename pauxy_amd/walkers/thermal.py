"""Population of thermal walkers on the device (the ``trial.name == 'thermal'`` branch of walkers/handler.py:77-100
and walkers/thermal.py, walkers/stack.py of the reference).

A thermal walker is its Green's function G [2, M, M] and a stack of propagator products; both live in the library
(k_thermal.hip: Hubbard, discrete fields, real matrices; k_thermal_cplx.hip: continuous fields, complex matrices, and
with them the running product of the current bin and M0 = det G -- the UEG with its diagonal trial, and the Hubbard
model with a dense trial when a ``Continuous`` propagator configures the population).  ``walkers[i]`` are light views
with the members the reference's driver and estimators read (``weight``, ``G``, ``M0``, ``stack``, ``stack_size``,
``stack_length``, ``local_energy``, ``greens_function``)."""
import numpy

from pauxy_amd import _lib as L
from pauxy_amd.context import get_context, hidden
from pauxy_amd.propagation import thermal_continuous
from pauxy_amd.propagation.thermal_hubbard import thermal_constants
from pauxy_amd.propagation.thermal_planewave import planewave_constants
from pauxy_amd.trial_density import update_stack

def _wide_max_basis():
    """The wide route's bound as the library computes it from ts_greens_wide_lds (thermal_wide.h); a library that does
    not export it, or none built yet, leaves the literal: 16 (M (M | 1) + 1152) + 512 bytes within 160 KiB."""
    try:
        return int(L.load().afq_thermal_wide_max_basis())
    except (L.AfqLibraryError, AttributeError):
        return 95


def _far_max_basis():
    """The far route's bound as the library computes it (k_thermal_cplx.hip): no matrix in LDS, so the 128 columns of two
    per lane bind; a library that does not export it, or none built yet, leaves the literal."""
    try:
        return int(L.load().afq_thermal_far_max_basis())
    except (L.AfqLibraryError, AttributeError):
        return 128


def _quad_max_basis():
    """The quad route's bound as the library computes it (k_thermal_cplx.hip): the far placement with four columns per
    lane, 256 in all; a library that does not export it, or none built yet, leaves the literal."""
    try:
        return int(L.load().afq_thermal_quad_max_basis())
    except (L.AfqLibraryError, AttributeError):
        return 256


def _delayed_max_basis():
    """The delayed route's bound as the library computes it from its kernels' LDS (k_thermal.hip) and the 128 columns of
    two per lane; a library that does not export it, or none built yet, leaves the literal."""
    try:
        return int(L.load().afq_thermal_delayed_max_basis())
    except (L.AfqLibraryError, AttributeError):
        return 128


# The largest basis of the complex walkers by (kind, route): what fits the 160 KiB of LDS of a work-group.  The route is
# streamed_greens (False / True), 'wide' (walkers: {wide_basis: True}: one complex matrix in LDS, two columns per lane),
# 'far' (walkers: {far_basis: True}: the wide route with that matrix in device memory as well) or 'quad'
# (walkers: {quad_basis: True}: the far route with four columns per lane).
MAX_BASIS = {
    ('planewave', False): 47,            # ts_greens_lds<cplx> (thermal_strat.h): four complex matrices
    ('planewave', True): 57,             # thc_slice_lds (k_thermal_cplx.hip): three complex matrices
    ('planewave', 'wide'): _wide_max_basis(),             # ts_greens_wide_lds (thermal_wide.h): one complex matrix
    ('planewave', 'far'): _far_max_basis(),               # the lanes: two columns each
    ('planewave', 'quad'): _quad_max_basis(),             # the lanes: four columns each
    ('hubbard_continuous', False): 47,   # ts_greens_lds<cplx>
    ('hubbard_continuous', True): 63,    # thd_slice_lds (k_thermal_cplx.hip): two complex matrices and BH1
    ('hubbard_continuous', 'wide'): _wide_max_basis(),    # ts_greens_wide_lds
    ('hubbard_continuous', 'far'): _far_max_basis(),      # the lanes
    ('hubbard_continuous', 'quad'): _quad_max_basis(),    # the lanes
    # the real walkers with walkers: {delayed_updates: True}: ts_greens_wide_lds<double> fits, the lanes bind
    ('discrete', 'delayed'): _delayed_max_basis(),
}
# how the refusal speaks of a kind: whose walkers, what M counts, what the slice kernel keeps in LDS
_BOUND_WORDS = {'planewave': ("thermal walkers", "plane waves", "three complex matrices"),
                'hubbard_continuous': ("thermal walkers with continuous fields", "sites", "two complex matrices and BH1")}
# a configuration changed away from time slice 0: within a kind by what its key is, else the kind itself
_CHANGED = {'discrete': "the stabilisation period", 'planewave': "the propagator's fb_bound",
            None: "the kind of field"}


class _QmcOf(object):
    """What a propagator's constructor reads of the QMC options."""

    def __init__(self, dt, nstblz):
        self.dt, self.nstblz = dt, nstblz


class ThermalWalkerView(object):
    _h = hidden()

    def __init__(self, handler, i):
        self._h = handler
        self.index = i
        self.stack_size = handler.stack_size
        self.stack_length = handler.stack_length
        self.num_slices = handler.num_slices
        self.lowrank = False
        self.ot = 1.0
        self.hybrid_energy = 0.0

    @property
    def weight(self):
        return float(self._h.dev.get(L.F_WEIGHT, self.index, 1)[0])

    @weight.setter
    def weight(self, value):
        self._h.dev.set(L.F_WEIGHT, numpy.array([float(numpy.real(value))]), self.index)

    @property
    def unscaled_weight(self):
        return float(self._h.dev.get(L.F_UNSCALED_WEIGHT, self.index, 1)[0])

    @property
    def total_weight(self):
        return self._h.total_weight

    @property
    def G(self):
        self._h.ensure_configured()
        return self._h.dev.get(L.F_THERMAL_G, self.index, 1)[0]

    @property
    def M0(self):
        """det G_s the next weight update divides by (continuous fields)."""
        self._h.ensure_configured()
        return self._h.dev.get(L.F_THERMAL_M0, self.index, 1)[0]

    @property
    def stack(self):
        """The walker's bins [nbins, 2, M, M]."""
        self._h.ensure_configured()
        return self._h.dev.get(L.F_THERMAL_STACK, self.index, 1)[0]

    def greens_function(self, trial, slice_ix=None, inplace=True):
        """walkers/thermal.py:90-95 -- for the whole population (the library moves every walker together)."""
        if not inplace:
            raise NotImplementedError("ThermalWalker.greens_function(inplace=False)")
        self._h.recompute_greens_function(trial, slice_ix)

    def local_energy(self, system, two_rdm=None):
        """(E, T, V) of this walker's G.  ``two_rdm`` (UEG): an array [2, 2, nq] that receives the pair sums of
        P = I - G^T per momentum transfer, what local_energy_ueg(system, P, two_rdm=...) fills (walkers/thermal.py:545-547)."""
        self._h.ensure_configured()
        if two_rdm is not None:
            if system.name != "UEG":
                raise NotImplementedError("thermal walkers: two_rdm is the structure factor of the UEG")
            G = self.G
            P = numpy.array([numpy.eye(G.shape[-1]) - G[s].T for s in range(2)])
            E, two = self._h.dev.ueg_pair_sums(P[None])
            two_rdm[...] = two[0]
            return tuple(E[0].real)
        E, _ = self._h.dev.thermal_energy()
        return tuple(E[self.index])


class ThermalWalkers(object):
    ctx = hidden()
    dev = hidden()
    system = hidden()
    trial = hidden()
    _prop = hidden()

    def __init__(self, system, trial, qmc, walker_opts={}, verbose=False, comm=None, nprop_tot=None, nbp=None,
                 device_id=None):
        if comm is not None and comm.size > 1:
            raise NotImplementedError("thermal walkers: more than one rank is not supported")
        if nbp is not None or nprop_tot is not None:
            raise NotImplementedError("thermal walkers: no back-propagation or ITCF with a thermal trial")
        if system.name not in ("Hubbard", "UEG"):
            raise NotImplementedError("thermal walkers: Hubbard systems only (no Generic / UEG) with discrete fields, and "
                                      "the UEG with continuous fields; %s has no thermal path" % system.name)
        # The walker kind: 'discrete' (Hubbard, real matrices), 'planewave' (UEG: complex, diagonal trial),
        # 'hubbard_continuous' (complex, dense trial).  The UEG's is known here.  A Hubbard population's is decided by
        # the propagator that configures it (ensure_configured(prop)); `continuous_fields: True` among the walkers'
        # options announces the dense kind, which is what lets `streamed_greens` through before a propagator exists.
        if system.name == "UEG":
            self.kind = 'planewave'
        else:
            self.kind = 'hubbard_continuous' if walker_opts.get('continuous_fields', False) else 'discrete'
        if not hasattr(trial, 'dmat_inv'):
            raise NotImplementedError("thermal walkers: a OneBody trial density matrix is needed (no MeanField)")
        if walker_opts.get('low_rank', False):
            raise NotImplementedError("thermal walkers: low_rank: True is not supported")
        self.pcont_method = walker_opts.get('population_control', 'comb')
        if self.pcont_method != 'comb':
            raise NotImplementedError("thermal walkers: population control '%s' is not supported (pair_branch "
                                      "included): comb only" % self.pcont_method)
        # the Green's function with T in device memory (k_thermal_cplx.hip, AFQ_THERMAL_STREAMED_GREENS)
        self.streamed_greens = bool(walker_opts.get('streamed_greens', False))
        if self.streamed_greens and self.kind == 'discrete':
            raise NotImplementedError("thermal walkers: streamed_greens belongs to the continuous fields (Hubbard "
                                      "walkers with discrete fields fit to M = 64 as they are; with "
                                      "hubbard_stratonovich: 'continuous' the driver announces the complex walkers, and "
                                      "walkers: {continuous_fields: True} does so by hand)")
        # one complex matrix in LDS and two columns per lane (thermal_wide.h, AFQ_THERMAL_WIDE)
        self.wide_basis = bool(walker_opts.get('wide_basis', False))
        if self.wide_basis and self.kind == 'discrete':
            raise NotImplementedError("thermal walkers: wide_basis belongs to the continuous fields (Hubbard walkers "
                                      "with discrete fields work one lane per column, M <= 64; with "
                                      "hubbard_stratonovich: 'continuous' the driver announces the complex walkers, and "
                                      "walkers: {continuous_fields: True} does so by hand)")
        if self.wide_basis and self.streamed_greens:
            raise NotImplementedError("thermal walkers: wide_basis and streamed_greens are two placements of the same "
                                      "matrices: ask for one")
        # the wide route with no matrix in LDS (thermal_wide.h, AFQ_THERMAL_FAR)
        self.far_basis = bool(walker_opts.get('far_basis', False))
        if self.far_basis and self.kind == 'discrete':
            raise NotImplementedError("thermal walkers: far_basis belongs to the continuous fields (Hubbard walkers "
                                      "with discrete fields reach M = 128 with delayed_updates; with "
                                      "hubbard_stratonovich: 'continuous' the driver announces the complex walkers, and "
                                      "walkers: {continuous_fields: True} does so by hand)")
        if self.far_basis and self.wide_basis:
            raise NotImplementedError("thermal walkers: far_basis and wide_basis are two placements of the same "
                                      "matrices: ask for one")
        if self.far_basis and self.streamed_greens:
            raise NotImplementedError("thermal walkers: far_basis and streamed_greens are two placements of the same "
                                      "matrices: ask for one")
        # the far route with four columns per lane (thermal_wide.h, AFQ_THERMAL_QUAD)
        self.quad_basis = bool(walker_opts.get('quad_basis', False))
        if self.quad_basis and self.kind == 'discrete':
            raise NotImplementedError("thermal walkers: quad_basis belongs to the continuous fields (Hubbard walkers "
                                      "with discrete fields reach M = 128 with delayed_updates; with "
                                      "hubbard_stratonovich: 'continuous' the driver announces the complex walkers, and "
                                      "walkers: {continuous_fields: True} does so by hand)")
        for other in ('far_basis', 'wide_basis', 'streamed_greens'):
            if self.quad_basis and getattr(self, other):
                raise NotImplementedError("thermal walkers: quad_basis and %s are two placements of the same "
                                          "matrices: ask for one" % other)
        # the slice by delayed updates and the wide real Green's function (k_thermal.hip, AFQ_THERMAL_DELAYED)
        self.delayed_updates = bool(walker_opts.get('delayed_updates', False))
        if self.delayed_updates and self.kind != 'discrete':
            raise NotImplementedError("thermal walkers: delayed_updates belongs to the discrete fields (Hubbard walkers "
                                      "with Hirsch fields; the complex walkers have wide_basis)")
        if self.kind != 'discrete':
            self._check_bound(self.kind, system.nbasis)
        if self.delayed_updates:
            bound = MAX_BASIS['discrete', 'delayed']
            if system.nbasis > bound:
                raise NotImplementedError("thermal walkers: M = %d > %d sites is not supported with delayed_updates (the "
                                          "wide Green's function works two columns per lane, 128 in all)"
                                          % (system.nbasis, bound))
        elif system.nbasis > 64 and not self.wide_basis and not self.far_basis and not self.quad_basis:
            raise NotImplementedError("thermal walkers: M = %d > 64 sites is not supported%s" % (
                system.nbasis, " (walkers: {delayed_updates: True} reaches M = %d)" % MAX_BASIS['discrete', 'delayed']
                if self.kind == 'discrete' else ""))
        self.nwalkers = qmc.nwalkers
        self.ntot_walkers = qmc.ntot_walkers
        self.walker_type = 'thermal'
        self.write_freq = 0
        self.write_restart = False
        self.use_log_shift = False
        self.num_slices = trial.num_slices
        # walkers/thermal.py:31-43
        self.stack_size = walker_opts.get('stack_size', None)
        if self.stack_size is None:
            self.stack_size = trial.stack_size
        if (self.num_slices // self.stack_size) * self.stack_size != self.num_slices:
            self.stack_size = update_stack(self.stack_size, self.num_slices)
        self.stack_length = self.num_slices // self.stack_size
        # walkers/handler.py:86-100: the stabilisation period against the stack size
        if self.stack_size % qmc.nstblz != 0 or qmc.nstblz < self.stack_size:
            if qmc.nstblz < self.stack_size:
                qmc.nstblz = self.stack_size
            else:
                qmc.nstblz = update_stack(qmc.nstblz, self.stack_size)
        self.nstblz = qmc.nstblz
        self.dt = qmc.dt
        self.ctx = get_context(system, trial, device_id)
        self.dev = self.ctx.dev
        self.system, self.trial = system, trial
        self.dev.walkers_alloc(self.nwalkers)
        self.nw = self.nwalkers
        self.target_weight = qmc.ntot_walkers
        self.total_weight = float(qmc.ntot_walkers)
        self.time_slice = 0
        self.path_index = 0
        self.configured = None      # (kind, key) the library is configured with; the key is what its configuration depends on
        self._prop = None
        self.last_parent_ix = None
        self.walkers = [ThermalWalkerView(self, i) for i in range(self.nw)]

    @property
    def continuous(self):
        """The UEG's walkers: complex with a diagonal trial."""
        return self.kind == 'planewave'

    @property
    def dense(self):
        """The library holds complex walkers with a dense trial (Hubbard with continuous fields)."""
        return self.configured is not None and self.configured[0] == 'hubbard_continuous'

    def ensure_configured(self, prop=None):
        """The library is configured on first use, by the kind's entry point with the propagator's constants; without a
        propagator yet (a walker's G read first) with the ones the kind's propagator would compute.  A propagator whose
        key differs from what was configured configures the library again: allowed only at time slice 0, and it starts
        the population afresh (bins, G, weights, and for the complex walkers right and M0 = the trial's; anything set on
        the walkers before is lost).  Complex walkers never go back to a discrete propagator."""
        if self.configured is not None and prop is None:
            return
        kind = self.kind
        if self.system.name == "Hubbard":
            hs_type = getattr(prop, 'hs_type', None)
            if self.dense and hs_type != 'continuous':
                raise RuntimeError("thermal walkers: the population carries complex walkers (continuous fields); a '%s' "
                                   "propagator cannot move it" % hs_type)
            if prop is not None:
                kind = 'hubbard_continuous' if hs_type == 'continuous' else 'discrete'
        key, configure = getattr(self, '_configure_' + kind)(prop)
        if self.configured == (kind, key):
            return
        if self.configured is not None and self.time_slice != 0:
            raise RuntimeError("thermal walkers: %s changed in the middle of a path"
                               % _CHANGED[kind if self.configured[0] == kind else None])
        if self.delayed_updates and kind != 'discrete':
            raise NotImplementedError("thermal walkers: delayed_updates belongs to the discrete fields (a '%s' "
                                      "propagator moves complex walkers)" % getattr(prop, 'hs_type', kind))
        configure(L.THERMAL_QUAD if self.quad_basis else L.THERMAL_FAR if self.far_basis else L.THERMAL_WIDE if self.wide_basis
                  else L.THERMAL_STREAMED_GREENS if self.streamed_greens
                  else L.THERMAL_DELAYED if self.delayed_updates else 0)
        self.kind, self.configured = kind, (kind, key)

    def _configure_discrete(self, prop):
        """Key: the propagator's stabilisation period, which decides when the Green's function is refreshed."""
        if self.streamed_greens:
            raise NotImplementedError("thermal walkers: streamed_greens belongs to the continuous fields (Hubbard "
                                      "walkers with discrete fields fit to M = 64 as they are)")
        if self.wide_basis:
            raise NotImplementedError("thermal walkers: wide_basis belongs to the continuous fields (Hubbard walkers "
                                      "with discrete fields work one lane per column, M <= 64)")
        if self.far_basis:
            raise NotImplementedError("thermal walkers: far_basis belongs to the continuous fields (Hubbard walkers "
                                      "with discrete fields reach M = 128 with delayed_updates)")
        if self.quad_basis:
            raise NotImplementedError("thermal walkers: quad_basis belongs to the continuous fields (Hubbard walkers "
                                      "with discrete fields reach M = 128 with delayed_updates)")
        nstblz = self.nstblz if prop is None else prop.nstblz

        def configure(options):
            _, auxf, _, _, BH1 = thermal_constants(self.system, self.trial, self.dt)
            self.dev.thermal_configure(self.num_slices, self.stack_size, nstblz, self.trial.dmat, self.trial.dmat_inv,
                                       BH1, auxf, options)
            self.nstblz = nstblz
        return nstblz, configure

    def _configure_planewave(self, prop):
        """Key: fb_bound.  BH1 and mf_shift are the propagator's, or what it would compute."""
        fb_bound = 1.0 if prop is None else prop.fb_bound

        def configure(options):
            BH1, mf_shift = (prop.BH1, prop.mf_shift) if prop is not None else planewave_constants(
                self.system, self.trial, self.dt)
            self.dev.thermal_configure_continuous(self.num_slices, self.stack_size, self.dt, self.trial.dmat,
                                                  self.trial.dmat_inv, BH1, mf_shift, fb_bound, options)
        return fb_bound, configure

    def _configure_hubbard_continuous(self, prop):
        """No key: BH1, mf_shift and mf_const_fac are what ``Continuous`` computes from the system and the trial, which
        is all they depend on."""
        def configure(options):
            p = prop or thermal_continuous.Continuous({}, _QmcOf(self.dt, self.nstblz), self.system, self.trial)
            self._check_bound('hubbard_continuous', self.system.nbasis)
            self.dev.thermal_configure_hubbard_continuous(self.num_slices, self.stack_size, self.dt, self.trial.dmat,
                                                          self.trial.dmat_inv, p.BH1, p.mf_shift, p.mf_const_fac, options)
        return (), configure

    def _check_bound(self, kind, M):
        who, unit, slice_keeps = _BOUND_WORDS[kind]
        if self.wide_basis:
            bound = MAX_BASIS[kind, 'wide']
            if M > bound:
                raise NotImplementedError("%s: M = %d > %d %s is not supported with wide_basis (the wide Green's function "
                                          "keeps one complex matrix of 16 M (M | 1) bytes and 18,944 bytes of vectors in the "
                                          "160 KiB of LDS)" % (who, M, bound, unit))
            return
        if getattr(self, 'far_basis', False):
            bound = MAX_BASIS[kind, 'far']
            if M > bound:
                raise NotImplementedError("%s: M = %d > %d %s is not supported with far_basis (the far Green's function "
                                          "keeps no matrix in LDS; a lane owns two columns, 128 in all)"
                                          % (who, M, bound, unit))
            return
        if getattr(self, 'quad_basis', False):
            bound = MAX_BASIS[kind, 'quad']
            if M > bound:
                raise NotImplementedError("%s: M = %d > %d %s is not supported with quad_basis (the quad Green's function "
                                          "keeps no matrix in LDS; a lane owns four columns, 256 in all)"
                                          % (who, M, bound, unit))
            return
        bound = MAX_BASIS[kind, self.streamed_greens]
        if M > bound:
            raise NotImplementedError("%s: M = %d > %d %s is not supported%s" % (
                who, M, bound, unit, " with streamed_greens (the slice kernel keeps %s in LDS)" % slice_keeps
                if self.streamed_greens else " (the complex Green's function keeps a walker's working set in LDS; "
                "walkers: {streamed_greens: True} reaches M = %d)" % MAX_BASIS[kind, True]))

    def set_total_weight(self, total_weight):
        self.total_weight = total_weight

    def recompute_greens_function(self, trial, time_slice=None):
        self.ensure_configured()
        self.dev.thermal_greens(self.time_slice if time_slice is None else time_slice)

    def pop_control(self, comm=None):
        """walkers/handler.py:225-338 on one rank: the comb, G and the stack travel with the clones."""
        if self.ntot_walkers == 1:
            return
        self.ensure_configured()
        r = numpy.random.random()
        try:
            pix, total = self.dev.popcontrol_comb(r, self.target_weight)
        except L.AfqError as e:
            if e.code == L.AFQ_EWEIGHT:
                raise SystemExit("# Warning: total weight is below 1e-8.  Something is seriously wrong.")
            raise
        self.last_parent_ix = pix
        self.set_total_weight(total)

    def cap_weights(self, frac=0.10):
        """qmc/thermal_afqmc.py:220-221 for every walker: |w| > frac total_weight -> frac total_weight."""
        self.dev.cap_weights(frac, self.total_weight)

    def reset(self, trial):
        """walkers/handler.py:424-430."""
        self.ensure_configured()
        self.dev.thermal_reset()
        self.time_slice = 0
        self.path_index += 1
