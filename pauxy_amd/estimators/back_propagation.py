"""Back-propagated estimator on the device, behind PAUXY's ``BackPropagation`` surface.

Mirrors pauxy/estimators/back_propagation.py:63-326 for RHF/UHF-type single-determinant
trials on a Generic, UEG or (discrete-field) Hubbard system, and for multi-determinant (NOMSD) trials on a Generic
system (``afq_bp_update_msd``: every determinant back-propagated, weighted by conj(c_d), its overlap with the walker at
the window's start and the norms its re-orthogonalisations took out; the reference itself fails on ``ndets > 1``, and
``two_rdm`` / ``evaluate_ekt`` are refused with it): same constructor signature and attributes (``tau_bp``,
``nmax``, ``splits``, ``calc_one_rdm``, ``restore_weights``, ``init_walker``), same
``update`` / ``print_step`` / ``zero`` methods.  The field history (walkers/stack.py
FieldConfig), ``phi_old`` and the back-propagation itself live on the device
(``afq_bp_configure`` / ``afq_bp_update``); one call handles the whole population.

Output: the per-window results are appended to ``self.one_rdm`` / ``self.denominator`` /
``self.energies`` (lists; ``rdm()`` returns their ratio like pauxy.analysis.extraction.extract_rdm)
and, when the container was given a file name, pushed by the root rank to the reference's
groups ``back_propagated/{denominator,energies,one_rdm}_<n>/<block>`` (back_propagation.py:288-324).

``two_rdm: True`` (the full spin-summed two-body RDM, back_propagation.py:168-175) and ``evaluate_ekt: True`` (the EKT
Fock matrices of estimators/ekt.py) add the lists ``self.two_rdm`` / ``self.fock_1p`` / ``self.fock_1h`` and the groups
``two_rdm_<n>`` / ``fock_1p_<n>`` / ``fock_1h_<n>``; the flat ``estimates`` vector and its slicing are the reference's,
including the Fock matrices' offset with ``one_rdm: False``.  These attributes exist only when the option is set.
EKT on a Generic system uses L_x[i, k] = hs_pot[i*M + k, x] (the reference's ekt.py asserts a 3-D array and fails on
the [M*M, K] vectors of a Generic system); it is refused for the Hubbard model and for complex Generic vectors.

``evaluate_energy: True`` works on all three systems: the full-G Cholesky energy (Generic), local_energy_hubbard
(Hubbard) and local_energy_ueg (UEG) of every walker's G_bp.  (The reference's own call passes the dispatcher an
``opt`` keyword it does not have and raises TypeError; the numbers are those of the call without it.)
``two_rdm: 'structure_factor'`` (UEG only; NotImplementedError for systems without momentum transfers) accumulates
sum_w weight_w two_rdm[G_bp[w]] with the [2, 2, nq] array local_energy_ueg(system, G, two_rdm=...) fills, in the
reference's flat layout (``two_rdm_shape = (2, 2, nq)``), complex and not normalised: ``self.two_rdm`` and the group
``two_rdm_<n>``.  The sums run over the system's index lists: ``UEG(..., full_lists=True)`` gives the complete pair
sums of a back-propagated Green's function, the default lists (the reference's: first nup plane waves) truncated ones.
One deliberate difference: the structure factor is evaluated whenever it is asked for, also with ``evaluate_energy:
False``; the reference fills the array only inside its energy call and would accumulate zeros there.

``two_rdm: 'correlation'`` (Generic, UEG and Hubbard systems, single-determinant trials; not in the reference's
estimator, whose analysis/correlation.py still reads such a dataset) accumulates sum_w weight_w corr[G_bp[w]] with the
[5, M, M] array of ``afq_correlations_full_g``: <n_is n_jt> in the slices 2s+t and <S+_i S-_j> in slice 4
(``two_rdm_shape = (5, M, M)``), complex and not normalised like the structure factor, in the same slot of the flat
vector, ``self.two_rdm`` and the group ``two_rdm_<n>``.  It is evaluated with or without ``evaluate_energy`` and
together with ``evaluate_ekt``.  estimators/correlation.py turns the normalised array into charge and spin correlations.

``two_rdm: 'pairing'`` (the same systems and trials; not in the reference either) accumulates sum_w weight_w
pair[G_bp[w]] with the [nb, nb, M, M] array of ``afq_pairing_full_g`` over the bond table ``pairing_bonds`` (an integer
array [nb, M]: the partner site of every site along every bond, -1 where there is none; nb <= 16).  A Hubbard system
takes ``estimators.pairing.lattice_bonds(nx, ny)`` (on-site, +x, -x, +y, -y) when none is given; any other system
without ``pairing_bonds`` is a ValueError.  ``two_rdm_shape = (nb, nb, M, M)``, complex and not normalised, in the same
slot of the flat vector, ``self.two_rdm`` and the group ``two_rdm_<n>``; evaluated with or without ``evaluate_energy``
and together with ``evaluate_ekt``.  The back-propagated Green's function is the transpose of <c+_i c_j>, so the stored
element [b, b', i, j] is <D+(j, j_b') D(i, i_b)> with D+(k, l) = c+_k,up c+_l,down (pair[b', b, j, i] of the header's
definition).  estimators/pairing.py forms the singlet pair fields and the s, extended-s and d-wave channels from it.
"""
import numpy


class BackPropagation(object):
    structure_factor = False
    correlation = False
    pairing = False

    def __init__(self, bp, root, filename, qmc, system, trial, dtype, BT2):
        self.tau_bp = bp.get('tau_bp', 0)
        self.nmax = int(self.tau_bp / qmc.dt)
        self.header = ['E', 'E1b', 'E2b']
        self.calc_one_rdm = bp.get('one_rdm', True)
        self.calc_two_rdm = bp.get('two_rdm', None)
        self.init_walker = bp.get('init_walker', False)
        self.nsplit = bp.get('nsplit', 1)
        self.splits = numpy.array([(i + 1) * (self.nmax // self.nsplit) for i in range(self.nsplit)])
        self.nreg = len(self.header)
        self.accumulated = False
        self.eval_energy = bp.get('evaluate_energy', False)
        self.eval_ekt = bp.get('evaluate_ekt', False)
        self.restore_weights = bp.get('restore_weights', None)
        ndets = int(getattr(trial, 'ndets', 1))           # (not kept: the attributes are the reference's)
        if system.name not in ("Generic", "UEG", "Hubbard") or (ndets != 1 and system.name != "Generic"):
            raise NotImplementedError("device back-propagation: Generic, UEG or Hubbard system; multi-determinant "
                                      "trials on Generic systems")
        if ndets != 1 and (self.calc_two_rdm is not None or self.eval_ekt):
            # sum_d w_d f[G_d] of forms quartic / cubic in G_d: not the one-body sums of afq_bp_update_msd
            raise NotImplementedError("back-propagated two_rdm / evaluate_ekt with a multi-determinant trial")
        if system.name == "Hubbard" and self.restore_weights is not None:
            # back_propagation.py:117-125: the Hubbard variant back-propagates the DISCRETE fields, which are recorded
            # without weight factors (hubbard.py:215-216, walkers/stack.py:35-49); afq_bp_configure refuses the
            # continuous Hubbard propagator
            raise NotImplementedError("restore_weights with the discrete Hubbard fields")
        if isinstance(self.calc_two_rdm, str):
            if self.calc_two_rdm not in ("structure_factor", "correlation", "pairing"):
                raise ValueError("two_rdm: True, 'structure_factor', 'correlation' or 'pairing'")
            # (instance attributes only with the option, like two_rdm)
            if self.calc_two_rdm == "structure_factor":
                self.structure_factor = True
            elif self.calc_two_rdm == "correlation":
                self.correlation = True
            else:
                self.pairing = True
        if self.pairing:
            bonds = bp.get('pairing_bonds', None)
            if bonds is None:
                if system.name != "Hubbard":
                    raise ValueError("two_rdm: 'pairing' needs pairing_bonds [nb, M] on a %s system" % system.name)
                from pauxy_amd.estimators.pairing import lattice_bonds
                bonds = lattice_bonds(system.nx, system.ny)[0]
            bonds = numpy.asarray(bonds)
            if (bonds.ndim != 2 or bonds.shape[1] != system.nbasis or not 1 <= bonds.shape[0] <= 16
                    or bonds.dtype.kind not in 'iu' or bonds.min() < -1 or bonds.max() >= system.nbasis):
                raise ValueError("pairing_bonds: an integer array [nb, M], 1 <= nb <= 16, entries in [-1, M)")
            self.pairing_bonds = bonds.astype(numpy.int32)
        if self.structure_factor and system.name != "UEG":
            # S(q) is a sum over momentum transfers: back_propagation.py:88-89 reads system.qvecs
            raise NotImplementedError("back-propagated two_rdm: 'structure_factor' needs a UEG system")
        if self.eval_ekt and system.name == "Hubbard":
            raise NotImplementedError("EKT: the Hubbard model has no Cholesky vectors")
        if (self.eval_ekt and system.name == "Generic" and numpy.iscomplexobj(system.hs_pot)
                and numpy.any(numpy.asarray(system.hs_pot).imag != 0)):
            raise NotImplementedError("EKT with complex Cholesky vectors (ekt.py's 4-fold-symmetry formula)")
        if (system.name == "Generic" and numpy.iscomplexobj(system.hs_pot)
                and numpy.any(numpy.asarray(system.hs_pot).imag != 0)):
            # the backward step applies B(-conj(x)) with the same L_n: B(x)^H only when every L_n is Hermitian
            M = system.nbasis
            L3 = numpy.asarray(system.hs_pot).reshape(M, M, -1)
            if not numpy.array_equal(L3, L3.conj().transpose(1, 0, 2)):
                raise NotImplementedError("back-propagation with non-Hermitian complex Cholesky vectors")
        if self.nmax < 1:
            raise ValueError("tau_bp shorter than one time step")
        M = system.nbasis
        self.G = numpy.zeros((2, M, M), dtype=numpy.complex128)
        self.nstblz = qmc.nstblz
        self.BT2 = BT2
        self.dt = qmc.dt
        dms_size = self.G.size
        if self.calc_two_rdm is not None:         # back_propagation.py:86-99,100-104: the flat layout of the reference
            self.two_rdm = []
            # back_propagation.py:88-94
            self.two_rdm_shape = ((2, 2, len(system.qvecs)) if self.structure_factor
                                  else (5, M, M) if self.correlation
                                  else (len(self.pairing_bonds),) * 2 + (M, M) if self.pairing else (M,) * 4)
            self.two_rdm_size = int(numpy.prod(self.two_rdm_shape))
            dms_size += self.two_rdm_size
        if self.eval_ekt:
            self.fock_1p = []
            self.fock_1h = []
            dms_size += 2 * M * M
        self.estimates = numpy.zeros(self.nreg + 1 + dms_size, dtype=dtype)
        self.global_estimates = numpy.zeros(self.nreg + 1 + dms_size, dtype=dtype)
        self.key = {'ETotal': "BP estimate for total energy.", 'E1B': "BP estimate for one-body energy.",
                    'E2B': "BP estimate for two-body energy."}
        self.root = root
        self.one_rdm = []
        self.denominator = []
        self.energies = []
        self.split_of = []                     # path length (buff_ix) of every stored window
        self.buff_ix = 0
        self._nsteps_seen = 0
        self.flush_every = bp.get('flush_every', None)
        self.output = None
        if root and filename is not None:
            self.setup_output(filename)

    def update(self, system, qmc, trial, psi, step, free_projection=False):
        """back_propagation.py:127-226 (update_uhf).  ``psi.walkers[0].field_configs.step`` of the
        reference is the device's per-walker step counter; walker 0 decides, as in the reference."""
        psi._end_sweep()
        psi._flush()
        dev = psi.dev
        buff_ix = int(dev.bp_steps()[0])
        if buff_ix not in self.splits:
            return
        if getattr(trial, 'ndets', 1) != 1 and not self.init_walker:
            # |psi_T> = sum_d c_d |D_d>: every determinant is back-propagated, weighted by conj(c_d) and its overlap
            # with the walker at the window's start, norms of the re-orthogonalisations included (afq_bp_update_msd)
            energies, denom, G, _ = dev.bp_update_msd(numpy.asarray(trial.psi), numpy.asarray(trial.coeffs), self.nstblz,
                                                      self.restore_weights, self.eval_energy,
                                                      reset=bool(buff_ix == self.splits[-1]))
            self.estimates[:self.nreg] += energies
            self.estimates[self.nreg] += denom
            self.estimates[self.nreg + 1:self.nreg + 1 + G.size] += G.ravel()
            psi._greens_version = -1
            self.accumulated = True
            self.buff_ix = buff_ix
            return
        phi0 = numpy.asarray(trial.init if self.init_walker else trial.psi, dtype=numpy.complex128)
        if phi0.ndim == 3:
            phi0 = phi0[0]
        two, ekt = self.calc_two_rdm is not None, bool(self.eval_ekt)
        if (two or ekt) and getattr(self, '_obs_dev', None) is not dev:
            self._setup_observables(dev, system)
        extra = {'two_rdm': two, 'ekt': ekt} if (two or ekt) else {}
        res = dev.bp_update(phi0, self.nstblz, self.restore_weights, self.eval_energy,
                            reset=bool(buff_ix == self.splits[-1]), **extra)     # back_propagation.py:219-222
        energies, denom, G = res[:3]
        self.estimates[:self.nreg] += energies
        self.estimates[self.nreg] += denom
        end = self.nreg + 1 + G.size
        self.estimates[self.nreg + 1:end] += G.ravel()
        if two:                                    # back_propagation.py:199-206
            self.estimates[end:end + self.two_rdm_size] += res[3]['two_rdm'].ravel()
            end += self.two_rdm_size
        if ekt:
            m2 = self.G[0].size
            self.estimates[end:end + m2] += res[3]['fock_1p'].ravel()
            self.estimates[end + m2:end + 2 * m2] += res[3]['fock_1h'].ravel()
        psi._greens_version = -1
        self.accumulated = True
        self.buff_ix = buff_ix

    def print_step(self, comm, nprocs, step, nsteps=1, free_projection=False):
        """back_propagation.py:269-316."""
        if not self.accumulated:
            return
        comm.Reduce(self.estimates, self.global_estimates, op=None)
        if comm.rank == 0:
            weight = self.global_estimates[self.nreg]
            self.denominator.append(numpy.array(weight))
            self.split_of.append(int(self.buff_ix))
            out = self.output
            if out is not None:
                out.push(numpy.array([weight]), 'denominator_%d' % self.buff_ix)
            if self.eval_energy:                        # back_propagation.py:291-297
                e = self.global_estimates[:self.nreg]
                self.energies.append(e.copy() if free_projection else e / weight)
                if out is not None:
                    out.push(self.energies[-1], 'energies_%d' % self.buff_ix)
            if self.calc_one_rdm:
                start = self.nreg + 1
                self.one_rdm.append(self.global_estimates[start:start + self.G.size].reshape(self.G.shape).copy())
                if out is not None:
                    out.push(self.one_rdm[-1], 'one_rdm_%d' % self.buff_ix)
            if self.calc_two_rdm:                      # back_propagation.py:304-308
                start = self.nreg + 1 + self.G.size
                self.two_rdm.append(self.global_estimates[start:start + self.two_rdm_size]
                                    .reshape(self.two_rdm_shape).copy())
                if out is not None:
                    out.push(self.two_rdm[-1], 'two_rdm_%d' % self.buff_ix)
            if self.eval_ekt:
                # back_propagation.py:310-324, slicing included: the offset skips the one-body RDM only when it is
                # output, so that with one_rdm: False the Fock matrices are read from its region, as there
                start = self.nreg + 1
                if self.calc_one_rdm:
                    start += self.G.size
                if self.calc_two_rdm:
                    start += self.two_rdm_size
                m2 = self.G[0].size
                shape = self.G[0].shape
                self.fock_1p.append(self.global_estimates[start:start + m2].reshape(shape).copy())
                self.fock_1h.append(self.global_estimates[start + m2:start + 2 * m2].reshape(shape).copy())
                if out is not None:
                    out.push(self.fock_1p[-1], 'fock_1p_%d' % self.buff_ix)
                    out.push(self.fock_1h[-1], 'fock_1h_%d' % self.buff_ix)
            if out is not None and self.buff_ix == self.splits[-1]:
                out.increment()
        self.accumulated = False
        self.zero()

    def _setup_observables(self, dev, system):
        """afq_bp_observables: the EKT's h1 = system.H1[0] and vectors (back_propagation.py:177-186)."""
        h1 = L = None
        if self.eval_ekt:
            h1 = numpy.asarray(system.H1[0])
            if system.name == "UEG":
                cv = system.chol_vecs
                cv = cv.toarray() if hasattr(cv, 'toarray') else numpy.asarray(cv)
                L = 2.0 * cv.T.reshape((system.nchol, system.nbasis, system.nbasis))
        two = ('structure_factor' if self.structure_factor else 'correlation' if self.correlation
               else 'pairing' if self.pairing else self.calc_two_rdm is not None)
        if self.pairing:
            dev.set_pairing_bonds(self.pairing_bonds)
        dev.bp_observables(two_rdm=two, ekt=bool(self.eval_ekt), h1=h1, L=L)
        self._obs_dev = dev

    def rdm(self):
        """one_rdm / denominator per window (analysis/extraction.py:36-62)."""
        return numpy.array(self.one_rdm) / numpy.array(self.denominator)[:, None, None, None]

    def zero(self):
        self.estimates[:] = 0
        self.global_estimates[:] = 0

    def setup_output(self, filename):
        """back_propagation.py:333-338."""
        from pauxy_amd.estimators.utils import H5EstimatorHelper
        from pauxy_amd.utils import io as _io
        if self.eval_energy:
            with _io.h5.File(filename, 'a') as fh5:
                fh5['back_propagated/headers'] = numpy.array(self.header).astype('S')
        self.output = H5EstimatorHelper(filename, 'back_propagated', flush_every=self.flush_every)
