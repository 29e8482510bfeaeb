"""Imaginary-time single-particle Green's function (ITCF) on the device, behind PAUXY's ``ITCF`` surface.

Follows the constructor and attributes of pauxy/estimators/itcf.py:78-155 (``nmax``, ``ntau``, ``neqlb``,
``nprop_tot``, ``spgf``, ``spgf_shape``, ``denom``, ``update``, ``print_step``, ``zero``) for single-determinant
trials on a Generic system or a Hubbard model with discrete fields.  Every ``nprop_tot`` steps one window runs on the
device (``afq_itcf_configure`` / ``afq_itcf_update``, k_itcf.hip) for the whole population; what it computes is
written down in DESIGN.md (row 8f-3) and restated in numpy in tests/itcf_ref.py.  The reference's own ITCF code cannot
run (it reads walker attributes that no longer exist) and pairs the wrong slices in its stable loop; this estimator
follows the specification, not that code.

Output: spgf / denom of every window, pushed by the root rank to ``single_particle_greens_function/real_space/<block>``:
``mode: 'full'`` [nmax + 1, 2, 2, M, M], ``'diagonal'`` [nmax + 1, 2, 2, M], a list of (i, j) pairs
[nmax + 1, 2, 2, len(list)].  The windows are also kept in ``self.windows``; ``extract_itcf`` reads the file back.
"""
import numpy


def _hermitian(L3):
    return numpy.array_equal(L3, L3.conj().transpose(1, 0, 2))


class ITCF(object):
    def __init__(self, itcf, qmc, trial, root, h5f, system, dtype, BT2, discrete=None, free_projection=False):
        self.stable = itcf.get('stable', True)
        self.restore_weights = itcf.get('restore_weights', True)
        self.tmax = itcf.get('tau_max', 0.0)
        self.teqlb = itcf.get('tau_eqlb', 0.0)
        self.mode = itcf.get('mode', 'full')
        self.stack_size = itcf.get('stack_size', 1)
        self.kspace = itcf.get('kspace', False)
        self.nmax = int(self.tmax / qmc.dt)
        self.dt = qmc.dt
        self.ntau = int(self.nmax / self.stack_size)
        self.neqlb = int(self.teqlb / qmc.dt)
        self.nprop_tot = self.nmax + self.neqlb
        self.nstblz = qmc.nstblz
        self.denom = 0
        self.BT2 = BT2
        if system.name == "UEG":
            raise NotImplementedError("itcf: the reference has no propagator matrix for the UEG")
        if system.name == "Hubbard" and discrete is False:
            raise NotImplementedError("itcf: continuous Hubbard fields (the reference builds B from discrete fields only)")
        if system.name not in ("Generic", "Hubbard"):
            raise NotImplementedError("itcf: Generic or Hubbard systems only")
        if free_projection:
            raise NotImplementedError("itcf: free projection (no field history is recorded)")
        if getattr(trial, 'ndets', 1) != 1:
            raise NotImplementedError("itcf: multi-determinant trials")
        if system.name == "Generic" and numpy.iscomplexobj(system.hs_pot) and numpy.any(numpy.asarray(system.hs_pot).imag != 0):
            M = system.nbasis
            if not _hermitian(numpy.asarray(system.hs_pot).reshape(M, M, -1)):
                # psi_L is back-propagated with B(-conj(x)), which is B(x)^H only for Hermitian L_n
                raise NotImplementedError("itcf: non-Hermitian complex Cholesky vectors")
        if system.name == "Hubbard" and self.restore_weights:
            raise NotImplementedError("itcf: restore_weights with the discrete Hubbard fields (no weight factors are recorded)")
        if self.kspace:
            raise NotImplementedError("itcf: kspace (the reference writes nothing for it)")
        if self.stack_size != 1:
            raise NotImplementedError("itcf: stack_size != 1")
        if system.nbasis > 128:
            raise NotImplementedError("itcf: more than 128 basis functions (the batched inverse of B)")
        if self.nmax < 1:
            raise ValueError("itcf: tau_max shorter than one time step")
        if not (self.mode in ('full', 'diagonal') or isinstance(self.mode, (list, tuple))):
            raise ValueError("itcf: mode is 'full', 'diagonal' or a list of (i, j) pairs")
        M = system.nbasis
        self.spgf_shape = (self.ntau + 1, 2, 2, M, M)
        self.spgf = numpy.zeros(self.spgf_shape, dtype=numpy.complex128)
        self.keys = [['up', 'down'], ['greater', 'lesser']]
        self.root = root
        self.windows = []
        self.flush_every = itcf.get('flush_every', None)
        self.output = None
        self._dev = None
        self.accumulated = False
        if root and h5f is not None:
            self.setup_output(h5f)

    def written(self, spgf):
        """The part of spgf [.., 2, 2, M, M] that ``mode`` writes."""
        if self.mode == 'full':
            return spgf
        if self.mode == 'diagonal':
            return numpy.diagonal(spgf, axis1=-2, axis2=-1).copy()
        ij = numpy.array(self.mode, dtype=int).reshape(-1, 2)
        return spgf[..., ij[:, 0], ij[:, 1]]

    def update(self, system, qmc, trial, psi, step, free_projection=False):
        """One window at every step != 0 with step % nprop_tot == 0 (itcf.py:157-178, print_step:538)."""
        if step == 0 or step % self.nprop_tot != 0:
            return
        psi._end_sweep()
        psi._flush()
        dev = psi.dev
        if self._dev is not dev:
            dev.itcf_configure(self.nmax, self.neqlb, self.stable, self.restore_weights)
            self._dev = dev
        psi_T = numpy.asarray(trial.psi, dtype=numpy.complex128)
        if psi_T.ndim == 3:
            psi_T = psi_T[0]
        spgf, denom = dev.itcf_update(psi_T, self.nstblz)
        self.spgf += spgf
        self.denom += denom
        psi._greens_version = -1
        self.accumulated = True

    def print_step(self, comm, nprocs, step, nsteps=None, free_projection=False):
        """itcf.py:524-558: sums over the ranks, spgf / denom to the file."""
        if not self.accumulated:
            return
        send = numpy.concatenate([numpy.array([self.denom], dtype=numpy.complex128), self.spgf.ravel()])
        recv = numpy.zeros_like(send)
        comm.Reduce(send, recv, op=None)
        if comm.rank == 0:
            denom = recv[0]
            itcf = recv[1:].reshape(self.spgf_shape) / denom
            self.windows.append(itcf)
            if self.output is not None:
                self.output.push(self.written(itcf), 'real_space')
                self.output.increment()
        self.accumulated = False
        self.zero()

    def zero(self):
        self.spgf[:] = 0
        self.denom = 0

    def setup_output(self, filename):
        from pauxy_amd.estimators.utils import H5EstimatorHelper
        self.output = H5EstimatorHelper(filename, 'single_particle_greens_function', flush_every=self.flush_every)
