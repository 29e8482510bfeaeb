"""The back-propagated pairing correlations over two ranks of the real driver on one GPU: the harness and the UEG set-up
of test_gpu_ueg_sf_multirank.py (two processes, gloo process group, the same auxiliary fields as one rank with twice the
walkers; the kernel does not depend on the system, the bond table is any table).  The [nb, nb, M, M] sums ride in the
estimator's vector through comm.Reduce; every window must be the single-rank one of the union population, to 1e-8."""
import os

import numpy
import pytest
import torch.multiprocessing as mp

from tests import pair_ref
from tests import test_gpu_multirank as mr
from tests import test_gpu_ueg_sf_multirank as sfm

pytestmark = pytest.mark.gpu
NW, NSTEPS, NBLOCKS = sfm.NW, sfm.NSTEPS, sfm.NBLOCKS
NB = 3


def drive(comm, nw_total, first, count):
    from pauxy_amd.qmc.afqmc import AFQMC
    s, t = sfm.build()
    feed = sfm.Feed(s.nfields, first, count)
    numpy.random.normal, numpy.random.random = feed.normal, feed.random
    options = {'qmc': {'timestep': 0.01, 'num_steps': NSTEPS, 'blocks': NBLOCKS, 'stabilise_freq': 5,
                       'pop_control_freq': 5, 'num_walkers': nw_total},
               'propagator': {'device_rng': False},
               'estimators': {'mixed': {'energy_eval_freq': 2, 'verbose': False},
                              'back_propagated': {'tau_bp': 0.04, 'one_rdm': True, 'evaluate_energy': True,
                                                  'two_rdm': 'pairing',
                                                  'pairing_bonds': pair_ref.random_table(NB, s.nbasis, 12)}}}
    afqmc = AFQMC(comm=comm, options=options, system=s, trial=t)
    w0 = numpy.exp(0.9 * numpy.random.RandomState(5).normal(size=2 * NW))[first:first + count]
    for i, w in enumerate(afqmc.psi.walkers):
        w.weight = w0[i]
    pix = []

    def on_step(step, psi):
        if step % 5 == 0:
            pix.append(numpy.array(psi.last_parent_ix).copy())
    afqmc.run_batched(on_step=on_step, fetch_popcontrol=True)
    root = comm is None or comm.rank == 0
    bp = afqmc.estimators.estimators['back_prop']
    out = dict(pix=numpy.array(pix), phi=numpy.array([w.phi for w in afqmc.psi.walkers]))
    if root:
        out.update(bp_two=numpy.array(bp.two_rdm), bp_one=numpy.array(bp.one_rdm), bp_E=numpy.array(bp.energies),
                   bp_den=numpy.array(bp.denominator))
    return out


def _worker(rank, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK='0')
        import torch
        import torch.distributed as dist
        from pauxy_amd.comm import TorchComm
        dist.init_process_group('gloo', rank=rank, world_size=2)
        comm = TorchComm(device=torch.device('cpu'))
        q.put((rank, drive(comm, 2 * NW, rank * NW, NW)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        q.put((rank, repr(e)))
        raise


def test_two_ranks_give_the_pairing_correlations_of_one_rank():
    import numpy.random as npr
    keep = npr.normal, npr.random
    try:
        one = drive(None, 2 * NW, 0, 2 * NW)
    finally:
        npr.normal, npr.random = keep
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = mr.free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in procs], key=lambda x: x[0])
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    for rank, out in res:
        assert isinstance(out, dict), (rank, out)
    a, b = res[0][1], res[1][1]
    assert numpy.array_equal(a['pix'], one['pix']) and numpy.array_equal(b['pix'], one['pix'])
    sfm.close(numpy.concatenate([a['phi'], b['phi']]), one['phi'])
    assert 'bp_two' not in b
    M = one['phi'].shape[1]
    assert one['bp_two'].shape == ((NSTEPS * NBLOCKS) // 4, NB, NB, M, M)
    for k in ('bp_den', 'bp_one', 'bp_two', 'bp_E'):
        print("PAIR-RANKS | %s | two ranks vs one: %.2e" % (
            k, numpy.max(numpy.abs(a[k] - one[k])) / max(1.0, numpy.max(numpy.abs(one[k])))))
        sfm.close(a[k], one[k])
    # the windows hold what they should: where the table has no partner the sums are exactly zero
    nbr = pair_ref.random_table(NB, M, 12)
    gone = (nbr < 0)[:, None, :, None] | (nbr < 0)[None, :, None, :]
    for two in one['bp_two']:
        assert not numpy.any(two[gone]) and numpy.max(numpy.abs(two[~gone])) > 1e-3
