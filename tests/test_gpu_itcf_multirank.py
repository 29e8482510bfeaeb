"""The ITCF estimator over two ranks of the real driver on one GPU (the harness of test_gpu_multirank.py: two processes,
gloo process group, the same auxiliary fields as one rank with twice the walkers).  Windows of 4 steps close between the
combs (every 5 steps), so walkers cloned across the rank boundary carry their field history, phi_old and weight factors
into windows that are still open; the ranks' sums [denom, spgf] are reduced and rank 0 divides.  The result must be the
single-rank one."""
import os

import numpy
import pytest
import torch.multiprocessing as mp

from tests import test_gpu_multirank as mr

pytestmark = pytest.mark.gpu
ITCF = {'tau_max': 0.0305, 'tau_eqlb': 0.0105}          # nmax 3, neqlb 1: nprop_tot 4


def drive(comm, nw_total, first, count):
    from pauxy_amd.estimators import itcf as itcf_mod
    got = []
    base_options = mr.options

    def options(nw, walkers=None):
        o = base_options(nw, walkers)
        o['estimators']['itcf'] = dict(ITCF)
        return o
    print_step = itcf_mod.ITCF.print_step

    def capture(self, comm_, nprocs, step, *a, **k):
        had = self.accumulated
        print_step(self, comm_, nprocs, step, *a, **k)
        if had and (comm_ is None or comm_.rank == 0):
            got.append((step, self.windows[-1].copy()))
    mr.options, itcf_mod.ITCF.print_step = options, capture
    try:
        out = mr.drive(comm, nw_total, first, count)
    finally:
        mr.options, itcf_mod.ITCF.print_step = base_options, print_step
    out['itcf'] = got
    return out


def _worker(rank, port, q):
    try:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK='0')
        import torch
        import torch.distributed as dist
        from pauxy_amd.comm import TorchComm
        dist.init_process_group('gloo', rank=rank, world_size=2)
        comm = TorchComm(device=torch.device('cpu'))
        q.put((rank, drive(comm, 2 * mr.NW, rank * mr.NW, mr.NW)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:
        q.put((rank, repr(e)))
        raise


def test_two_ranks_give_the_itcf_of_one_rank():
    import numpy.random as npr
    keep = npr.normal, npr.random
    try:
        one = drive(None, 2 * mr.NW, 0, 2 * mr.NW)
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
    mr.compare(one, a, b)                       # the walkers and the mixed estimator agree, as without the ITCF
    steps = [s for s, _ in one['itcf']]
    assert steps == [4, 8, 12, 16, 20], steps
    assert [s for s, _ in a['itcf']] == steps and b['itcf'] == []
    got_phi = numpy.concatenate([a['phi'], b['phi']])
    print("ITCF-RANKS | walkers bitwise equal: %s (max difference %.2e)" % (numpy.array_equal(got_phi, one['phi']),
                                                                          numpy.max(numpy.abs(got_phi - one['phi']))))
    assert numpy.array_equal(got_phi, one['phi'])
    for (step, g1), (_, g2) in zip(one['itcf'], a['itcf']):
        print("ITCF-RANKS | window closing at step %d | two ranks vs one: %.2e" % (
            step, numpy.max(numpy.abs(g2 - g1)) / max(1.0, numpy.max(numpy.abs(g1)))))
        assert g1.shape == g2.shape == (4, 2, 2, 12, 12) and numpy.isfinite(g1).all()
        # mr.compare's walkers are bitwise those of one rank (asserted here), so the windows differ by the order of the
        # sum over walkers alone: MARGIN x 1e-15 of tests/itcf_ref_ext.py
        assert numpy.max(numpy.abs(g2 - g1)) <= 100 * 1e-15 * max(1.0, numpy.max(numpy.abs(g1)))
