"""Everything a walker carries arrives with it, on every way a walker can move, with back-propagation, walker.G (mixed
one_rdm) and the log shift all switched on at once: afq_walkers_copy, afq_walker_pack / unpack, the clones of a one-rank
comb and of a pair-branch event, and the exchange slots of a two-rank comb.  The library lists a walker's arrays once
(csrc/walker_fields.h); an array missing from one of these paths shows up here as a column of the packed snapshot that
did not follow its walker.

Walkers are observed as afq_walker_pack lays them out (``snapshot`` of test_gpu_pair_branch.py) and compared bit for
bit, so there is no tolerance.  A destination equals its source in every column but the weight (the comb resets it, the
pair-branch plan writes it; the host copy and pack carry it along, which is asserted too).  A walker that is nobody's
destination keeps everything but its weight and its unscaled weight, which both plans rewrite for the whole population;
the clones copy the unscaled weight the plan left at the source, so destination and source are compared after the event.

The sizes are the formulas of the C ABI, per = M (na + nb):  afq_walker_pack_bytes = 16 (per + 4) + 32
[+ 16 (per + nbp K + 1) + 16 with back-propagation] [+ 32 M^2 with walker.G], and an exchange slot with a cached Green's
function is 2 per + 7 [+ per + nbp K + 2] [+ 2 M^2] units of 16 bytes."""
import numpy
import pytest

from pauxy_amd import _lib as L
from pauxy_amd import device as devmod
from pauxy_amd.walkers.handler import pair_branch_plan
from tests.helpers import generic_model, make_device
from tests.test_gpu_pair_branch import DeviceBuffer, columns, snapshot

pytestmark = pytest.mark.gpu
NW, NBP = 6, 3


@pytest.fixture(scope='module')
def model(golden):
    return generic_model(golden('generic_ops.npz'), 'A_')


def walkers_on(model, seed, bp=True, rdm=True):
    """NW walkers after three steps and one energy evaluation.  phi, phi_old, ot, the hybrid energy, the field history
    with its factors, walker.G and the cached Green's function are walker specific through the steps; eloc, detR, the
    phase, the unscaled weight and log_detR, which none of this writes, are set to distinct values.  Only the history length
    (3 for everyone) is not."""
    dev = make_device(model, NW)
    if rdm:
        dev.estimates_rdm(True)
    dev.set_log_shift(True, 0.3, 0.1)
    rng = numpy.random.RandomState(seed)
    nt = model.na + model.nb
    dev.set(L.F_PHI, model.psi[None] + 0.05 * (rng.rand(NW, model.M, nt) + 1j * rng.rand(NW, model.M, nt)))
    dev.set(L.F_OT, dev.calc_overlap())
    if bp:
        dev.bp_configure(NBP)                            # (phi_old starts as the current phi)
    dev.set(L.F_ELOC, rng.rand(NW) + 1j * rng.rand(NW))
    dev.set(L.F_DETR, 0.5 + rng.rand(NW))
    dev.set(L.F_PHASE, numpy.exp(1j * rng.rand(NW)))
    dev.set(L.F_LOG_DETR, 0.1 + rng.rand(NW))
    dev.set(L.F_UNSCALED_WEIGHT, 0.5 + rng.rand(NW))
    for _ in range(3):
        dev.propagate(rng.normal(size=(NW, dev.K)), 0.0)
    dev.estimates_update(True)
    return dev


def pack_bytes_formula(dev, bp, rdm):
    per = dev.M * (dev.na + dev.nb)
    return 16 * (per + 4) + 32 + (16 * (per + NBP * dev.K + 1) + 16 if bp else 0) + (32 * dev.M ** 2 if rdm else 0)


def slot_units_formula(dev, bp, rdm):
    per = dev.M * (dev.na + dev.nb)
    return 2 * per + 7 + (per + NBP * dev.K + 2 if bp else 0) + (2 * dev.M ** 2 if rdm else 0)


def bits(a):
    return numpy.ascontiguousarray(a).view(numpy.uint64)


def check_moved(dev, before, after, origin, src_after=None, weight_too=False):
    """after[i] is before[origin[i]]: see the module docstring.  src_after: the sources' snapshot after the event when
    they live on another handle."""
    origin = numpy.asarray(origin)
    ucol, wcol = columns(dev)
    moved = origin != numpy.arange(len(origin)) if src_after is None else numpy.ones(len(origin), dtype=bool)
    assert moved.any()
    but_weight = numpy.ones(after.shape[1], dtype=bool)
    but_weight[wcol] = weight_too
    kept = but_weight.copy()
    kept[ucol] = weight_too
    src = after if src_after is None else src_after
    assert numpy.array_equal(bits(after[moved][:, but_weight]), bits(src[origin[moved]][:, but_weight]))
    assert numpy.array_equal(bits(after[~moved][:, kept]), bits(before[~moved][:, kept]))
    if src_after is None:       # the sources themselves are among the walkers that kept their state
        assert not numpy.isin(origin[moved], numpy.where(moved)[0]).any()


def test_the_walkers_differ_in_every_array(model):
    dev = walkers_on(model, 1)
    snap = snapshot(dev)
    assert snap.shape[1] * 8 == dev.pack_bytes() == pack_bytes_formula(dev, True, True)
    same = [c for c in range(snap.shape[1]) if len(set(bits(snap[:, c]).tolist())) == 1]
    print('columns equal for all walkers:', same)
    assert len(same) <= 1                                # the history length and its padding, one 8-byte column
    for c in set(range(snap.shape[1])) - set(same):
        assert len(set(bits(snap[:, c]).tolist())) == NW, c
    log_detR = dev.get(L.F_LOG_DETR)
    assert numpy.all(log_detR != 0.0) and len(set(log_detR.tolist())) == NW
    assert numpy.array_equal(snap[:, columns(dev)[1] + 1], log_detR)
    dev.close()


def test_copy_walker(model):
    dev = walkers_on(model, 2)
    before = snapshot(dev)
    dev.copy_walker(1, 4)
    check_moved(dev, before, snapshot(dev), [0, 1, 2, 3, 1, 5], weight_too=True)
    dev.close()


def test_pack_and_unpack_into_another_index(model):
    dev = walkers_on(model, 3)
    before = snapshot(dev)
    buf = DeviceBuffer(dev, dev.pack_bytes())
    dev.pack(2, buf.ptr.value)
    dev.unpack(5, buf.ptr.value)
    dev.sync()
    buf.free()
    check_moved(dev, before, snapshot(dev), [0, 1, 2, 3, 4, 2], weight_too=True)
    dev.close()


def test_one_rank_comb(model):
    """Weights 3, 3, 3, 1e-3, 1e-3, 1e-3 and r = 0.37: the teeth (k + r) 9.003 / 6 fall two on each heavy walker and none on
    a light one, so the pairs are (0, 3), (1, 4), (2, 5)."""
    dev = walkers_on(model, 4)
    dev.set(L.F_WEIGHT, numpy.array([3.0, 3.0, 3.0, 1e-3, 1e-3, 1e-3]))
    before = snapshot(dev)
    pix, _ = dev.popcontrol_comb(0.37, NW)
    assert pix.tolist() == [2, 2, 2, 0, 0, 0]
    after = snapshot(dev)
    check_moved(dev, before, after, [0, 1, 2, 0, 1, 2])
    assert numpy.all(after[:, columns(dev)[1]] == 1.0)
    dev.close()


def test_one_rank_pair_branch(model):
    dev = walkers_on(model, 5)
    w = numpy.array([0.05, 2.5, -1.3, 1.0, 6.0, 0.1])
    u = numpy.full(NW // 2, 0.5)
    new_w, mult_h, pairs, nd_h = pair_branch_plan(w / (numpy.abs(w).sum() / NW), 0.1, 4.0, u)
    assert nd_h == 2
    dev.set(L.F_WEIGHT, w)
    before = snapshot(dev)
    mult, nd, _ = dev.popcontrol_pair_branch(u, NW, 0.1, 4.0)
    assert nd == nd_h and numpy.array_equal(mult, mult_h)
    origin = numpy.arange(NW)
    for c, k in pairs:
        origin[k] = c
    check_moved(dev, before, snapshot(dev), origin)
    dev.close()


@pytest.mark.parametrize('bp,rdm', [(True, True), (True, False), (False, True), (False, False)])
def test_two_rank_comb_and_the_sizes(model, bp, rdm):
    """Every heavy walker on rank 0, every dead one on rank 1: walker i of rank 1 becomes walker i of rank 0, and rank 0 has
    written NW slots of the formula's size."""
    ranks = [walkers_on(model, 6 + i, bp, rdm) for i in range(2)]
    devmod.comm_init_local(ranks)
    for rk in ranks:
        assert rk.pack_bytes() == pack_bytes_formula(rk, bp, rdm)
        rk.comm_set_capacity(NW)
    ranks[0].set(L.F_WEIGHT, numpy.full(NW, 3.0))
    ranks[1].set(L.F_WEIGHT, numpy.full(NW, 1e-3))
    before = [snapshot(rk) for rk in ranks]
    assert not numpy.array_equal(before[0][:, :columns(ranks[0])[0]], before[1][:, :columns(ranks[0])[0]])
    pix, _ = devmod.popcontrol_comb_local(ranks, 0.37, 2 * NW)
    assert numpy.all(pix[:NW] == 2) and numpy.all(pix[NW:] == 0)
    after = [snapshot(rk) for rk in ranks]
    check_moved(ranks[1], before[1], after[1], numpy.arange(NW), src_after=after[0])
    ucol, wcol = columns(ranks[0])
    kept = numpy.ones(after[0].shape[1], dtype=bool)
    kept[[ucol, wcol]] = False
    assert numpy.array_equal(bits(after[0][:, kept]), bits(before[0][:, kept]))
    st = [rk.comm_stats() for rk in ranks]
    print('bytes sent per walker', st[0]['bytes_sent'] // NW, 'formula', 16 * slot_units_formula(ranks[0], bp, rdm))
    assert st[0]['walkers_sent'] == NW and st[1]['walkers_sent'] == 0 and st[0]['error'] == 0 and st[0]['overflow'] == 0
    assert st[0]['bytes_sent'] == NW * 16 * slot_units_formula(ranks[0], bp, rdm) and st[1]['bytes_sent'] == 0
    for rk in ranks:
        rk.close()
