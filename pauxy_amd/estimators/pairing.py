"""Pair-field correlation functions from the back-propagated ``two_rdm: 'pairing'`` array (host numpy only).

The estimator (estimators/back_propagation.py, kernels in csrc/k_pair.hip) stores per window the un-normalised
pair [nb, nb, M, M] over a bond table nbr [nb, M] (nbr[b][i] = i_b, the partner site of i along bond b, -1 = none).  With
D+(k, l) = c+_k,up c+_l,down and P(k, l; m, n) = <D+(k, l) D(m, n)>,

    pair[b, b', i, j] = P(i, i_b; j, j_b') = G_0[i, j] G_1[i_b, j_b']        for G[i,j] = <c+_i c_j>.

The functions here take NORMALISED inputs, ``two_rdm / denominator`` and ``one_rdm / denominator`` (utils.io.extract_rdm
returns them so).  The back-propagated Green's function is the transpose of <c+_i c_j>, and the stored array is the
transposed form X[b, b', i, j] = pair[b', b, j, i].  `uncorrelated`, `singlet` and `channel` (with real weights) commute
with that exchange of the index pairs: given transposed-form inputs they return the transposed form of their result,
so that nothing has to be converted on the way; ``x.transpose(1, 0, 3, 2)`` converts an array at the end (or at the start).
"""
import numpy


def lattice_bonds(nx, ny, periodic=True):
    """(nbr int32 [nb, M], inverse [nb]) of the nx x ny lattice with the site order of systems.Hubbard, i = ix + nx iy:
    the bonds on-site, +x, -x, +y, -y (ny = 1: on-site, +x, -x).  periodic=False puts -1 where the partner would cross
    an edge.  inverse[b] is the bond of the opposite displacement: nbr[inverse[b]][nbr[b][i]] == i wherever nbr[b][i]
    is a site."""
    M = nx * ny
    ix, iy = numpy.arange(M) % nx, numpy.arange(M) // nx
    steps = [(0, 0), (1, 0), (-1, 0)] + ([(0, 1), (0, -1)] if ny > 1 else [])
    nbr = numpy.zeros((len(steps), M), dtype=numpy.int32)
    for b, (dx, dy) in enumerate(steps):
        jx, jy = ix + dx, iy + dy
        inside = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny)
        nbr[b] = numpy.where(inside | periodic, jx % nx + nx * (jy % ny), -1)
    inverse = numpy.array([0, 2, 1, 4, 3][:len(steps)])
    return nbr, inverse


def _gather(a, rows, cols):
    """out[b, b', i, j] = a[b, b', rows[b][i], cols[b'][j]], 0 where either index is -1."""
    nb, M = rows.shape
    ok = (rows >= 0)[:, None, :, None] & (cols >= 0)[None, :, None, :]
    r, c = numpy.maximum(rows, 0)[:, None, :, None], numpy.maximum(cols, 0)[None, :, None, :]
    b, bp = numpy.arange(nb)[:, None, None, None], numpy.arange(nb)[None, :, None, None]
    return numpy.where(ok, a[b, bp, r, c], 0)


def uncorrelated(one_rdm, nbr):
    """[nb, nb, M, M]: the pairing array of the averaged Green's function one_rdm [2, M, M],
    one_rdm[0][i, j] one_rdm[1][i_b, j_b'], so that ``pair - uncorrelated(one_rdm, nbr)`` is the vertex part."""
    one_rdm, nbr = numpy.asarray(one_rdm), numpy.asarray(nbr)
    nb = nbr.shape[0]
    g1 = numpy.broadcast_to(one_rdm[1], (nb, nb) + one_rdm[1].shape)
    return one_rdm[0][None, None] * _gather(g1, nbr, nbr)


def singlet(pair, nbr, inverse):
    """[nb, nb, M, M]: <Ds+_b(i) Ds_b'(j)> of the singlet pair field Ds+_b(i) = (D+(i, i_b) + D+(i_b, i)) / sqrt(2),

        1/2 [P(i, i_b; j, j_b') + P(i, i_b; j_b', j) + P(i_b, i; j, j_b') + P(i_b, i; j_b', j)],

    each term an element of `pair`: D+(i_b, i) is the pair of site i_b along the bond inverse[b].  0 where i_b or j_b'
    is -1.  The on-site bond gives Ds+ = sqrt(2) D+(i, i): its diagonal element is 2 <n_i,up n_i,down>."""
    pair, nbr, inverse = numpy.asarray(pair), numpy.asarray(nbr), numpy.asarray(inverse)
    nb, M = nbr.shape
    own = numpy.broadcast_to(numpy.arange(M), (nb, M))
    own = numpy.where(nbr >= 0, own, -1)                # (the undefined pair fields are left out of every term)
    flip_b = pair[inverse]                              # [b, b', ...] = pair[inverse[b], b', ...]
    flip_c = pair[:, inverse]
    flip_bc = pair[inverse][:, inverse]
    return 0.5 * (_gather(pair, own, own) + _gather(flip_c, own, nbr) + _gather(flip_b, nbr, own)
                  + _gather(flip_bc, nbr, nbr))


def channel(ps, form):
    """[M, M]: sum_bb' form[b] form[b'] ps[b, b', i, j], the correlator of the pair field sum_b form[b] Ds+_b(i) with
    one real weight per bond (s_wave, extended_s, d_wave)."""
    form = numpy.asarray(form, dtype=float)
    return numpy.einsum('b,c,bcij->ij', form, form, numpy.asarray(ps))


def s_wave(nb=5):
    """The on-site pair of the table of lattice_bonds."""
    f = numpy.zeros(nb)
    f[0] = 1.0
    return f


def extended_s(nb=5):
    """+1 on every neighbour bond of the table of lattice_bonds, normalised: / 2 on the square lattice."""
    f = numpy.ones(nb) / numpy.sqrt(nb - 1.0)
    f[0] = 0.0
    return f


def d_wave(nb=5):
    """+1 on the bonds +-x, -1 on +-y, / 2 (the table of lattice_bonds with ny > 1)."""
    if nb != 5:
        raise ValueError("d_wave: the five bonds of a two-dimensional lattice")
    return numpy.array([0.0, 0.5, 0.5, -0.5, -0.5])
