"""Numpy restatement of the pairing correlations of one Green's function G [2, M, M] (spin 0 = up, 1 = down) over a bond
table nbr [nb, M] (partner sites, -1 = none), written from Wick's theorem for one pair of determinants and not from
the kernel (pauxy_amd/csrc/k_pair.hip): a gather and a product,

    pair[b, b', i, j] = G_0[i, j] G_1[nbr[b][i], nbr[b'][j]]      <c+_i,up c+_ib,down c_jb',down c_j,up>, G[i,j] = <c+_i c_j>

and 0 where either partner is -1, whatever G holds.  `window` sums over walkers in numpy.longdouble."""
import numpy


def pair(G, nbr, dtype=numpy.complex128):
    G = numpy.asarray(G).astype(dtype)
    nbr = numpy.asarray(nbr)
    ok = nbr >= 0
    at = numpy.where(ok, nbr, 0)
    g1 = G[1][at[:, None, :, None], at[None, :, None, :]]                     # [nb, nb, M, M]
    both = ok[:, None, :, None] & ok[None, :, None, :]
    return numpy.where(both, G[0][None, None] * g1, 0).astype(dtype)


def window(Gs, wts, nbr):
    """sum_w wts[w] pair(Gs[w]) in extended precision, returned as complex128; weight-zero walkers are left out."""
    nb, M = numpy.asarray(nbr).shape
    acc = numpy.zeros((nb, nb, M, M), dtype=numpy.clongdouble)
    for G, w in zip(Gs, wts):
        if w != 0:
            acc += numpy.clongdouble(w) * pair(G, nbr, numpy.clongdouble)
    return acc.astype(numpy.complex128)


def chain_table(M):
    """on-site, +1, -1 on a periodic chain of M sites."""
    i = numpy.arange(M)
    return numpy.array([i, (i + 1) % M, (i - 1) % M], dtype=numpy.int32)


def random_table(nb, M, seed):
    """Any table: random partners with repeated targets and about one entry in five -1 (at least one where M allows)."""
    rng = numpy.random.RandomState(seed)
    nbr = rng.randint(0, M, size=(nb, M)).astype(numpy.int32)
    nbr[rng.rand(nb, M) < 0.2] = -1
    nbr[nb - 1, M - 1] = -1
    nbr[0, 0] = min(1, M - 1)
    if M > 2:
        nbr[0, 1] = nbr[0, 2] = 0               # a repeated target
    return nbr
