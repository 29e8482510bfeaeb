"""Charge and spin correlation functions from the back-propagated ``two_rdm: 'correlation'`` array (host numpy only).

The estimator (estimators/back_propagation.py, kernels in csrc/k_corr.hip) stores per window the un-normalised
corr [5, M, M]: <n_is n_jt> in the slices 2s+t (s, t = 0 up, 1 down) and <S+_i S-_j> in slice 4.  The functions here
take NORMALISED inputs, ``two_rdm / denominator`` and ``one_rdm / denominator`` (utils.io.extract_rdm returns them so).
"""
import numpy


def spin_charge(corr, one_rdm):
    """(charge, szsz, ss), each [M, M], from corr [5, M, M] and one_rdm [2, M, M]:

      charge[i,j] = <n_i n_j>      = sum_st corr[2s+t]                                   n_i = n_i,up + n_i,down
      szsz[i,j]   = <Sz_i Sz_j>    = (corr[0] - corr[1] - corr[2] + corr[3]) / 4
      ss[i,j]     = <S_i . S_j>    = szsz + (corr[4] + corr[4]^T) / 2 - d_ij (one_rdm[0][i,i] - one_rdm[1][i,i]) / 2

    (S_i . S_j = Sz_i Sz_j + (S+_i S-_j + S-_i S+_j) / 2 and S-_i S+_j = S+_j S-_i - 2 d_ij Sz_i.)
    The result does not depend on the convention of the Green's function, G[i,j] = <c+_i c_j> or its transpose (the
    back-propagated one is the transpose): the slices 0-3 and the diagonal of one_rdm are the same for both, and slice 4
    is transposed with G but enters only as corr[4] + corr[4]^T."""
    corr = numpy.asarray(corr)
    one_rdm = numpy.asarray(one_rdm)
    charge = corr[0] + corr[1] + corr[2] + corr[3]
    szsz = 0.25 * (corr[0] - corr[1] - corr[2] + corr[3])
    ss = szsz + 0.5 * (corr[4] + corr[4].T) - 0.5 * numpy.diag(numpy.diag(one_rdm[0]) - numpy.diag(one_rdm[1]))
    return charge, szsz, ss


def translation_average(c, nx, ny):
    """out [ny, nx]: out[ry, rx] = mean over the sites i of c[i, i + r] on the periodic nx x ny lattice, with the site
    ordering of systems.Hubbard, i = ix + nx * iy (ny = 1: a chain)."""
    c = numpy.asarray(c)
    M = nx * ny
    if c.shape != (M, M):
        raise ValueError("translation_average: c must be [nx * ny, nx * ny]")
    ix, iy = numpy.arange(M) % nx, numpy.arange(M) // nx
    out = numpy.zeros((ny, nx), dtype=c.dtype)
    for ry in range(ny):
        for rx in range(nx):
            j = (ix + rx) % nx + nx * ((iy + ry) % ny)
            out[ry, rx] = numpy.mean(c[numpy.arange(M), j])
    return out
