"""Numpy restatement of the correlation functions of one Green's function G [2, M, M] (spin 0 = up, 1 = down), written
from Wick's theorem for one pair of determinants and not from the kernel (pauxy_amd/csrc/k_corr.hip):

    corr[2s+t][i,j] = G_s[i,i] G_t[j,j]                                   s != t     <n_is n_jt>
    corr[2s+s][i,j] = G_s[i,i] G_s[j,j] + G_s[i,j] (d_ij - G_s[j,i])                 <n_is n_js>
    corr[4][i,j]    = G_0[i,j] (d_ij - G_1[j,i])                                     <S+_i S-_j>, G[i,j] = <c+_i c_j>

`window` sums over walkers in numpy.longdouble."""
import numpy


def corr(G, dtype=numpy.complex128):
    G = numpy.asarray(G).astype(dtype)
    M = G.shape[-1]
    eye = numpy.eye(M).astype(dtype)
    n = [numpy.diag(G[0]), numpy.diag(G[1])]
    out = numpy.zeros((5, M, M), dtype=dtype)
    for s in range(2):
        for t in range(2):
            out[2 * s + t] = numpy.outer(n[s], n[t])
            if s == t:
                out[2 * s + t] += G[s] * (eye - G[s].T)
    out[4] = G[0] * (eye - G[1].T)
    return out


def window(Gs, wts):
    """sum_w wts[w] corr(Gs[w]) in extended precision, returned as complex128."""
    M = numpy.asarray(Gs[0]).shape[-1]
    acc = numpy.zeros((5, M, M), dtype=numpy.clongdouble)
    for G, w in zip(Gs, wts):
        acc += numpy.clongdouble(w) * corr(G, numpy.clongdouble)
    return acc.astype(numpy.complex128)
