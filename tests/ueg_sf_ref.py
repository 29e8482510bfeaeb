"""numpy restatement of the UEG energy's pair sums per momentum transfer (test infrastructure).

  Gkpq[s,q]  = sum_a G_s[ikpq_i[q][a], ikpq_kpq[q][a]]        Gpmq[s,q] = sum_b G_s[ipmq_i[q][b], ipmq_pmq[q][b]]
  Gprod[s,q] = sum_{a,b} G_s[ipmq_i[q][b], ikpq_kpq[q][a]] G_s[ikpq_i[q][a], ipmq_pmq[q][b]]
  two_rdm[s,s,q] = Gkpq[s,q] Gpmq[s,q] - Gprod[s,q]           two_rdm[s,t,q] = Gkpq[s,q] Gpmq[t,q]   (s != t)
  ke = sum_s sum_i H1[s,i,i] G_s[i,i]     pe = 1 / (2 vol) sum_q vqvec[q] sum_st two_rdm[s,t,q]

Written from these formulas with fancy indexing per momentum transfer; ``system`` is anything with the attributes
ikpq_i, ikpq_kpq, ipmq_i, ipmq_pmq (lists of index arrays), vqvec, vol and H1 [2, M, M] (diagonal).
"""
import numpy


def lists_of(system):
    return system.ikpq_i, system.ikpq_kpq, system.ipmq_i, system.ipmq_pmq


def pair_sums(lists, G):
    """two_rdm[2, 2, nq] of one Green's function G[2, M, M]."""
    ki, kk, pi, pp = lists
    nq = len(ki)
    G = numpy.asarray(G, dtype=numpy.complex128)
    gk = numpy.zeros((2, nq), dtype=numpy.complex128)
    gp = numpy.zeros((2, nq), dtype=numpy.complex128)
    gx = numpy.zeros((2, nq), dtype=numpy.complex128)
    for s in range(2):
        for q in range(nq):
            a_i, a_k = numpy.asarray(ki[q], dtype=int), numpy.asarray(kk[q], dtype=int)
            b_i, b_p = numpy.asarray(pi[q], dtype=int), numpy.asarray(pp[q], dtype=int)
            gk[s, q] = G[s][a_i, a_k].sum()
            gp[s, q] = G[s][b_i, b_p].sum()
            if len(a_i) and len(b_i):
                gx[s, q] = (G[s][b_i[None, :], a_k[:, None]] * G[s][a_i[:, None], b_p[None, :]]).sum()
    two = numpy.zeros((2, 2, nq), dtype=numpy.complex128)
    two[0, 0] = gk[0] * gp[0] - gx[0]
    two[1, 1] = gk[1] * gp[1] - gx[1]
    two[0, 1] = gk[0] * gp[1]
    two[1, 0] = gk[1] * gp[0]
    return two


def energy(system, G, two):
    """(E, ke, pe) from the pair sums ``two`` of G (no ecore)."""
    h = numpy.asarray(system.H1)
    ke = sum(numpy.dot(numpy.diag(h[s]), numpy.diag(G[s])) for s in range(2))
    pe = numpy.dot(numpy.asarray(system.vqvec), two.sum(axis=(0, 1))) / (2.0 * system.vol)
    return numpy.array([ke + pe, ke, pe])


def evaluate(system, G):
    two = pair_sums(lists_of(system), G)
    return energy(system, G, two), two


def window(system, Gs, wts):
    """(sum_w wt_w (E, ke, pe)[G_w], sum_w wt_w two_rdm[G_w]) over Green's functions Gs[w, 2, M, M]."""
    E = numpy.zeros(3, dtype=numpy.complex128)
    two = None
    for G, wt in zip(Gs, wts):
        if wt == 0:
            continue
        e, t = evaluate(system, G)
        E += wt * e
        two = wt * t if two is None else two + wt * t
    return E, two


def hubbard_energy(T, U, G):
    """estimators/hubbard.py:93-114 on a full Green's function."""
    ke = numpy.sum(T[0] * G[0] + T[1] * G[1])
    pe = U * numpy.dot(numpy.diag(G[0]), numpy.diag(G[1]))
    return numpy.array([ke + pe, ke, pe])


def ragged(d, name):
    flat, off = d[name], d[name + '_off']
    return [flat[off[i]:off[i + 1]].astype(numpy.int64) for i in range(len(off) - 1)]
