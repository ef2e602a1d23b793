"""Independent model of CovarianceSamplingDataPointsFilter: numpy only, written from the text of include/lsgpu_icp.h
("CovarianceSamplingDataPointsFilter", steps 1-9); it calls nothing of the library.  Every float operation is one numpy float32
operation (one rounding, no fma), every double one a float64 one; sums run left to right in index order."""
from __future__ import annotations

import numpy as np

F = np.float32
D = np.float64


class BadArg(Exception):
    """The text's LSGPU_BAD_ARG."""


def jacobi(C21):
    """Step 5 -> (X (6, 6) float32, column k the k-th eigenvector; values (6,) float64, ascending)."""
    A = np.zeros((6, 6), D)
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = D(C21[k])
            k += 1
    V = np.eye(6, dtype=D)
    one, two = D(1.0), D(2.0)
    with np.errstate(all="ignore"):   # (a tiny a_pq: theta overflows to inf, t is 0 -- as in C)
        _sweeps(A, V, one, two)
    order = sorted(range(6), key=lambda j: (A[j, j], j))
    X = np.stack([V[:, j] for j in order], axis=1).astype(F)
    return X, np.array([A[j, j] for j in order], D)


def _sweeps(A, V, one, two):
    for _sweep in range(30):
        off = D(0.0)
        for p in range(6):
            for q in range(p + 1, 6):
                off = off + A[p, q] * A[p, q]
        if off == 0.0:
            break
        for p in range(6):
            for q in range(p + 1, 6):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (two * apq)
                at = np.abs(theta) + np.sqrt(theta * theta + one)
                t = -one / at if theta < 0.0 else one / at
                cs = one / np.sqrt(t * t + one)
                sn = t * cs
                for r in range(6):
                    akp, akq = A[r, p], A[r, q]
                    A[r, p] = cs * akp - sn * akq
                    A[r, q] = sn * akp + cs * akq
                for r in range(6):
                    apk, aqk = A[p, r], A[q, r]
                    A[p, r] = cs * apk - sn * aqk
                    A[q, r] = sn * apk + cs * aqk
                A[p, q] = A[q, p] = D(0.0)
                for r in range(6):
                    vkp, vkq = V[r, p], V[r, q]
                    V[r, p] = cs * vkp - sn * vkq
                    V[r, q] = sn * vkp + cs * vkq


def _seq_sum(x):
    """Left-to-right sum in the array's own type (np.cumsum adds sequentially)."""
    return np.cumsum(x)[-1]


def sums_and_vectors(xyz1, normals, torque_norm, S=None, len_sum=None):
    """Steps 1-4 -> (c, Lnorm, v (n, 6) float32, C21 (21,) float64).  S / len_sum: the sums of step 1 / of the lengths of step 2
    taken as given instead of added here (what follows them is formed from them)."""
    p = np.asarray(xyz1, F)[:, :3]
    nr = np.asarray(normals, F)
    n = p.shape[0]
    with np.errstate(all="ignore"):
        S = np.array([_seq_sum(p[:, a].astype(D)) for a in range(3)], D) if S is None else np.asarray(S, D)
        if not np.all(np.isfinite(S)):
            raise BadArg("S")
        c = (S / D(n)).astype(F)
        d = p - c
        if torque_norm == 0:
            L = F(1.0)
        elif torque_norm == 1:
            ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            L = F((_seq_sum(ln.astype(D)) if len_sum is None else D(len_sum)) / D(n))
        else:
            ext = p.max(axis=0) - p.min(axis=0)
            L = F(ext.max() * F(0.5))
        if L == 0 or not np.isfinite(L):
            raise BadArg("Lnorm")
        invL = F(1.0) / L
        mx = d[:, 1] * nr[:, 2] - d[:, 2] * nr[:, 1]
        my = d[:, 2] * nr[:, 0] - d[:, 0] * nr[:, 2]
        mz = d[:, 0] * nr[:, 1] - d[:, 1] * nr[:, 0]
        v = np.stack([invL * mx, invL * my, invL * mz, nr[:, 0], nr[:, 1], nr[:, 2]], axis=1).astype(F)
        vd = v.astype(D)
        C21 = np.array([_seq_sum(vd[:, a] * vd[:, b]) for a in range(6) for b in range(a, 6)], D)
    if not np.all(np.isfinite(C21)):
        raise BadArg("C")
    return c, L, v, C21


def magnitudes(v, X):
    """Step 6 -> (n, 6) float32."""
    with np.errstate(all="ignore"):
        cols = []
        for k in range(6):
            s = v[:, 0] * X[0, k] + v[:, 1] * X[1, k]
            for a in range(2, 6):
                s = s + v[:, a] * X[a, k]
            cols.append(np.abs(s))
    return np.stack(cols, axis=1).astype(F)


def walk(mag, nb):
    """Steps 7-8 -> the nb chosen indices in pick order."""
    n = mag.shape[0]
    # decreasing magnitude, ties by ascending index: a stable ascending sort of the complemented bit patterns
    lists = [np.argsort(~mag[:, k].view(np.uint32), kind="stable") for k in range(6)]
    pos = [0] * 6
    chosen = np.zeros(n, bool)
    t = np.zeros(6, F)
    out = []
    with np.errstate(all="ignore"):
        for _ in range(nb):
            k = 0
            for i in range(6):
                if t[k] > t[i]:
                    k = i
            while chosen[lists[k][pos[k]]]:
                pos[k] += 1
            i = int(lists[k][pos[k]])
            pos[k] += 1
            chosen[i] = True
            out.append(i)
            t = t + mag[i] * mag[i]
    return np.array(out, np.int32)


def cov_sampling(xyz1, normals, nb_sample, torque_norm):
    """The module -> (xyz1', normals', ids)."""
    xyz1 = np.asarray(xyz1, F)
    normals = np.asarray(normals, F)
    n = xyz1.shape[0]
    if nb_sample >= n:
        return xyz1.copy(), normals.copy(), np.arange(n, dtype=np.int32)
    _c, _L, v, C21 = sums_and_vectors(xyz1, normals, torque_norm)
    X, _w = jacobi(C21)
    ids = walk(magnitudes(v, X), nb_sample)
    return xyz1[ids], normals[ids], ids
