"""Clouds that drive every way the device loop finds the trim limit (lsgpu_policy.h, k_normal_eq_loop), and
the numpy model of the distances the loop sees -- numpy plus the CPU oracle, no device.  Test infrastructure only.

The reference is a room corner: three orthogonal walls of M x M points at spacing SP with analytic normals (one plane
would make the 6x6 system singular).  A wall's normal is the axis along which all its points are 0, so a reading point
made by lifting a reference point by `off` along its normal has, in the mean-centred frame, exactly the squared distance
off * off to it whenever `off` is a multiple of 2^-18: every coordinate stays in one binade and nothing is rounded.
`pairs` puts every chosen point into the reading twice, lifted by +off and by -off; the residuals cancel exactly, the
update is 0 in every iteration, T stays where it was and iteration 0's distances are every iteration's distances.

Cases (trim ratio RATIO; A-D: T_init = I, thresholds 0, 12 iterations, the loop ends on the counter):
  identical       the reference itself: every d2 is 0, limit 0, every pair kept
  zeros_majority  80 % copies + pairs of a tenth of the points: limit 0 with a positive tail that is left out
  overfull        40 % copies + pairs of 30 % of the points, all at 1/32: the limit 2^-10 is tied 7372 times, the rank
                  sits in the middle of the ties and every one of them is kept
  thin256/thin258 12 000 reading points, all in pairs; a block of 256 / 258 ties at 2^-10 across the rank, alone in its
                  2^11-bit-step slice: exactly at / two above the in-kernel ranking's capacity
  jump            tight checker, cap 40, half the points lifted by +-1/32 once each (unbalanced): the limit grows by more
                  than the search cap's 1.1 in one iteration, stays in its 12-bit bin for the next, then falls to 0.64 x
                  its predecessor on the first iteration the accelerated selects are armed for
"""
import functools

import numpy as np

M, SP = 64, 0.1
N_REF = 3 * M * M
RATIO = 0.75
QUANT = 2.0 ** -18      # offsets are multiples of this: exact in the centred frame (see above)
TIE_OFF = 1.0 / 32      # its square, 2^-10, is the tied limit of overfull / thin* / jump's first iteration
CASES = ("identical", "zeros_majority", "overfull", "thin256", "thin258", "jump")


@functools.lru_cache(maxsize=None)
def corner():
    """-> (xyz1 (N_REF, 4) float32, normals (N_REF, 3) float32): walls z = 0, x = 0, y = 0."""
    g = (SP * np.arange(1, M + 1)).astype(np.float32)
    u, v = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    o = np.zeros_like(u)
    walls = [(np.stack([u, v, o], 1), (0, 0, 1)), (np.stack([o, u, v], 1), (1, 0, 0)), (np.stack([u, o, v], 1), (0, 1, 0))]
    xyz = np.ones((N_REF, 4), np.float32)
    xyz[:, :3] = np.concatenate([w for w, _ in walls])
    nrm = np.concatenate([np.tile(np.float32(n), (M * M, 1)) for _, n in walls])
    xyz.setflags(write=False)
    nrm.setflags(write=False)
    return xyz, nrm


def _offsets(rng, lo, hi, count):
    return (np.round(rng.uniform(lo, hi, count) / QUANT) * QUANT).astype(np.float32)


def lifted(idx, off):
    ref, nrm = corner()
    out = ref[idx].copy()
    out[:, :3] += np.asarray(off, np.float32).reshape(-1, 1) * nrm[idx]
    return out


def pairs(idx, off):
    """Every reference point of `idx` twice: lifted by +off and by -off along its normal."""
    off = np.broadcast_to(np.asarray(off, np.float32), (len(idx),))
    return np.concatenate([lifted(idx, off), lifted(idx, -off)])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, ref, nrm, reading, T_init (4x4), cfg (the checker's fields, for the oracle's and the device's config))."""
    ref, nrm = corner()
    n = N_REF
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)
    cfg = dict(trim_ratio=RATIO, max_iterations=12, min_diff_rot=0.0, min_diff_trans=0.0)
    if name == "identical":
        reading = ref.copy()
    elif name == "zeros_majority":
        t = n // 10
        reading = np.concatenate([ref[perm[:8 * t]], pairs(perm[8 * t:9 * t], _offsets(rng, 0.01, 0.05, t))])
    elif name == "overfull":
        c, p = int(0.4 * n), int(0.3 * n)
        reading = np.concatenate([ref[perm[:c]], pairs(perm[c:c + p], TIE_OFF)])
    elif name in ("thin256", "thin258"):
        ties = int(name[4:])
        total, rank = 12000, int(RATIO * 12000)
        below = (rank - 128) // 2                       # pairs under the tie block: the block starts 128 under the rank
        above = total // 2 - below - ties // 2
        off = np.concatenate([_offsets(rng, 0.002, 0.025, below), np.full(ties // 2, TIE_OFF, np.float32),
                              _offsets(rng, 0.04, 0.06, above)])
        reading = pairs(perm[:total // 2], off)
    elif name == "jump":
        sel = np.random.default_rng(5).permutation(n)[:n // 2]
        sign = np.where(np.arange(len(sel)) % 2 == 0, 1.0, -1.0).astype(np.float32)
        reading = ref.copy()
        reading[sel] = lifted(sel, sign * np.float32(TIE_OFF))
        cfg.update(max_iterations=40, min_diff_rot=1e-5, min_diff_trans=1e-4)
    else:
        raise KeyError(name)
    reading = np.ascontiguousarray(reading, np.float32)
    reading.setflags(write=False)
    return dict(name=name, ref=ref, nrm=nrm, reading=reading, T_init=np.eye(4), cfg=cfg)


_ORACLE_RUNS = {}


def oracle_run(oracle, name):
    """The CPU oracle's alignment of a case, computed once -> dict(rc, T (16, column major), iterations, trace)."""
    if name not in _ORACLE_RUNS:
        c = case(name)
        ocfg = oracle.config_yaml(accum_double=1, **c["cfg"])
        T16 = np.ascontiguousarray(c["T_init"].astype(np.float32).T).reshape(16)
        rc, To, st, tr = oracle.icp_compute(ocfg, c["reading"], c["ref"], c["nrm"], T16, 64)
        _ORACLE_RUNS[name] = dict(rc=rc, T=To, iterations=st.iterations, trace=tr)
    return _ORACLE_RUNS[name]


def distances_per_iteration(oracle, name, trace):
    """The squared distances the loop's select sees in every iteration of `trace` (the oracle's): the reading under T_init
    with the float reference mean taken off its translation, then under T_iter of the iteration before; nearest neighbours
    from the oracle's k-d tree on the centred reference."""
    c = case(name)
    ref = c["ref"]
    mean = (ref[:, :3].astype(np.float64).sum(0) / ref.shape[0]).astype(np.float32)
    ref_c = ref.copy()
    ref_c[:, :3] -= mean
    T0 = np.ascontiguousarray(c["T_init"].astype(np.float32).T).reshape(16).copy()
    T0[12:15] -= mean
    q0 = oracle.transform_points(T0, c["reading"])
    kd = oracle.KdTree(ref_c)
    out = []
    for k in range(len(trace)):
        q = q0 if k == 0 else oracle.transform_points(trace[k - 1]["T_iter"], q0)
        out.append(kd.nn(q)[1])
    return out


def bits(x):
    return int(np.float32(x).view(np.uint32))


def slice_count(d2, limit):
    """How many distances share the limit's 2^11-bit-step slice (what the in-kernel ranking sets aside)."""
    return int(((np.asarray(d2, np.float32).view(np.uint32) >> 11) == (bits(limit) >> 11)).sum())
