"""Readings of every size at which k_normal_eq_loop takes another path (lsgpu_solve.hip.h: the grid, the unrolled
accumulation, the last block's reduction of the partials), and the numpy model of one iteration's 29 sums -- numpy plus the
CPU oracle, no device.  Test infrastructure only; tests/test_reading_sizes.py and tests/size_worker.py use it.

The reference is the 64-step scan of synth.scan_pair through the oracle's SamplingSurfaceNormal filter (knn 10, ratio 0.5,
seed 4): 2026 points with normals.  A reading of n points is n evenly spaced points of a denser reading of the same scene
from the same poses (scan_pair(RD_AZ): 69 461 points; scan_pair(WORKER_AZ): 138 925 for the worker's largest case), so
T_init and T_true are the 64-step pair's whatever n is.

What a size reaches.  The grid is nb = min(blocks, ceil(pairs / 256)), `blocks` 256 unless LSGPU_NE_BLOCKS says otherwise
(the worker runs with 64).  A lane's unroll slot u takes pair j0 + u * 256 * nb, so slot u is used iff pairs > u * 256 * nb,
and the outer loop runs a second round iff pairs > 8 * 256 * nb.  The last block gives each of 8 slices per = ceil(nb / 8)
rows of partials, loads them 16 at a time and the rest one by one: tail_shape(nb).

The model (Model.iteration) restates one iteration from a pose: transform (the oracle's, bit-identical with the device's),
exact nearest neighbours (the oracle's k-d tree; the two nearest from tests/cpp/knn_brute.c to see ties), the trimmed
limit by partition, and per kept pair the terms as the kernel forms them -- J = [p x n ; n] and r = (p - q) . n in float32,
one rounding per operation, the products J_a J_c and -J_a r in float64 (exact: 24 x 24 bits) -- summed per slot in
extended precision (pairwise, 64-bit mantissa: 1e-17 of sum |term| at these counts; math.fsum where long double is no
wider than double), together with sum |term| per slot, the scale of the bar.
"""
import functools
import hashlib
import math

import numpy as np

from laser_slam_amd import synth

REF_AZ, RD_AZ, WORKER_AZ = 64, 1088, 2176
RATIO = 0.75
DEFAULT_BLOCKS, WORKER_BLOCKS = 256, 64
UNROLL = 8          # kNeUnroll
BAR = 1e-12         # |device - model| <= BAR * sum |term| per entry: 80 dependent double additions at most, x 100
TIE_CAP = 8         # kept pairs per iteration whose two nearest reference points are equally far; above it the case fails
TOL_T, TOL_R = 1e-4, 1e-5   # m, rad: the bars of tests/test_gpu_parity.py

# reading size -> (the grid, the highest unroll slot in use, rounds of the outer loop, what the size is there for)
DEFAULT_SIZES = {
    7: (1, 0, 1, "smaller than a wave; the oracle does not converge"),
    63: (1, 0, 1, "one short of a wave and of a 64-query search tile"),
    64: (1, 0, 1, "exactly one wave, one search tile"),
    65: (1, 0, 1, "one past a wave"),
    255: (1, 0, 1, "one short of a block: the only block is its own last block"),
    256: (1, 0, 1, "exactly one block"),
    257: (2, 0, 1, "two blocks, the second with one pair: six slices empty"),
    1793: (8, 0, 1, "nb 8: every slice one row"),
    2049: (9, 0, 1, "nb 9: per 2, slices 5-7 start past the end"),
    30720: (120, 0, 1, "nb 120: per 15, tail rows only"),
    30721: (121, 0, 1, "nb 121: per 16, exactly one 16-row batch"),
    32769: (129, 0, 1, "nb 129: per 17, a batch plus one row"),
    65281: (256, 0, 1, "nb 256: the full grid, slot 0 only"),
    65537: (256, 1, 1, "nb 256: one lane in unroll slot 1"),
}
WORKER_SIZES = {
    2049: (9, 0, 1, "nb 9 again, under the other block count"),
    16385: (64, 1, 1, "nb 64: one lane in unroll slot 1"),
    30721: (64, 1, 1, "nb 64: slot 1 nearly full"),
    65537: (64, 4, 1, "nb 64: slots 0-4"),
    131073: (64, 7, 2, "nb 64: the second round of the outer loop"),
}
P2P_SIZES = (63, 65, 257, 2049, 30721, 32769, 65537)
KNN3_SIZES = {63: 1, 65: 1, 257: 4, 683: 9, 10241: 121}     # reading size -> the grid of its 3 n pairs
BATCH_SIZES = (63, 257, 2049, 30721)
SUMS_SIZES = (1, 63, 64, 65, 257, 4099, 65537)


def grid(pairs, blocks=DEFAULT_BLOCKS):
    """-> (nb, highest unroll slot in use, rounds of the outer loop) of a launch over `pairs` pairs."""
    nb = min(blocks, -(-pairs // 256))
    stride = 256 * nb
    return nb, min(UNROLL - 1, (pairs - 1) // stride), -(-pairs // (UNROLL * stride))


def tail_shape(nb):
    """The last block's reduction of nb rows: rows per slice, slices with rows, slices that start past the end, the most
    16-row batches and single rows any slice loads."""
    per = -(-nb // 8)
    rows = [max(0, min(nb, (s + 1) * per) - s * per) for s in range(8)]
    return dict(per=per, filled=sum(r > 0 for r in rows), past_end=sum(s * per > nb for s in range(8)),
                batches=max(r // 16 for r in rows), singles=max(r % 16 for r in rows))


# ------------------------------------------------------------------------------------------------ the clouds
@functools.lru_cache(maxsize=None)
def scans(n_az):
    ref, rd, T_true, T_init = synth.scan_pair(n_az)
    for a in (ref, rd):
        a.setflags(write=False)
    return ref, rd, T_true, T_init


def poses():
    """-> (T_init, T_true) of the 64-step pair: every denser pair has the same."""
    return scans(REF_AZ)[3], scans(REF_AZ)[2]


_REFERENCE = []


def reference(oracle):
    """-> (xyz1 (2026, 4), normals (2026, 3)) float32, computed once on the CPU."""
    if not _REFERENCE:
        rf, rn = oracle.sampling_surface_normal(scans(REF_AZ)[0], 10, 0.5, 4)
        rf.setflags(write=False)
        rn.setflags(write=False)
        _REFERENCE.append((rf, rn))
    return _REFERENCE[0]


def reading(n, n_az=RD_AZ):
    rd = scans(n_az)[1]
    assert n <= len(rd), (n, len(rd))
    assert np.array_equal(scans(n_az)[3], poses()[0]) and np.array_equal(scans(n_az)[2], poses()[1])
    return np.ascontiguousarray(rd[np.linspace(0, len(rd) - 1, n).astype(np.int64)])


def worker_az(n):
    """The scan a worker case is cut from: the default-grid cases' wherever that is large enough (the same reading, so the
    two block counts can be compared), the denser one above."""
    return RD_AZ if n <= len(scans(RD_AZ)[1]) else WORKER_AZ


def reference_mean(ref):
    """The mean lsgpu_icp_set_reference and the oracle centre the reference on: the double sum, rounded to float."""
    return (ref[:, :3].astype(np.float64).sum(0) / len(ref)).astype(np.float32)


_ORACLE_RUNS = {}


def oracle_run(oracle, n, n_az=RD_AZ):
    """The CPU oracle's alignment of the reading of n points, computed once -> dict(rc, T 4x4, iterations, converged, trace)."""
    if (n, n_az) not in _ORACLE_RUNS:
        rf, rn = reference(oracle)
        rc, To, st, tr = oracle.icp_compute(oracle.config_yaml(accum_double=1, num_threads=16), reading(n, n_az), rf, rn,
                                            synth.colmajor(poses()[0]), 64)
        _ORACLE_RUNS[(n, n_az)] = dict(rc=rc, T=synth.from_colmajor(To), iterations=st.iterations, converged=st.converged,
                                       trace=tr)
    return _ORACLE_RUNS[(n, n_az)]


# ------------------------------------------------------------------------------------------------ the model
def bits(x):
    return int(np.float32(x).view(np.uint32))


def plane_terms(p, q, n):
    """Per pair the 29 terms of the point-to-plane sums, as k_normal_eq / k_normal_eq_loop form them.  p, q, n: (m, 3)
    float32 -> (m, 29) float64."""
    p, q, n = (np.asarray(a, np.float32) for a in (p, q, n))
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    J = np.stack([py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz], 1)
    assert J.dtype == np.float32
    r = (px - q[:, 0]) * nx + (py - q[:, 1]) * ny + (pz - q[:, 2]) * nz
    assert r.dtype == np.float32
    Jd, rd = J.astype(np.float64), r.astype(np.float64)
    t = np.empty((len(p), 29))
    k = 0
    for a in range(6):
        for c in range(a, 6):
            t[:, k] = Jd[:, a] * Jd[:, c]
            k += 1
    for a in range(6):
        t[:, 21 + a] = -(Jd[:, a] * rd)
    t[:, 27] = 1.0
    t[:, 28] = rd * rd
    return t


def point_terms(p, q):
    """Per pair the 29 terms of the point-to-point sums (p2p_terms): p, q, q p^T row major, 12 zeros, 1, |p - q|^2 with the
    difference in float32 and (e0 e0 + e1 e1) + e2 e2 in float64."""
    p, q = (np.asarray(a, np.float32) for a in (p, q))
    e = (p - q).astype(np.float64)
    pd, qd = p.astype(np.float64), q.astype(np.float64)
    t = np.zeros((len(p), 29))
    t[:, 0:3], t[:, 3:6] = pd, qd
    for a in range(3):
        for c in range(3):
            t[:, 6 + 3 * a + c] = qd[:, a] * pd[:, c]
    t[:, 27] = 1.0
    t[:, 28] = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return t


_WIDE = np.finfo(np.longdouble).nmant >= 63


def exact_sums(terms):
    """-> (sum, sum |term|) per slot, float64 of the extended-precision sums."""
    cols = np.ascontiguousarray(terms.T)
    if _WIDE:
        wide = cols.astype(np.longdouble)
        return wide.sum(1).astype(np.float64), np.abs(wide).sum(1).astype(np.float64)
    return (np.array([math.fsum(c) for c in cols]), np.array([math.fsum(np.abs(c)) for c in cols]))


def unpack(sums):
    """29 sums -> (A 6x6 symmetric, b 6)."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    return A + np.triu(A, 1).T, np.asarray(sums[21:27]).copy()


class Model:
    """One iteration of the point-to-plane, 1-NN, trimmed loop from a pose, and the stand-alone sums of given matches."""

    def __init__(self, oracle, brute, ref, nrm, mean=None):
        self.oracle, self.brute = oracle, brute
        self.mean = reference_mean(ref) if mean is None else np.asarray(mean, np.float32)
        self.ref_c = ref.copy()
        self.ref_c[:, :3] = ref[:, :3] - self.mean
        self.nrm = np.asarray(nrm, np.float32)
        self.kd = oracle.KdTree(self.ref_c)

    def mean_frame_pose(self, T_init):
        T = np.asarray(T_init, np.float32).copy()
        T[:3, 3] = T[:3, 3] - self.mean
        return synth.colmajor(T)

    def moved(self, rd, T_init):
        """The reading as the loop holds it: under T_init with the reference mean taken off its translation."""
        return self.oracle.transform_points(self.mean_frame_pose(T_init), rd)

    def iteration(self, moved, T_prev16):
        """-> dict(limit, n_used, sums, mag, widen (29 each), ties): the sums of the pairs the trimmed limit keeps at the
        pose T_prev16 (column major, the T_iter before the iteration's update)."""
        p = self.oracle.transform_points(T_prev16, moved)
        ids, d2 = self.kd.nn(p, threads=16)
        two_i, two_d = self.brute(self.ref_c, p, 2)
        assert np.array_equal(two_d[:, 0], d2)                  # two independent exact searches agree
        m = len(d2)
        rank = min(m - 1, int(np.float32(m) * np.float32(RATIO)))   # the rank of test_trim_limit_exact
        limit = np.partition(d2, rank)[rank]
        keep = d2 <= limit
        q, n = self.ref_c[ids, :3], self.nrm[ids]
        sums, mag = exact_sums(plane_terms(p[keep, :3], q[keep], n[keep]))
        # a query whose two nearest reference points are equally far may be matched to either: the bar of every slot
        # is widened by the difference between the two candidates' terms
        tied = np.flatnonzero(keep & (two_d[:, 0] == two_d[:, 1]))
        widen = np.zeros(29)
        if 0 < len(tied) <= TIE_CAP:
            one = plane_terms(p[tied, :3], self.ref_c[two_i[tied, 0], :3], self.nrm[two_i[tied, 0]])
            other = plane_terms(p[tied, :3], self.ref_c[two_i[tied, 1], :3], self.nrm[two_i[tied, 1]])
            widen = np.abs(one - other).sum(0)
        return dict(limit=np.float32(limit), n_used=int(keep.sum()), sums=sums, mag=mag, widen=widen, ties=int(len(tied)))

    def check_trace(self, moved, trace):
        """Every iteration of a trace (the oracle's or the device's: T_iter, limit, n_used, A, b) against the model fed
        the trace's own pose before that iteration.  -> dict(worst_A, worst_b: the largest |trace - model| / sum |term|,
        ties: tied kept pairs over all iterations, failures: what missed, in words)."""
        worst_A = worst_b = 0.0
        ties, failures = 0, []
        eye = synth.colmajor(np.eye(4))
        iu = np.triu_indices(6)
        for k, t in enumerate(trace):
            m = self.iteration(moved, eye if k == 0 else trace[k - 1]["T_iter"])
            ties += m["ties"]
            if m["ties"] > TIE_CAP:
                failures.append(f"iteration {k}: {m['ties']} tied kept pairs, more than the cap of {TIE_CAP}")
            if bits(t["limit"]) != bits(m["limit"]):
                failures.append(f"iteration {k}: limit {t['limit']!r} for the model's {m['limit']!r}")
            if int(t["n_used"]) != m["n_used"]:
                failures.append(f"iteration {k}: n_used {t['n_used']} for the model's {m['n_used']}")
            A, b = np.asarray(t["A"], np.float64).reshape(6, 6), np.asarray(t["b"], np.float64)
            if not np.array_equal(A, A.T):
                failures.append(f"iteration {k}: A is not symmetric")
            got = np.concatenate([A[iu], b])
            err = np.abs(got - m["sums"][:27])
            bar = BAR * m["mag"][:27] + m["widen"][:27]
            ratio = err / np.where(m["mag"][:27] > 0, m["mag"][:27], 1.0)
            worst_A, worst_b = max(worst_A, float(ratio[:21].max())), max(worst_b, float(ratio[21:].max()))
            for s in np.flatnonzero(~(err <= bar)):
                failures.append(f"iteration {k}: slot {s} off by {err[s]:.3e}, bar {bar[s]:.3e} (ratio {ratio[s]:.3e})")
        return dict(worst_A=worst_A, worst_b=worst_b, ties=ties, failures=failures)

    def sums(self, query, T16, ids, d2, limit, p2p):
        """The stand-alone sums (lsgpu_normal_eq / lsgpu_point_to_point) of the pairs with an id, a finite distance and
        d2 <= limit -> (sums, mag, keep)."""
        p = self.oracle.transform_points(T16, query)
        with np.errstate(invalid="ignore"):
            keep = (ids >= 0) & np.isfinite(d2) & (d2 <= np.float32(limit))
        safe = np.where(ids >= 0, ids, 0)[keep]
        q = self.ref_c[safe, :3]
        terms = point_terms(p[keep, :3], q) if p2p else plane_terms(p[keep, :3], q, self.nrm[safe])
        s, mag = exact_sums(terms) if keep.any() else (np.zeros(29), np.zeros(29))
        return s, mag, keep


# ------------------------------------------------------------------------------------------------ a device case
def trace_bytes(trace):
    """What an alignment computed, iteration by iteration (the timing and search counters of a record left out)."""
    return b"".join(np.ascontiguousarray(t[key]).tobytes() for t in trace for key in ("T_iter", "A", "b", "x")) + \
        np.array([[bits(t["limit"]), t["n_used"]] for t in trace], np.int64).tobytes()


def device_case(oracle, model, h, n, n_az=RD_AZ):
    """Aligns the reading of n points twice on `h` (a point-to-plane, 1-NN handle whose reference is the model's) and
    checks it against the oracle and the model -> dict of plain facts (JSON-able); `failures` empty = everything held."""
    T_init = poses()[0]
    rd = reading(n, n_az)
    T, st = h.align(rd, T_init)
    tr = h.trace()
    T2, _st2 = h.align(rd, T_init)
    tr2 = h.trace()
    want = oracle_run(oracle, n, n_az)
    out = model.check_trace(model.moved(rd, T_init), tr)
    f = out["failures"]
    if T.tobytes() != T2.tobytes() or trace_bytes(tr) != trace_bytes(tr2):
        f.append("the second alignment of the same reading differs from the first")
    if want["rc"] != 0 or want["iterations"] <= 4:
        f.append(f"the oracle: rc {want['rc']}, {want['iterations']} iterations")
    if (st.iterations, st.converged) != (want["iterations"], want["converged"]) or len(tr) != st.iterations:
        f.append(f"{st.iterations} iterations, converged {st.converged}, {len(tr)} records; the oracle: "
                 f"{want['iterations']}, {want['converged']}")
    for k, (a, b) in enumerate(zip(tr, want["trace"])):
        if bits(a["limit"]) != bits(b["limit"]) or int(a["n_used"]) != int(b["n_used"]):
            f.append(f"iteration {k}: limit {a['limit']!r}, n_used {a['n_used']}; the oracle: {b['limit']!r}, {b['n_used']}")
    dt, dr = synth.pose_error(want["T"], T.astype(np.float64))
    if not (dt <= TOL_T and dr <= TOL_R):
        f.append(f"pose off the oracle's by {dt:.3e} m, {dr:.3e} rad")
    out.update(n=n, iterations=int(st.iterations), converged=int(st.converged), dt=dt, dr=dr,
               digest=hashlib.sha1(T.tobytes() + trace_bytes(tr)).hexdigest())
    return out
