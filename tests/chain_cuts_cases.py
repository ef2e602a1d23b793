"""What tests/test_chain_cuts.py shares between its cases, and (run as a program) the worker of its side-stream case.

The identity under test: lsgpu_icp_compute on a handle with lsgpu_icp_set_chain_cuts, given the RAW clouds (route a), equals
lsgpu_icp_compute on a handle without it, given the clouds the sequential chain -- lsgpu_apply_point_filters, one module after
the other -- leaves (route b): T_out, the iteration count, the trace records and the position of the library's draw stream,
bit for bit.

Route b for a reading section with modules BEHIND RandomSampling.  The issue that asked for these tests words route b as "the
clouds cut by apply_point_filters, with the reading's RandomSampling left to compute".  Taken literally that samples AFTER all
cut modules, which is another chain than [MinDist, RandomSampling, MaxDist, BoundingBox]: RandomSampling draws once per point
that reaches it, so moving it behind two more cuts pairs other draws with other points (on the case's pair the CPU oracle
converges after 7 iterations one way and 17 the other, 0.19 apart).  So route b runs the sequential chain with the module where
the document has it: the reference's draws first (lsgpu_icp_filter_reference on the cut reference with the chain seed, which
leaves the stream where compute's reference filter leaves it), then lsgpu_apply_point_filters on the reading with RandomSampling
as a type 5 module at its position (seed -1: it continues), then compute with the same seed, the cut clouds and NO reading
module -- its reference filter repeats the same draws.  The stream position of route b is the one behind the sequential
chain.  Where every cut module stands in front of RandomSampling the literal wording holds, and the tests use it as it is."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np

RS = "RandomSampling"     # the place of RandomSamplingDataPointsFilter in a list of reading modules

# the issue's case 2: modules as (type, dim, flag, v)
READING = [(2, -1, 0, [5.0]), RS, (1, -1, 0, [25.0]), (3, 0, 1, [-1, 1, -8, 8, -3, 3])]
REFERENCE = [(1, -1, 0, [30.0]), (2, -1, 0, [4.5]), (3, 0, 0, [-40, 40, -40, 40, -2.5, 2.5]), (6, 0, 0, [])]
SEED, PROB = 5, 0.5


def point_filters(mods, prob=PROB, cls=None):
    """[(type, dim, flag, v) | RS] -> a ctypes array of lsgpu_point_filter (RS: a type 5 module with `prob`)"""
    from laser_slam_amd import _lib
    cls = cls or _lib.PointFilter
    arr = (cls * len(mods))()
    for a, m in zip(arr, mods):
        typ, dim, flag, v = (5, 0, 0, [prob]) if m == RS else m
        a.type, a.dim, a.flag = typ, dim, flag
        for i, x in enumerate(v):
            a.v[i] = x
    return arr


def chain_cuts(reading, reference=()):
    """-> icp.ChainCuts of the cut modules of `reading` (RS marks where RandomSampling stands) and `reference`"""
    from laser_slam_amd import icp
    cut = [m for m in reading if m != RS]
    at = list(reading).index(RS) if RS in reading else len(cut)
    t = lambda ms: tuple((m[0], m[1], m[2], tuple(float(x) for x in m[3])) for m in ms)
    return icp.ChainCuts(t(cut), t(reference), at)


def stream_position():
    """A fingerprint of where the library's draw stream stands: which of its next 64 draws are below 0.5 (consumes them)"""
    from laser_slam_amd import icp
    return tuple(int(i) for i in icp.random_sampling(64, 0.5, seed=-1))


def trace_bytes(h):
    """The numerical record of lsgpu_icp_get_trace (the timings and the launch policy's counters are not results)"""
    out = b""
    for t in h.trace():
        out += np.ascontiguousarray(t["T_iter"]).tobytes() + np.float32(t["limit"]).tobytes() + np.int64(t["n_used"]).tobytes()
        out += np.ascontiguousarray(t["A"]).tobytes() + np.ascontiguousarray(t["b"]).tobytes() + np.ascontiguousarray(t["x"]).tobytes()
    return out


def sequential_reading(h, reading, rd, prob=PROB):
    """The reading behind the sequential chain on handle h (the stream continues); `left` = is RandomSampling left to compute?"""
    left = RS in reading and reading[-1] == RS
    mods = [m for m in reading if not (left and m == RS)]
    return (np.ascontiguousarray(h.apply_point_filters(point_filters(mods, prob), rd, seed=-1)) if mods else rd), left


def route_a(make_handle, reading, reference, rd, ref, T_init, prob=PROB, seed=SEED, **chain):
    """compute on the raw clouds, the cut modules on the handle -> (T bytes, iterations, trace bytes, stream position, handle stats)"""
    with make_handle() as h:
        h.set_chain_cuts(chain_cuts(reading, reference))
        T, st = h.compute(rd, ref, T_init, prob if RS in reading else -1.0, seed=seed, **chain)
        return T.tobytes(), int(st.iterations), trace_bytes(h), stream_position(), (int(st.final_n_used), h.info().n_reference)


def route_b(make_handle, reading, reference, rd, ref, T_init, prob=PROB, seed=SEED, **chain):
    """compute on the clouds the sequential chain leaves, no cut module on the handle (see the module's docstring)"""
    from laser_slam_amd import icp
    with make_handle() as h:
        ref_cut = np.ascontiguousarray(h.apply_point_filters(point_filters(reference), ref)) if reference else ref
        icp.random_sampling(0, 0.5, seed=seed)                       # the chain seed
        if chain.get("ssn_knn", 10) > 0:
            h.filter_reference(ref_cut, chain.get("ssn_knn", 10), chain.get("ssn_ratio", 0.5), seed=-1)   # the reference's draws
        rd_cut, left = sequential_reading(h, reading, rd, prob)
        if left:   # every cut module in front of RandomSampling: it is left to compute, as the issue words it
            T, st = h.compute(rd_cut, ref_cut, T_init, prob, seed=seed, **chain)
            pos = stream_position()
        else:
            pos = stream_position()                                  # behind the sequential chain
            T, st = h.compute(rd_cut, ref_cut, T_init, -1.0, seed=seed, **chain)
        return T.tobytes(), int(st.iterations), trace_bytes(h), pos, (int(st.final_n_used), h.info().n_reference), (len(rd_cut), len(ref_cut))


def main():
    """Both routes of case 2 in this process (started with LSGPU_NO_SIDE_STREAM=1: switches are read once) -> one JSON line"""
    from laser_slam_amd import icp, synth
    ref, rd, _T_true, T_init = synth.scan_pair(64)
    a = route_a(icp.IcpHandle, READING, REFERENCE, rd, ref, T_init)
    b = route_b(icp.IcpHandle, READING, REFERENCE, rd, ref, T_init)
    dg = lambda r: hashlib.sha256(r[0] + np.int64(r[1]).tobytes() + r[2] + repr(r[3]).encode()).hexdigest()
    print("CUTS_RESULT " + json.dumps({"a": dg(a), "b": dg(b), "iterations": a[1], "T": np.frombuffer(a[0], np.float32).tolist()}))


if __name__ == "__main__":
    main()
