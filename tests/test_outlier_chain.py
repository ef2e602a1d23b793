"""KDTreeMatcher maxDist and chains of Trimmed- / Max- / Min- / MedianDistOutlierFilter through every layer: both YAML
loaders, the four config fields, the launch policy, and on the GPU the bounded search (lsgpu_knn / lsgpu_knn_k) against
masked exact neighbours and the device loop against a test-side loop built from the oracle's primitives.

The contract (include/lsgpu_icp.h, "maxDist and outlier-filter chains"): a match is valid iff d2 <= maxDist^2 (else id -1,
d2 +inf); quantiles are taken over the valid matches; a pair is kept iff it passes every filter; the trace's limit is the
smallest upper threshold present, n_used counts kept pairs."""
import ctypes as C
import hashlib
import io
import os
import subprocess

import numpy as np
import pytest

from host_loop import d2_f32
from laser_slam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)

HEAD = ("readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
        "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n")
TAIL = ("errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
        "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n"
        "  - DifferentialTransformationChecker:\n      minDiffRotErr: 0.001\n      minDiffTransErr: 0.01\n"
        "      smoothLength: 4\n")
MODULE = {"trim": ("TrimmedDistOutlierFilter", "ratio"), "max": ("MaxDistOutlierFilter", "maxDist"),
          "min": ("MinDistOutlierFilter", "minDist"), "median": ("MedianDistOutlierFilter", "factor")}


def chain_yaml(filters, knn=1, max_dist=None, matcher_extra=""):
    """filters: [(key of MODULE, value or None for the module's default)], in the order given."""
    y = HEAD + f"matcher:\n  KDTreeMatcher:\n    knn: {knn}\n    epsilon: 0\n"
    if max_dist is not None:
        y += f"    maxDist: {max_dist}\n"
    y += matcher_extra
    if filters:
        y += "outlierFilters:\n"
        for key, v in filters:
            name, par = MODULE[key]
            y += f"  - {name}\n" if v is None else f"  - {name}:\n      {par}: {v}\n"
    return y + TAIL


# the chains the GPU tests run (pairs of synth: guess about 0.3 m / 1.5 deg off).  name -> config fields
CHAINS = {
    "matcher+trim": dict(trim=0.75, matcher=0.5),
    "max+trim": dict(trim=0.75, max=0.15),
    "min+trim": dict(trim=0.75, min=0.15),
    "median": dict(median=1.5),
    "all": dict(trim=0.9, matcher=0.5, max=0.45, min=0.1, median=2.0),
    "all64k": dict(trim=0.9, matcher=0.25, max=0.2, min=0.05, median=2.0),     # (the denser pair)
    # a maxDist above the k-best search's 1 m cap: a reading point with an invalid match searches the whole 3.25 m ball
    # again through the fallback in every iteration, and its list may come back partly empty (tests/test_knn_k_edges.py)
    "wide-matcher+trim": dict(trim=0.75, matcher=3.25),
}
WIDE = "wide-matcher+trim"


def _fields(ch):
    return dict(matcher_max_dist=ch.get("matcher", 0.0), outlier_max_dist=ch.get("max", 0.0),
                outlier_min_dist=ch.get("min", 0.0), outlier_median_factor=ch.get("median", 0.0))


# ------------------------------------------------------------------------------------------------ CPU: loaders, config

def test_python_loader_reads_the_chain():
    from laser_slam_amd import icp
    o = icp.ICP()
    vals = {"trim": 0.8, "max": 0.4, "min": 0.02, "median": 2.5}
    attr = {"trim": "trim_ratio", "max": "outlier_max_dist", "min": "outlier_min_dist", "median": "outlier_median_factor"}
    absent = {"trim": 1.0, "max": 0.0, "min": 0.0, "median": 0.0}
    for key in vals:                                             # each module alone
        o.load_from_yaml(io.StringIO(chain_yaml([(key, vals[key])])))
        for k2 in vals:
            assert getattr(o.chain, attr[k2]) == (vals[k2] if k2 == key else absent[k2]), (key, k2)
        assert o.chain.matcher_max_dist == 0.0
    o.load_from_yaml(io.StringIO(chain_yaml([(k, vals[k]) for k in ("trim", "max", "min", "median")])))
    a = o.chain
    o.load_from_yaml(io.StringIO(chain_yaml([(k, vals[k]) for k in ("median", "min", "trim", "max")])))
    assert a == o.chain and all(getattr(a, attr[k]) == vals[k] for k in vals)
    o.load_from_yaml(io.StringIO(chain_yaml([(k, None) for k in vals])))   # module defaults
    assert (o.chain.trim_ratio, o.chain.outlier_max_dist, o.chain.outlier_min_dist, o.chain.outlier_median_factor) == (0.85, 1.0, 1.0, 3.0)
    o.load_from_yaml(io.StringIO(chain_yaml([("trim", 0.75)], max_dist=0.5)))
    assert o.chain.matcher_max_dist == 0.5
    o.load_from_yaml(io.StringIO(chain_yaml([("trim", 0.75)], max_dist="inf")))
    assert o.chain.matcher_max_dist == 0.0
    o.load_from_yaml(io.StringIO(chain_yaml([])))
    assert o.chain.trim_ratio == 1.0 and o.chain.matcher_max_dist == 0.0
    # YAML floats with a leading dot are plain floats; .inf is infinity (absent for the two maxDist)
    o.load_from_yaml(io.StringIO(chain_yaml([("trim", ".85"), ("min", ".05"), ("median", ".5"), ("max", ".25")], max_dist=".5")))
    assert (o.chain.matcher_max_dist, o.chain.trim_ratio, o.chain.outlier_min_dist, o.chain.outlier_median_factor,
            o.chain.outlier_max_dist) == (0.5, 0.85, 0.05, 0.5, 0.25)
    for inf in (".inf", ".Inf", ".INF", "+.inf", "inf"):
        o.load_from_yaml(io.StringIO(chain_yaml([("max", inf)], max_dist=inf)))
        assert o.chain.matcher_max_dist == 0.0 and o.chain.outlier_max_dist == 0.0, inf
    bad = [(chain_yaml([("max", 0.4), ("max", 0.5)]), "MaxDistOutlierFilter"),
           (chain_yaml([("min", 0.1), ("trim", 0.7), ("min", 0.1)]), "MinDistOutlierFilter"),
           (chain_yaml([("median", 2), ("median", 2)]), "MedianDistOutlierFilter"),
           (chain_yaml([("trim", 0.7), ("trim", 0.7)]), "TrimmedDistOutlierFilter"),
           (chain_yaml([("max", "0.4\n      ratio: 0.5")]), "MaxDistOutlierFilter"),
           (chain_yaml([("median", "2\n      maxDist: 0.5")]), "MedianDistOutlierFilter"),
           (chain_yaml([("max", 0)]), "MaxDistOutlierFilter"),
           (chain_yaml([("median", -1)]), "MedianDistOutlierFilter"),
           (chain_yaml([("min", -1)]), "MinDistOutlierFilter"),
           (chain_yaml([("trim", 0.7)], max_dist=0), "KDTreeMatcher"),
           (chain_yaml([("trim", 0.7)], max_dist=-1), "KDTreeMatcher"),
           (chain_yaml([("trim", 0.7)], max_dist="-.inf"), "KDTreeMatcher"),
           (chain_yaml([("max", "-.inf")]), "MaxDistOutlierFilter"),
           (chain_yaml([("min", ".inf")]), "MinDistOutlierFilter"),
           (chain_yaml([("median", ".inf")]), "MedianDistOutlierFilter")]
    for y, module in bad:
        with pytest.raises(_lib.LsgpuError) as e:
            o.load_from_yaml(io.StringIO(y))
        assert e.value.code == _lib.BAD_CONFIG and module in str(e.value), (y, str(e.value))
    with pytest.raises(_lib.LsgpuError) as e:                    # refused for the modules it lacks
        o.load_from_yaml("outlierFilters:\n  - MaxDistOutlierFilter\n")
    assert "required" in str(e.value)
    c = icp.ChainConfig()
    assert (c.matcher_max_dist, c.outlier_max_dist, c.outlier_min_dist, c.outlier_median_factor) == (0, 0, 0, 0)


def _build_cpp(tmp_path, name, link=True):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "laser_slam_amd", "cpp", "include"),
           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe]
    if link:
        cmd += ["-L", os.path.join(ROOT, "laser_slam_amd"), "-llsgpu_icp", "-Wl,-rpath," + os.path.join(ROOT, "laser_slam_amd")]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and name + ": ok" in r.stdout, r.stdout + r.stderr


def test_cpp_loader_reads_the_chain(tmp_path):
    _build_cpp(tmp_path, "chain_loader_check")


def test_chain_policy(tmp_path):
    _build_cpp(tmp_path, "chain_policy_check", link=False)


def test_chain_fields_keep_the_config_layout():
    K = _lib.IcpConfig
    c = K()
    assert C.sizeof(c) == 7 * 4 + 8 * 4                        # the struct did not grow
    names = ["trim_ratio", "max_iterations", "min_diff_rot", "min_diff_trans", "smooth_length", "cell_size",
             "profile_kernels", "reserved", "error_minimizer", "matcher_knn", "matcher_max_dist", "outlier_max_dist",
             "outlier_min_dist", "outlier_median_factor", "reserved_"]
    assert [getattr(K, n).offset for n in names] == [4 * i for i in range(15)]
    for preset in (_lib.lib().lsgpu_icp_config_yaml, _lib.lib().lsgpu_icp_config_default):
        preset(C.byref(c))
        assert all(getattr(c, n) == 0 for n in names[10:14])
    for n in names[10:14]:
        for v in (-1.0, float("nan"), -0.5):
            _lib.lib().lsgpu_icp_config_yaml(C.byref(c))
            setattr(c, n, v)
            h = C.c_void_p()
            assert _lib.lib().lsgpu_icp_create(C.byref(c), 0, C.byref(h)) == _lib.BAD_CONFIG, (n, v)
    for n in names[12:14]:                                       # +inf where it has no meaning
        _lib.lib().lsgpu_icp_config_yaml(C.byref(c))
        setattr(c, n, float("inf"))
        h = C.c_void_p()
        assert _lib.lib().lsgpu_icp_create(C.byref(c), 0, C.byref(h)) == _lib.BAD_CONFIG


# ------------------------------------------------------------------------------------------------ the test-side loop

@pytest.fixture(scope="module")
def brute(tmp_path_factory):
    """knn_brute (tests/cpp/knn_brute.c): exact k-NN in the device's arithmetic, 16 threads at most."""
    so = str(tmp_path_factory.mktemp("knn_brute") / "libknn_brute.so")
    subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "knn_brute.c"), "-o", so, "-lm"])
    L = C.CDLL(so)
    L.knn_brute.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def knn(ref_xyz1, q_xyz1, k):
        r = np.ascontiguousarray(ref_xyz1, np.float32)
        q = np.ascontiguousarray(q_xyz1, np.float32)
        ids = np.empty((len(q), k), np.int32)
        d2 = np.empty((len(q), k), np.float32)
        assert L.knn_brute(r.ctypes.data, len(r), q.ctypes.data, len(q), k, 16, ids.ctypes.data, d2.ctypes.data) == 0
        return ids, d2
    return knn


def _mul4(a, b):
    """a @ b in float32 with the operation order of hostmath::mul4 / the oracle's mat4_mul (4x4, row-major numpy)."""
    s = a[:, 0:1] * b[0:1, :]
    s = s + a[:, 1:2] * b[1:2, :]
    s = s + a[:, 2:3] * b[2:3, :]
    s = s + a[:, 3:4] * b[3:4, :]
    return s.astype(np.float32)


def _p2p_sums(p, q):
    pd, qd = p.astype(np.float64), q.astype(np.float64)
    e = (p - q).astype(np.float64)
    s = np.zeros(29)
    s[0:3] = pd.sum(0)
    s[3:6] = qd.sum(0)
    s[6:15] = np.einsum("na,nc->ac", qd, pd).ravel()
    s[27] = len(p)
    s[28] = (e * e).sum()
    return s


def _sq(v):
    return np.float32(np.float32(v) * np.float32(v))             # one float multiply


def mask_matches(ids, d2, max_dist):
    """KDTreeMatcher maxDist: a match is valid iff d2 <= maxDist^2; invalid: id -1, d2 +inf (in place on copies)."""
    ids, d2 = ids.copy(), d2.copy()
    if max_dist:
        out = ~(d2 <= _sq(max_dist))
        ids[out] = -1
        d2[out] = INF
    return ids, d2


def host_chain_icp(oracle, nn, rd, ref, nrm, T_init, k, chain, p2p=False, mean=None):
    """ICP::compute steps 2-7 with a chain {trim, matcher, max, min, median}: exact neighbours (nn(ref, q, k) -> ids, d2 of
    shape N x k), mask beyond the matcher's maxDist, quantiles by lso_trim_limit over the valid matches, the smallest upper
    threshold, MinDist masked the same way, minimizer on the masked pairs, the oracle's checkers.
    -> (T, iterations, converged, [(limit, n_used)], per-iteration facts), or None at ("no_convergence", it)."""
    from laser_slam_amd import icp
    ratio, smooth, max_it, lim_rot, lim_trans = chain.get("trim", 1.0), 4, 40, 0.001, 0.01
    if mean is None:
        mean = np.add.accumulate(ref[:, :3].astype(np.float64), axis=0)[-1] / len(ref)
    mean = np.asarray(mean, np.float32)
    ref_c = ref.copy()
    ref_c[:, :3] = ref[:, :3] - mean
    T_rm_in = np.asarray(T_init, np.float32).copy()
    T_rm_in[:3, 3] = T_rm_in[:3, 3] - mean
    reading = oracle.transform_points(synth.colmajor(T_rm_in), rd)
    T_iter = np.eye(4, dtype=np.float32)
    hist, rot7 = [T_iter.copy()], [np.float32(0)]
    it, converged, trace, facts = 0, False, [], []
    while True:
        step = oracle.transform_points(synth.colmajor(T_iter), reading)
        ids, d2 = nn(ref_c, step, k)
        n_all = ids.size
        ids, d2 = mask_matches(ids, d2, chain.get("matcher"))
        idf, df = ids.ravel().copy(), d2.ravel().copy()          # Matches, k x N column major, flattened
        n_valid = int(np.isfinite(df).sum())
        rc, trim_lim = oracle.trim_limit(df, ratio)
        if rc != 0:
            return None, it
        uppers = {"trim": np.float32(trim_lim)}
        if chain.get("max"):
            uppers["max"] = _sq(chain["max"])
        if chain.get("median"):
            rc, med = oracle.trim_limit(df, 0.5)
            assert rc == 0
            uppers["median"] = np.float32(np.float32(chain["median"]) * np.float32(med))
        binding = min(uppers, key=lambda u: (uppers[u], u != "trim"))
        limit = uppers[binding]
        n_min = 0
        if chain.get("min"):
            low = np.isfinite(df) & (df < _sq(chain["min"]))
            n_min = int((low & (df <= limit)).sum())
            idf[low] = -1
            df[low] = INF
        pf = np.repeat(step, k, axis=0)                          # the reading point once per match
        if p2p:
            w = (df <= limit) & (idf >= 0)
            used = int(w.sum())
            if used == 0:
                return None, it
            dT = icp.point_to_point_solve(_p2p_sums(pf[w, :3], ref_c[idf[w], :3]))
        else:
            rc, _A, _b, _x, dT16, used = oracle.point_to_plane(pf, ref_c, nrm, idf, df, limit, 1)
            if rc != 0:
                return None, it
            dT = dT16.reshape(4, 4).T
        T_iter = _mul4(dT, T_iter)
        trace.append((np.float32(limit), int(used)))
        facts.append(dict(invalid=1.0 - n_valid / n_all, binding=binding, min_removed=n_min, valid=n_valid, used=int(used)))
        it += 1
        if it >= max_it:                              # CounterTransformationChecker
            break
        rot7.append(abs(np.float32(icp.rotation_distance(T_iter, hist[-1]))))
        hist.append(T_iter.copy())
        n = len(hist)
        if n > smooth:                                # DifferentialTransformationChecker (float, hostmath::checker_check)
            rot, trans = np.float32(0), np.float32(0)
            for i in range(n - 1, n - smooth - 1, -1):
                rot = np.float32(rot + rot7[i])
                dx, dy, dz = (hist[i][:3, 3] - hist[i - 1][:3, 3]).astype(np.float32)
                trans = np.float32(trans + abs(np.sqrt(np.float32(np.float32(dx * dx + dy * dy) + dz * dz))))
            rot = np.float32(rot / np.float32(smooth))
            trans = np.float32(trans / np.float32(smooth))
            if rot < np.float32(lim_rot) and trans < np.float32(lim_trans):
                converged = True
                break
    Tmean = np.eye(4, dtype=np.float32)
    Tmean[:3, 3] = mean
    return (_mul4(Tmean, _mul4(T_iter, T_rm_in)), it, converged, trace, facts), it


def _inputs(oracle, pair, seed=4):
    """reference filtered, reading sampled: what the device loop and the test-side loop are both handed."""
    rf, rn = oracle.sampling_surface_normal(pair["ref"], 10, 0.5, seed)
    keep = oracle.random_sampling(len(pair["rd"]), 0.5, -1)
    return rf, rn, pair["rd"][keep], pair["T_init"]


def test_reference_loop_without_new_fields_is_the_oracle_loop(oracle, brute, pair4k):
    rf, rn = oracle.sampling_surface_normal(pair4k["ref"], 10, 1.0, 0)
    rc, To, sto, tro = oracle.icp_compute(oracle.config_yaml(accum_double=1), pair4k["rd"], rf, rn,
                                          synth.colmajor(pair4k["T_init"]), 40)
    assert rc == 0
    (T, it, conv, tr, _f), _ = host_chain_icp(oracle, brute, pair4k["rd"], rf, rn, pair4k["T_init"], 1, dict(trim=0.75))
    assert (it, int(conv)) == (sto.iterations, sto.converged)
    assert tr == [(np.float32(t["limit"]), int(t["n_used"])) for t in tro]
    assert np.array_equal(T, synth.from_colmajor(To).astype(np.float32))


# (pair fixture, k, p2p, chain) of every device-loop case below
LOOP_CASES = [("pair4k", k, p2p, name) for name in CHAINS if name not in ("all64k", WIDE) for k in (1, 3) for p2p in (False, True)] + \
             [("pair64k", 1, False, "all64k"), ("pair4k", 4, False, WIDE), ("pair4k", 2, True, WIDE)]

_host_cache = {}


def _host(oracle, brute, request, case):
    if case not in _host_cache:
        pair_name, k, p2p, name = case
        rf, rn, rd, T_init = _inputs(oracle, request.getfixturevalue(pair_name))
        r, _ = host_chain_icp(oracle, brute, rd, rf, rn, T_init, k, CHAINS[name], p2p=p2p)
        t, _ = host_chain_icp(oracle, brute, rd, rf, rn, T_init, k, dict(trim=CHAINS[name].get("trim", 1.0)), p2p=p2p)
        _host_cache[case] = (r, t)
    return _host_cache[case]


BATCH_K, BATCH_CHAIN = 3, "all"


def _batch_pairs(oracle):
    """the four small pairs of the align_batch test: (filtered reference, normals, reading, guess)."""
    pairs = []
    for i, n_az in enumerate([96, 160, 64, 128]):
        ref, rd, _Tt, Ti = synth.scan_pair(n_az, noise_seeds=(3000 + i, 4000 + i), guess_seed=3000 + i)
        rf, rn = oracle.sampling_surface_normal(ref, 10, 0.5, i)
        pairs.append((rf, rn, rd, Ti))
    return pairs


def _check_not_vacuous(case, ch, r, t, binding):
    assert r is not None and t is not None, case
    _T, _it, _conv, trace, facts = r
    if ch is CHAINS[WIDE]:                                       # (3.25 m leaves the pair few invalid matches: some, in every iteration)
        assert all(0.0 < f["invalid"] <= 0.60 for f in facts), (case, [f["invalid"] for f in facts])
    elif ch.get("matcher"):
        assert 0.05 <= facts[0]["invalid"] <= 0.60, (case, facts[0]["invalid"])
    if ch.get("min"):
        assert facts[-1]["min_removed"] >= 0.01 * facts[-1]["valid"], (case, facts[-1])
    binding |= {f["binding"] for f in facts}
    plain = t[3]
    for i, rec in enumerate(trace):                              # differs from the Trimmed-only trace in every iteration
        assert i >= len(plain) or rec != plain[i], (case, i, rec)


def test_the_batch_pairs_are_not_vacuous(oracle, brute):
    """The same conditions for the pairs and the chain of the align_batch test."""
    ch = CHAINS[BATCH_CHAIN]
    for i, (rf, rn, rd, Ti) in enumerate(_batch_pairs(oracle)):
        r, _ = host_chain_icp(oracle, brute, rd, rf, rn, Ti, BATCH_K, ch)
        t, _ = host_chain_icp(oracle, brute, rd, rf, rn, Ti, BATCH_K, dict(trim=ch["trim"]))
        _check_not_vacuous(("batch", i), ch, r, t, set())


def test_the_tested_chains_are_not_vacuous(oracle, brute, request):
    """What keeps the GPU comparisons from passing with the new fields ignored (from the test-side loop, every case)."""
    binding = set()
    for case in LOOP_CASES:
        r, t = _host(oracle, brute, request, case)
        _check_not_vacuous(case, CHAINS[case[3]], r, t, binding)
    assert {"median", "trim"} <= binding, binding


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def icp_mod():
    from laser_slam_amd import icp
    return icp


def _check_knn_k(ids, d2, bids, bd2, ref_c, q):
    """Device k-NN against the masked exact k-NN of queries q in the centred reference ref_c: ascending (invalid last),
    d2 bit for bit, ids equal up to exact ties -- and a point the device names instead of the brute force's lies at exactly
    the distance reported for it (invalid entries, -1 / +inf, are invalid on both sides and never differ)."""
    assert (np.diff(np.where(np.isinf(d2), np.float32(3e38), d2), axis=1) >= 0).all()
    assert np.array_equal(d2, bd2)
    assert np.array_equal(ids < 0, np.isinf(d2)) and np.array_equal(bids < 0, ids < 0)
    ref_c, q = np.ascontiguousarray(ref_c, np.float32), np.ascontiguousarray(q, np.float32)
    jj, ss = np.nonzero(ids != bids)
    for j, s in zip(jj, ss):
        tied = (d2[j] == d2[j, s]).sum() >= 2 or d2[j, s] == d2[j][np.isfinite(d2[j])][-1] or d2[j, s] == d2[j, -1]
        assert tied, (j, s, ids[j], bids[j], d2[j])
    if jj.size:
        assert (ids[jj, ss] >= 0).all() and (ids[jj, ss] < len(ref_c)).all()
        at = d2_f32(q[jj, :3], ref_c[ids[jj, ss], :3])
        bad = np.flatnonzero(at.view(np.uint32) != d2[jj, ss].view(np.uint32))
        assert bad.size == 0, (jj[bad][:5], ss[bad][:5], ids[jj, ss][bad][:5], at[bad][:5], d2[jj, ss][bad][:5])
    srt = np.sort(np.where(ids < 0, -1 - np.arange(ids.shape[1], dtype=np.int32), ids), axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()


@pytest.mark.gpu
def test_knn_honours_matcher_max_dist(icp_mod, oracle, brute, pair4k):
    ref, rd = pair4k["ref"], pair4k["rd"]
    max_dist = 0.5
    # a reading point with no reference point in range, and one exactly at d2 == maxDist^2 from a reference point that
    # stands alone (3, 4, 12 scaled: |v| = 0.5 and its square 0.25 are exact in float; the reference is centred on a mean
    # taken from the handle, so the pair is placed after that mean is known)
    far_ref = np.float32([500.0, 500.0, 40.0, 1.0])
    ref2 = np.vstack([ref, far_ref[None]]).astype(np.float32)
    with icp_mod.IcpHandle(matcher_max_dist=max_dist) as h, icp_mod.IcpHandle() as h0:
        h.set_reference(ref2, None)
        h0.set_reference(ref2, None)
        mean = h.reference_mean()
        ref_c = ref2.copy()
        ref_c[:, :3] -= mean
        T = synth.colmajor(pair4k["T_init"]).copy()
        T[12:15] -= mean
        q = oracle.transform_points(T, rd)
        edge = ref_c[-1].copy()
        edge[:3] += np.float32([3.0, 4.0, 12.0]) * np.float32(0.5 / 13.0)
        lonely = np.float32([-300.0, 200.0, 90.0, 1.0])
        q = np.vstack([q, edge[None], lonely[None]]).astype(np.float32)
        _i, dd = brute(ref_c, q[-2:], 1)
        ident = np.eye(4, dtype=np.float32).T.ravel().copy()
        for k in (1, 3, 8):
            ids, d2 = h.knn_k(q, k, ident)
            bids, bd2 = mask_matches(*brute(ref_c, q, k), max_dist)
            _check_knn_k(ids, d2, bids, bd2, ref_c, q)
            assert ids[-1].max() == -1 and np.isinf(d2[-1]).all()                 # nothing in range
            if dd[0, 0] == _sq(max_dist):                                         # (the construction landed exactly on the edge)
                assert ids[-2, 0] == len(ref2) - 1 and d2[-2, 0] == _sq(max_dist)  # inclusive: valid
            inv = np.isinf(d2).mean()
            assert 0.02 < inv < 0.98, inv
        ids1, d21 = h.knn(q, ident)
        b1, bd1 = mask_matches(*brute(ref_c, q, 1), max_dist)
        _check_knn_k(ids1[:, None], d21[:, None], b1, bd1, ref_c, q)
        assert dd[0, 0] == _sq(max_dist), dd                                      # the edge case was really exercised
        # a handle without maxDist still returns every neighbour
        _i0, d0 = h0.knn(q, ident)
        assert np.isfinite(d0).all()


@pytest.mark.gpu
def test_trim_limit_skips_invalid_matches(icp_mod, oracle):
    rng = np.random.default_rng(5)
    with icp_mod.IcpHandle() as h:
        for n, share in ((1000, 0.3), (65537, 0.9), (7, 0.5), (300001, 0.01)):
            d2 = (rng.gamma(2.0, 0.01, n) ** 2).astype(np.float32)
            d2[rng.random(n) < share] = INF
            d2[0] = np.float32(0.01)
            for ratio in (0.75, 0.5, 1.0, 0.001):
                rc, want = oracle.trim_limit(d2, ratio)
                assert rc == 0 and np.float32(h.trim_limit(d2, ratio)) == np.float32(want), (n, ratio)
        with pytest.raises(_lib.ConvergenceError):
            h.trim_limit(np.full(100, INF, np.float32), 0.75)


def _device(icp_mod, rf, rn, rd, T_init, k, p2p, ch):
    mini = "PointToPointErrorMinimizer" if p2p else "PointToPlaneErrorMinimizer"
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.trim_ratio = ch.get("trim", 1.0)
    with icp_mod.IcpHandle(cfg, 0, mini, matcher_knn=k, **_fields(ch)) as h:
        h.set_reference(rf, None if p2p else rn)
        Tg, st = h.align(rd, T_init)
        trg = [(np.float32(t["limit"]), int(t["n_used"])) for t in h.trace()]
        mean = h.reference_mean()
    return Tg, st, trg, mean


def _compare(Tg, st, trg, host):
    Th, ith, convh, trh, _facts = host
    print("device", st.iterations, st.converged, trg)
    print("host  ", ith, int(convh), trh)
    assert (st.iterations, st.converged) == (ith, int(convh)), (st.iterations, st.converged, ith, convh)
    assert trg == trh
    assert st.final_n_used == trh[-1][1] and np.float32(st.final_limit) == trh[-1][0]
    dt, dr = synth.pose_error(Tg.astype(np.float64), Th.astype(np.float64))
    print("pose error", dt, dr)
    assert dt <= 1e-5 and dr <= 1e-6, (dt, dr)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LOOP_CASES, ids=lambda c: f"{c[0]}-k{c[1]}-{'p2p' if c[2] else 'p2plane'}-{c[3]}")
def test_device_loop_matches_reference_loop(icp_mod, oracle, brute, request, case):
    pair_name, k, p2p, name = case
    rf, rn, rd, T_init = _inputs(oracle, request.getfixturevalue(pair_name))
    Tg, st, trg, mean = _device(icp_mod, rf, rn, rd, T_init, k, p2p, CHAINS[name])
    host, _ = host_chain_icp(oracle, brute, rd, rf, rn, T_init, k, CHAINS[name], p2p=p2p, mean=mean)
    assert host is not None
    _compare(Tg, st, trg, host)


FULL_CHAIN = dict(trim=0.75, matcher=0.3, min=0.01)


def _kd_nn(oracle):
    def nn(ref_c, q, k):
        assert k == 1
        ids, d2 = oracle.KdTree(ref_c).nn(q, 16)
        return np.asarray(ids, np.int32)[:, None], np.asarray(d2, np.float32)[:, None]
    return nn


@pytest.mark.gpu
def test_device_loop_matches_reference_loop_full_size(icp_mod, oracle):
    ref, rd, _T_true, T_init = synth.scan_pair(16384)
    rf, rn, rdk, T_init = _inputs(oracle, dict(ref=ref, rd=rd, T_init=T_init), seed=5)
    Tg, st, trg, mean = _device(icp_mod, rf, rn, rdk, T_init, 1, False, FULL_CHAIN)
    host, _ = host_chain_icp(oracle, _kd_nn(oracle), rdk, rf, rn, T_init, 1, FULL_CHAIN, mean=mean)
    assert host is not None
    assert 0.05 <= host[4][0]["invalid"] <= 0.60 and host[4][-1]["min_removed"] >= 0.01 * host[4][-1]["valid"], (host[4][0], host[4][-1])
    _compare(Tg, st, trg, host)


def _digest(T, st, trace):
    hsh = hashlib.sha256()
    hsh.update(np.ascontiguousarray(T).tobytes())
    hsh.update(repr((st.iterations, st.converged, st.final_limit, st.final_n_used)).encode())
    for t in trace:
        hsh.update(np.float32(t["limit"]).tobytes() + np.int64(t["n_used"]).tobytes() + np.ascontiguousarray(t["T_iter"]).tobytes())
    return hsh.hexdigest()


@pytest.mark.gpu
def test_yaml_chain_through_compute_and_module_order(icp_mod, oracle, brute, pair64k):
    ref, rd, T_init = pair64k["ref"], pair64k["rd"], pair64k["T_init"]
    ch = CHAINS["all64k"]
    mods = [("trim", ch["trim"]), ("max", ch["max"]), ("min", ch["min"]), ("median", ch["median"])]
    digests, Ts = [], []
    for order in (mods, [mods[3], mods[2], mods[0], mods[1]]):
        o = icp_mod.ICP()
        o.load_from_yaml(io.StringIO(chain_yaml(order, knn=1, max_dist=ch["matcher"])))
        o.chain.seed = 4
        T = o.compute(rd, ref, T_init)
        digests.append(_digest(T, o.last_stats, o._handle.trace()))
        Ts.append((T, o.last_stats, [(np.float32(t["limit"]), int(t["n_used"])) for t in o._handle.trace()]))
    assert digests[0] == digests[1]
    # ... and the whole of ICP::compute (filters on the device, seed 4) is the reference loop on the oracle's filters
    rf, rn = oracle.sampling_surface_normal(ref, 10, 0.5, 4)
    keep = oracle.random_sampling(len(rd), 0.5, -1)
    host, _ = host_chain_icp(oracle, brute, rd[keep], rf, rn, T_init, 1, ch)
    T, st, tr = Ts[0]
    _compare(T, st, tr, host)


@pytest.mark.gpu
def test_align_batch_with_a_chain_is_sequential_align(icp_mod, oracle, brute):
    ch = CHAINS[BATCH_CHAIN]
    pairs = _batch_pairs(oracle)
    refs, nrms, rds, Tis = map(list, zip(*pairs))
    cfg = _lib.IcpConfig()
    _lib.lib().lsgpu_icp_config_yaml(C.byref(cfg))
    cfg.trim_ratio = ch["trim"]
    hs = [icp_mod.IcpHandle(cfg, matcher_knn=BATCH_K, **_fields(ch)) for _ in range(2)]
    Tb, stb, rcb = icp_mod.align_batch(hs, refs, nrms, rds, Tis)
    for h in hs:
        h.close()
    assert list(rcb) == [0] * len(pairs)
    with icp_mod.IcpHandle(cfg, matcher_knn=BATCH_K, **_fields(ch)) as h, icp_mod.IcpHandle(cfg, matcher_knn=3) as plain:
        for i, (rf, rn, rd, Ti) in enumerate(pairs):
            h.set_reference(rf, rn)
            T, st = h.align(rd, Ti)
            assert np.array_equal(T, Tb[i]) and st.iterations == stb[i].iterations and st.iterations > 1
            assert st.final_n_used == stb[i].final_n_used and st.final_limit == stb[i].final_limit
            # ... and both are the reference loop
            trg = [(np.float32(t["limit"]), int(t["n_used"])) for t in h.trace()]
            host, _ = host_chain_icp(oracle, brute, rd, rf, rn, Ti, BATCH_K, ch, mean=h.reference_mean())
            assert host is not None
            _compare(Tb[i], stb[i], trg, host)
            plain.set_reference(rf, rn)
            _Tp, stp = plain.align(rd, Ti)
            assert (stp.final_limit, stp.final_n_used) != (st.final_limit, st.final_n_used)


@pytest.mark.gpu
def test_nothing_within_max_dist_is_no_convergence(icp_mod, oracle, pair4k):
    rf, rn, rd, T_init = _inputs(oracle, pair4k)
    with icp_mod.IcpHandle(matcher_max_dist=1e-4) as h:
        h.set_reference(rf, rn)
        T_out = np.full(16, 7.0, np.float32)
        st = _lib.IcpStats()
        q = np.ascontiguousarray(rd, np.float32)
        Ti = np.ascontiguousarray(synth.colmajor(T_init), np.float32)
        rc = _lib.lib().lsgpu_icp_align(h._h, q.ctypes.data_as(C.POINTER(C.c_float)), len(q),
                                        Ti.ctypes.data_as(C.POINTER(C.c_float)), T_out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
        assert rc == _lib.NO_CONVERGENCE and np.array_equal(T_out, Ti)
        with pytest.raises(_lib.ConvergenceError):
            h.align(rd, T_init)
        ids, d2 = h.knn(rd, synth.colmajor(T_init))              # the handle works on the next call
        assert len(ids) == len(rd)
    with icp_mod.IcpHandle(matcher_max_dist=0.5) as h:
        h.set_reference(rf, rn)
        _T, st = h.align(rd, T_init)
        assert st.iterations > 1


@pytest.mark.gpu
def test_split_scan_refuses_a_chain_handle(icp_mod, pair4k):
    for f in ("matcher_max_dist", "outlier_max_dist", "outlier_min_dist", "outlier_median_factor"):
        with icp_mod.IcpHandle(**{f: 0.5}) as h:
            with pytest.raises(_lib.LsgpuError) as e:
                h.comm_init(0, 1, icp_mod.comm_unique_id())
            assert e.value.code == _lib.BAD_CONFIG and "split-scan" in str(e.value)
            h.set_reference(pair4k["ref"], None)                 # the handle stays usable on its own
            ids, _d2 = h.knn(pair4k["rd"])
            assert len(ids) == len(pair4k["rd"])
