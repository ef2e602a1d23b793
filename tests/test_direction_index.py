"""The direction-index search (k_knn_cone, csrc/lsgpu_cone.hip.h) where its window bounds can go wrong.

The kernel has no kernel-level entry point: a test sees it through the trace of an align.  With the reference filter's
normals (one per box of ten points) a near-miss neighbour on the same surface patch leaves A unchanged; here every
reference point has its own normal (tests/cone_cases.py), every comparison reads b as well, and the CPU tests below prove
per case that ONE wrong match among the inliers moves A or b by more than ten times the bars the GPU comparison uses.

Cases (O = the reference frame's origin; base scene = synth.scan_pair(64)'s reference scan, 4096 points; the reading is
every second reference point, moved rigidly, 5 mm of noise; checker 1e-5 rad / 1e-4 m, at most 40 iterations; every case at
trim_ratio 0.75 (the YAML's) and 0.98 -- no forced variant loses the index at 0.98, so 0.98 it is):
  seam          600 points on the wall x = 6 m across azimuth 0, 50 each with y = +0, y = -0, y = -1e-9 x (4 + t == 4.0f)
  axes          wall patches across x = 0 at y = +-5 m and across y = 0 at x = -6 m, points exactly on the axes
  steep         ceiling z = 2.5 m and floor z = -1.7 m patches over / under the sensor (1500 points each), one point on the
                polar axis (a NaN pseudo-azimuth in the build)
  near_origin   300 points in a 5 cm ball around O, O itself among them (0 x inf in k_cone_keys / k_cone_rows)
  thin_rows     3000 points on z = -0.1 rho + 0.0002 sin(3 az) rho / 30, rho in [1, 30] m, and nothing else: zeta spans
                1.3e-5, the max(zr, 1e-3) floor holds, the cloud fills 2 of 128 rows (rows 10..23 of 1024).  The waviness is
                the smallest tried: the tilted normals alone keep the yaw observable, at amplitude 0 the loop behaves the
                same.  At 0.75 the oracle's loop runs its 40 iterations (the tightened checker never fires, at no amplitude
                up to 1.6 m: the trimmed set keeps flipping, 19 limits jump above the search cap and are repeated
                uncapped); at 0.98 it stops after 8.  rho starts at 1 m because at the 3 m of the existing disc the
                frame's origin lies outside the widened box: no index is built and the cloud never reaches k_knn_cone
  dense_bin     2500 points on a 10 cm x 10 cm wall patch 40 m out: windows longer than kConeMaxWin
  two_shells    a 1 m2 wall patch at 5 m with 30 % holes, a second wall 15 cm behind it
  duplicates    the base scene, every point twice (twins share one normal; A and b do not depend on which twin is matched,
                so the oracle comparison is the full one)
  n1023..n1027  the base scene cut to that many points: the build threshold (n1023 has no index), 3 / 0 / 1 / 2 pad slots
  tails63..257  seam with readings of 63, 64, 65, 255, 257 points

Variants, one child process each (tests/cone_worker.py; "forced" = LSGPU_CONE_MAX_OCC=1e9 LSGPU_CONE_HEAVY_SHARE=2
LSGPU_NO_INDEX_REST=1 LSGPU_CONE_FROM=1): V0 LSGPU_NO_CONE, V1 the product's policy, V2 forced, V3 forced without the
probe, V4-V7 forced with 8 x 64, 1024 x 65536, 1024 x 64, 8 x 65536 rows x columns.

Recorded on the CPU (model of tests/cone_cases.py, default 128 x 8192 bins: largest count of a class over the iterations >= 1
at 0.75; iterations of the oracle at 0.75 / 0.98; smallest swap ratio = min over both ratios, iteration 1 and the last, 200
sampled inliers, in units of the GPU comparison's bar -- the assertion asks for more than 10):
  case         near-O polar wide  long  wrap served  occupied rows  iterations  smallest swap ratio
  seam              0     0    0     0   163   2237  109             7 / 6      1.2e4
  axes              0     0    0     0    32   2469  114             7 / 6      6.1e3   (208 served lanes span a quadrant join)
  steep             0   476  125     0    55   3122   41             8 / 6      2.0e3   (8 x 64 bins: 828 polar, 522 wide)
  near_origin     115    19   30     0    42   2124  118             9 / 7      2.6e4
  thin_rows         0     0    0     0     1   1500    2            40 / 8      2.6e4
  dense_bin         0     0    0  1241    32   2056   65             7 / 6      1.4e3
  two_shells        0     0    0     0    32   2977   94             8 / 6      1.2e3
  duplicates        0     0    0     0    64   4040   64             7 / 6      1.5e4
  n1023             -     -    -     -     -      -    -             8 / 6      8.0e4
  n1024..n1027      0     0    0     0   8-9 505-507 16 (n1024), 64  6-12 / 6   4.8e4
  tails63..257      0     0    0     0  5-18 60-244  109             6-9 / 5-7  1.3e5
  1024 x 65536 bins: 960 of 1024 rows empty in duplicates and n1025..n1027, 1008 in n1024, 954 in dense_bin, both end rows
  occupied; patches that span z in [-1, 1] fill rows between the rings (empty: seam and two_shells 600, axes 494,
  near_origin 715, steep 880), thin_rows (1010 empty) leaves the end rows empty by design -- so the >= 900 check is made
  where the scan's rings are all there is.
Recorded on the MI355X (launches of the index / summed stragglers of its iterations / largest per iteration, at 0.75; V3 as
V2 within a few lanes; V0 and n1023 0 launches everywhere; every comparison bit for bit, V0 against the oracle A <= 5.2e-15,
b <= 5.1e-15 of its scale, pose equal):
  case         reading   V1 (policy)    V2 (forced)     V4 8x64        V5 1024x65536  V6 1024x64    V7 8x65536
  seam (0.98)   2348     5/0/0          6/0/0           5/0/0          6/0/0          6/0/0         5/0/0
  axes          2498     7/0/0          8/0/0           7/0/0          8/0/0          8/0/0         7/0/0
  steep         3548     8/822/157      9/2428/567      8/1775/340     9/528/143      9/462/79      9/5140/1325
  near_origin   2198     9/293/67       10/426/132      9/537/83       10/424/133     10/427/127    9/539/88
  thin_rows     1500     11/0/0         12/0/0          11/0/0         12/0/0         11/0/0        12/0/0     (19 repeats)
  dense_bin     3298     7/5811/1197    8/7066/1241     7/5989/1234    8/0/0          8/0/0         7/884/206
  two_shells    3005     0 (rested)     9/0/0           8/0/0          9/0/0          9/0/0         9/0/0
  duplicates    4096     0 (rested)     8/0/0           7/0/0          8/0/0          8/0/0         7/0/0
  n1024..n1027  512-514  5-17/0/0       6-18/0/0        6-18/0/0       6-18/0/0       6-18/0/0      6-18/0/0
  tails63..257  63-257   0-17/0/0       6-18/0/0        5-17/0/0       6-18/0/0       6-18/0/0      5-17/0/0
  (V1's handle rests the index from two_shells on, after dense_bin's timed searches; a launch count above the iteration
  count holds launches enqueued behind the end of the loop; with more than 3 points per occupied bin the index starts one
  iteration later.  dense_bin's 1241 is the CPU model's count to the lane, steep's 567 of 3548 its 17 %.  The file: 20 s.)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from laser_slam_amd import synth

import cone_cases as cc
import host_loop
from cone_cases import LONG, NEAR_O, POLAR, SERVED, WIDE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TOL_T, TOL_R = 1e-4, 1e-5        # test_gpu_parity's pose bars
TOL_A, TOL_B = cc.TOL_A, cc.TOL_B

FORCED = {"LSGPU_CONE_MAX_OCC": "1e9", "LSGPU_CONE_HEAVY_SHARE": "2", "LSGPU_NO_INDEX_REST": "1", "LSGPU_CONE_FROM": "1"}
VARIANTS = {
    "V0": {"LSGPU_NO_CONE": "1"},
    "V1": {},
    "V2": dict(FORCED),
    "V3": dict(FORCED, LSGPU_NO_CONE_PROBE="1"),
    "V4": dict(FORCED, LSGPU_CONE_ROWS="8", LSGPU_CONE_COLS="64"),
    "V5": dict(FORCED, LSGPU_CONE_ROWS="1024", LSGPU_CONE_COLS="65536"),
    "V6": dict(FORCED, LSGPU_CONE_ROWS="1024", LSGPU_CONE_COLS="64"),
    "V7": dict(FORCED, LSGPU_CONE_ROWS="8", LSGPU_CONE_COLS="65536"),
}
FORCED_VARIANTS = ["V2", "V3", "V4", "V5", "V6", "V7"]


@pytest.fixture(scope="module")
def brute(tmp_path_factory):
    return host_loop.build_brute(tmp_path_factory.mktemp("knn_brute"))


# ------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("name", cc.CASES)
def test_the_oracle_converges_on_every_case(oracle, name):
    """What keeps the comparisons from being vacuous, as test_the_oracle_converges_on_every_loop_case has it: the oracle's
    loop runs, for more than four iterations, at both ratios.  Every case but thin_rows at 0.75 also ends on the
    checker, not on the iteration count."""
    for ratio in cc.RATIOS:
        rc, _T, sto, tro = cc.oracle_run(oracle, name, ratio)
        assert rc == 0 and 4 < sto.iterations <= 40 and len(tro) == sto.iterations, (name, ratio, rc, sto.iterations)
        if (name, ratio) != ("thin_rows", cc.TRIM_YAML):
            assert sto.converged and sto.iterations < 40, (name, ratio, sto.iterations)


def test_cases_are_what_the_table_says():
    base, base_n = cc.base_scene()
    assert base.shape == (4096, 4) and np.allclose(np.linalg.norm(base_n, axis=1), 1.0)
    for name in cc.CASES:
        c = cc.case(name)
        n = c["nrm"].astype(np.float64)
        assert c["ref"].dtype == c["nrm"].dtype == c["rd"].dtype == F and len(c["ref"]) == len(c["nrm"])
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 2e-7, name
        if name != "duplicates":                                  # every reference point has a normal of its own
            assert len(np.unique(c["nrm"], axis=0)) == len(c["nrm"]), name
    # the tilt: 0.2 .. 2 degrees off the geometric normal
    s = cc.case("seam")
    ang = np.degrees(np.arccos(np.clip(np.abs(s["nrm"][s["patch"]].astype(np.float64)[:, 0]), 0, 1)))
    assert 0.19 < ang.min() and ang.max() < 2.01 and ang.max() - ang.min() > 1.5, (ang.min(), ang.max())
    p = s["ref"][s["patch"]]
    assert (p[:, 0] == 6).all() and (p[:50, 1] == 0).all() and not np.signbit(p[:50, 1]).any()
    assert (p[50:100, 1] == 0).all() and np.signbit(p[50:100, 1]).all()
    t = (p[100:150, 1] / (np.abs(p[100:150, 0]) + np.abs(p[100:150, 1]))).astype(F)
    assert (t < 0).all() and (F(4) + t == F(4)).all()             # the column clamp applies
    # ... and as the build sees them (centred point minus O, float32): pa exactly 0 in column 0 for the y = +-0 points,
    # pa exactly 4, clamped into the last column, for the y = -1e-9 x points
    ix = cc.Index(s["ref"])
    pa, col = ix.pa[s["patch"]], ix.col[s["patch"]]
    assert (pa[:100] == 0).all() and (col[:100] == 0).all() and (pa[100:150] == 4).all() and (col[100:150] == cc.COLS - 1).all()
    a = cc.case("axes")
    p = a["ref"][a["patch"]]
    assert (p[:, 0] == 0).sum() == 60 and (p[:, 1] == 0).sum() == 60
    pa = cc.Index(a["ref"]).pa[a["patch"]]                       # the quadrant joins themselves, and points on both sides
    for join, sl in ((1.0, slice(0, 300)), (3.0, slice(300, 600)), (2.0, slice(600, 900))):
        assert (pa[sl] == join).sum() >= 30 and (pa[sl] < join).sum() >= 50 and (pa[sl] > join).sum() >= 50, (join, pa[sl])
    st = cc.case("steep")
    p = st["ref"][st["patch"]]
    assert ((p[:, 0] == 0) & (p[:, 1] == 0)).sum() == 1 and set(np.unique(p[:, 2])) == {F(2.5), F(-1.7)}
    o = cc.case("near_origin")
    p = o["ref"][o["patch"]]
    assert len(p) == 300 and (p[0, :3] == 0).all() and np.linalg.norm(p[:, :3], axis=1).max() <= 0.05
    d = cc.case("dense_bin")
    p = d["ref"][d["patch"]]
    assert len(p) == 2500 and (p[:, 0] == 40).all() and np.ptp(p[:, 1]) <= 0.1 and np.ptp(p[:, 2]) <= 0.1
    w = cc.case("two_shells")
    p = w["ref"][w["patch"]]
    assert set(np.unique(p[:, 0])) == {F(5.0), F(5.15)} and 0.6 < (p[:, 0] == 5).sum() / 1400 < 0.8
    rd_x = (w["rd"][:, :3].astype(np.float64) - cc.T_OFF[:3, 3]) @ cc.T_OFF[:3, :3]     # the reading, moved back
    assert ((np.abs(rd_x[:, 0] - 5.0) < 0.03).sum() > 200) and ((np.abs(rd_x[:, 0] - 5.15) < 0.03).sum() > 200)
    du = cc.case("duplicates")
    assert np.array_equal(du["ref"][0::2], du["ref"][1::2]) and np.array_equal(du["nrm"][0::2], du["nrm"][1::2])
    for n in cc.N_CUTS:
        assert len(cc.case(f"n{n}")["ref"]) == n
    for n in cc.TAILS:
        assert len(cc.case(f"tails{n}")["rd"]) == n and cc.case(f"tails{n}")["ref"] is s["ref"]
    th = cc.case("thin_rows")
    ix = cc.Index(th["ref"])
    assert ix.zeta_hi - ix.zeta_lo < 1e-3 and len(ix.occupied) <= 2, (ix.zeta_hi - ix.zeta_lo, ix.occupied)
    assert all(cc.origin_inside(cc.case(name)["ref"]) for name in cc.CASES)      # or no index is built at all
    for name in cc.CASES:                                        # sizes: about 4-8 k reference points, the cuts apart
        if name[0] != "n" and name != "thin_rows":
            assert 4000 <= len(cc.case(name)["ref"]) <= 8192, name


def _counts(its):
    return np.array([np.bincount(cl, minlength=6) for cl, _cr in its])


@pytest.mark.parametrize("name", list(cc.INTENDED))
def test_each_case_reaches_its_class(oracle, brute, name):
    """At least 100 queries of the class the case is there for, in one iteration >= 1, under the default bins."""
    for ratio in cc.RATIOS:
        ix, its = cc.model_iterations(oracle, brute, name, ratio)
        cnt = _counts(its)
        print(name, ratio, "rows occupied", len(ix.occupied), "zeta span", ix.zeta_hi - ix.zeta_lo,
              "largest count per class", dict(zip(cc.CLASS_NAMES, cnt.max(0).tolist())))
        assert cnt[:, cc.INTENDED[name]].max() >= 100, (name, ratio, cnt.max(0))
        if name == "axes":          # ... of them, lanes whose window spans a quadrant join of the diamond angle
            assert max(int((cr & (cl == SERVED)).sum()) for cl, cr in its) >= 100
        if name == "near_origin":
            assert ix.nan_zeta == 1                              # O itself: 0 x inf in the build
        if name == "steep":
            assert ix.nan_pa == 1                                # the point on the polar axis
    if name == "steep":             # `wide` needs a quarter of the columns: reached under the 8 x 64 bins of V4
        _ix, its = cc.model_iterations(oracle, brute, name, cc.TRIM_YAML, 8, 64)
        assert _counts(its)[:, WIDE].max() >= 100 and _counts(its)[:, POLAR].max() >= 100


def test_the_largest_index_is_mostly_empty_rows():
    """V5, 1024 x 65536: at least 900 rows empty and both end rows occupied, wherever the cloud is nothing but the scan's
    rings (and in dense_bin, whose patch is a dot).  seam, axes, steep, near_origin, two_shells and thin_rows are
    deliberately outside this assertion: a patch that spans z in [-1, 1] fills the rows between the rings (494-880 rows
    stay empty) and thin_rows' zeta floor leaves the end rows empty; their counts stand in the module's docstring."""
    for name in cc.BASE_ONLY + ["dense_bin"]:
        ix = cc.Index(cc.case(name)["ref"], 1024, 65536)
        assert 1024 - len(ix.occupied) >= 900 and ix.occupied[0] == 0 and ix.occupied[-1] == 1023, (name, len(ix.occupied))


@pytest.mark.parametrize("name", cc.SERVED_CASES)
def test_cases_meant_to_be_served_are_served(oracle, brute, name):
    """At most 25 % of the queries fall back to the voxel grid, in every iteration >= 1, under the default bins (V2, V3)."""
    for ratio in cc.RATIOS:
        _ix, its = cc.model_iterations(oracle, brute, name, ratio)
        fb = _counts(its)[:, [NEAR_O, POLAR, WIDE, LONG]].sum(1) / len(cc.case(name)["rd"])
        assert fb.max() <= 0.25, (name, ratio, fb)


@pytest.mark.parametrize("name", cc.CASES)
def test_one_wrong_match_is_seen(oracle, brute, name):
    """The detector's sensitivity: at the oracle's iteration 1 and its last, A and b recomputed in float64 from brute-force
    matches (they ARE the oracle's: same inliers, A to 1e-12, b to 1e-12 of its scale); then one inlier's match replaced
    by the query's second-nearest point, for 200 sampled inliers: every single swap moves A or b by more than 10 x the
    GPU comparison's bar."""
    for ratio in cc.RATIOS:
        tro = cc.oracle_run(oracle, name, ratio)[3]
        for k in (1, len(tro) - 1):
            inl, A, b, S = cc.iteration_sums(oracle, brute, name, ratio, k)
            assert len(inl) == tro[k]["n_used"]
            assert np.linalg.norm(A - tro[k]["A"]) <= 1e-12 * np.linalg.norm(A)
            assert (np.abs(b - tro[k]["b"]) <= 1e-12 * S).all()
            r = cc.swap_sensitivity(oracle, brute, name, ratio, k)
            print(f"{name} ratio {ratio} iteration {k}: {len(r)} swaps, smallest change {r.min():.3g} x the bar, median {np.median(r):.3g}")
            assert len(r) == min(200, len(inl)) and r.min() > 10.0, (name, ratio, k, r.min())


# ------------------------------------------------------------------------------------------------ GPU

_runs = {}
_stopped = []      # (variant, why) of the one child that did not end well: nothing is started after it
# what a failed HIP call reads like: lsgpu_strerror(LSGPU_HIP_ERROR) and the HIPC detail, the runtime's and the driver's own
HIP_ERROR_TEXTS = ("HIP runtime error", "HIP error", "hipError", "illegal memory access", "unspecified launch failure",
                   "Memory access fault", "HSA_STATUS_ERROR")


def _stop(v, why):
    _stopped.append((v, why))
    pytest.fail(why)


def run_variant(v):
    """The child of variant v, once: {case: {ratio: run}}.  A child that does not end well -- its time limit, a signal, any
    exit status but 0 (134 and 139 among them, and the 1 of an LsgpuError that carries a failed HIP call), a HIP error
    text in its output, a missing result line -- fails the test that asked for it and is remembered: no child, of this
    variant or another, is started after it."""
    if v in _runs:
        return _runs[v]
    if _stopped:
        pytest.fail(f"no child is started after this one: {_stopped[0][1]}")
    env = {k: val for k, val in os.environ.items() if not k.startswith("LSGPU_") or k == "LSGPU_SO"}   # no switch but the variant's
    env.update(VARIANTS[v])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cone_worker.py")], env=env, capture_output=True,
                           text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        _stop(v, f"{v}: the child ran into its time limit; output so far: {str(e.stdout)[-1500:]}")
    text = r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CONE_RESULT ")]
    hip = [t for t in HIP_ERROR_TEXTS if t in text]
    if r.returncode != 0 or hip or len(lines) != len(cc.CASES):
        _stop(v, f"{v}: the child ended with status {r.returncode}, {len(lines)} of {len(cc.CASES)} result lines, HIP error "
                 f"texts {hip}: {r.stdout[-1500:]} {r.stderr[-1500:]}")
    out = {}
    for ln in lines:
        d = json.loads(ln[len("CONE_RESULT "):])
        out[d["case"]] = {float(k): run for k, run in d["runs"].items()}
    _runs[v] = out
    return out


def test_a_child_that_fails_is_the_last_one_started(monkeypatch):
    """run_variant on the CPU, with the child faked: an LsgpuError exit (status 1, the project's own text for a failed HIP
    call) is terminal, and neither that variant nor another starts a child afterwards."""
    import test_direction_index as me
    calls = []

    def fake_run(*a, **k):
        calls.append(k["env"].get("LSGPU_NO_CONE"))
        return subprocess.CompletedProcess(a, 1, "CONE_RESULT {}\n", "laser_slam_amd._lib.LsgpuError: HIP runtime error: "
                                           "lsgpu_icp.hip:1 hipStreamSynchronize(h->stream) -> unspecified launch failure")
    monkeypatch.setattr(me, "_runs", {})
    monkeypatch.setattr(me, "_stopped", [])
    monkeypatch.setattr(me.subprocess, "run", fake_run)
    for v in ("V0", "V0", "V2"):
        with pytest.raises(pytest.fail.Exception):
            me.run_variant(v)
    assert calls == ["1"] and me._stopped[0][0] == "V0" and not me._runs
    # a clean exit with a result line missing, or a HIP error text beside status 0, stops the file as well
    for out, err in (("", ""), ("\n".join("CONE_RESULT {}" for _ in cc.CASES), "HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION")):
        monkeypatch.setattr(me, "_stopped", [])
        monkeypatch.setattr(me.subprocess, "run", lambda *a, **k: subprocess.CompletedProcess(a, 0, out, err))
        with pytest.raises(pytest.fail.Exception):
            me.run_variant("V1")
        assert me._stopped and not me._runs


def _cap_repeats(run):
    """Iterations whose trim limit came out above the search cap -- 1.1 x the limit before (kCapFactor), float -- and
    were repeated uncapped on the voxel grid (csrc/lsgpu_solve.hip.h): in them every lane counts as a straggler, and
    they are not the index's."""
    lim = [_f32(h)[0] for h in run["limit"]]
    return [k for k in range(1, len(lim)) if not lim[k] <= F(lim[k - 1] * F(cc.CAP_FACTOR))]


def _f64(h):
    return np.frombuffer(bytes.fromhex(h), np.float64)


def _f32(h):
    return np.frombuffer(bytes.fromhex(h), np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.CASES)
def test_voxel_grid_run_matches_the_oracle(oracle, brute, name):
    """V0 against oracle.icp_compute (accum_double): equal iteration count; per iteration the limit bit for bit, the inlier
    count, A to 1e-9 relative Frobenius, b to 1e-9 of the sum of the absolute values of its terms (float64 recomputation);
    the pose within 1e-4 m / 1e-5 rad.  No launch of the index."""
    runs = run_variant("V0")[name]
    for ratio in cc.RATIOS:
        g = runs[ratio]
        rc, To, sto, tro = cc.oracle_run(oracle, name, ratio)
        assert rc == 0 and g["iterations"] == sto.iterations and g["iterations"] > 4, (name, ratio, g["iterations"], sto.iterations)
        assert g["launches"] == 0
        worst_a = worst_b = 0.0
        for k, t in enumerate(tro):
            assert _f32(g["limit"][k])[0] == F(t["limit"]), (name, ratio, k)
            assert g["n_used"][k] == t["n_used"], (name, ratio, k)
            _inl, _A, _b, S = cc.iteration_sums(oracle, brute, name, ratio, k)
            ea = np.linalg.norm(_f64(g["A"][k]).reshape(6, 6) - t["A"]) / np.linalg.norm(t["A"])
            eb = (np.abs(_f64(g["b"][k]) - t["b"]) / S).max()
            worst_a, worst_b = max(worst_a, ea), max(worst_b, eb)
            assert ea < TOL_A, (name, ratio, k, ea)
            assert eb <= TOL_B, (name, ratio, k, eb)
        dt, dr = synth.pose_error(To, _f32(g["T"]).reshape(4, 4).astype(np.float64))
        print(f"{name} ratio {ratio}: {g['iterations']} iterations, A off by {worst_a:.2e}, b by {worst_b:.2e} of its scale, "
              f"|dt| {dt:.2e} m, |dr| {dr:.2e} rad")
        assert dt <= TOL_T and dr <= TOL_R, (name, ratio, dt, dr)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [v for v in VARIANTS if v != "V0"])
def test_every_variant_returns_what_the_voxel_grid_returns(v):
    """DESIGN.md's claim about the switches on these geometries and the four extreme bin shapes: per case and ratio T, the
    iteration count and per iteration limit, n_used, A, b, T_iter are those of V0 bit for bit.  And the index really
    served: launches >= 1 in the forced variants wherever the reference has 1024 points, none without an index; lanes
    are handed to the voxel grid where the case is there for it, and not more than half of them where it is not."""
    base, got = run_variant("V0"), run_variant(v)
    for name in cc.CASES:
        nq = len(cc.case(name)["rd"])
        for ratio in cc.RATIOS:
            a, b = base[name][ratio], got[name][ratio]
            for key in ("T", "iterations", "limit", "n_used", "A", "b", "T_iter"):
                assert a[key] == b[key], (v, name, ratio, key)
            repeated = _cap_repeats(b)
            assert b["cap_retries"] == a["cap_retries"] == len(repeated), (v, name, ratio, b["cap_retries"], repeated)
            # (Follow-up: which iterations searched the index is re-derived here from the policy's rules; the policy may
            # also take an align off the index on a high straggler share, which no forced switch disables.  A per-iteration
            # "searched the index" word in the trace would be the robust source -- an ABI change, outside this file.)
            # the index's iterations: from LSGPU_CONE_FROM on (2 unless forced to 1; one later where the index holds more
            # than 3 points per occupied bin: csrc/lsgpu_policy.h, dense_wait), the uncapped repeats apart
            first = (1 if v in FORCED_VARIANTS else 2) + (1 if b["occupancy"] > 3.0 else 0)
            strag = [s for k, s in enumerate(b["stragglers"]) if k >= first and k not in repeated] or [0]
            print(f"{v} {name} ratio {ratio}: launches {b['launches']} of {b['iterations']} iterations ({len(repeated)} repeated "
                  f"uncapped), stragglers sum {sum(strag)} max {max(strag)} of {nq}, occupancy {b['occupancy']:.2f}, "
                  f"heavy share {b['heavy_share']:.3f}")
            if name == "n1023":
                assert b["launches"] == 0, (v, name, ratio)
            elif v in FORCED_VARIANTS:
                assert b["launches"] >= 1, (v, name, ratio)
                if v == "V2" and name in ("steep", "near_origin", "dense_bin"):
                    assert sum(strag) > 0, (v, name, ratio)
                if v in ("V2", "V3") and name in cc.SERVED_CASES:
                    assert max(strag) <= nq // 2, (v, name, ratio, strag)
    assert all(run["launches"] == 0 for runs in base.values() for run in runs.values())
