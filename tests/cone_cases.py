"""Cases, normals and the CPU model of tests/test_direction_index.py (and its worker, tests/cone_worker.py).

The direction index (csrc/lsgpu_cone.hip.h: k_cone_keys / k_cone_gather / k_cone_rows build it, k_knn_cone searches it)
is exact through a chain of hand-derived bounds whose margins were simulated on the spinning-lidar pair only.  Every case
here is a well-conditioned base scene -- synth.scan_pair(64)'s reference scan, 4096 points, the sensor at the frame's origin
O -- plus a patch of points placed where one of those bounds is tight (the table in test_direction_index.py's docstring).

Normals: the geometric normal of the surface a point was generated on, tilted by 0.2-2 degrees about an axis in the tangent
plane, both drawn from a hash of the point's index: no two reference points share a normal, so a search that returns a
near-miss neighbour on the same surface patch changes the rows [p x n; n] of the normal equations (with the reference
filter's shared box normals it does not).

The CPU model (`Index`, `classify`) restates, in float32 numpy from the header's prose, the build's binning and the query
side's window arithmetic (devtools/sim_cone_f32.py is the precedent).  It classifies queries -- near-O, polar, wide, long
window, wrapping, served -- to prove on the CPU that a case reaches what it is for; it is not a second implementation to
trust and decides no assertion about the device's results.  numpy only (+ the oracle's primitives handed in by the caller).
"""
import numpy as np

from laser_slam_amd import synth

F = np.float32
ROWS, COLS = 128, 8192             # LSGPU_CONE_ROWS / LSGPU_CONE_COLS defaults (csrc/lsgpu_tuning.h)
MAX_WIN = 512                      # kConeMaxWin
GAP = 0.002                        # LSGPU_GAP default
CAP_FACTOR, CAP_MARGIN2 = 1.1, 1.05 * 1.05    # kCapFactor, kCapSearchMargin2
TRIM_YAML = 0.75                   # icp_default.yaml
TRIM_WIDE = 0.98                   # nearly every pair in the sums (no variant loses the index at it: test_direction_index)
RATIOS = (TRIM_YAML, TRIM_WIDE)
MIN_DIFF_ROT, MIN_DIFF_TRANS = 1e-5, 1e-4     # the checker of the existing index tests
T_OFF = synth.se3(0.2, 0.1, 0.0, yaw=np.deg2rad(1.5))
THIN_WAVE = 0.0002                 # thin_rows: amplitude [m at 30 m] of the waviness (see thin_rows_cloud)

N_CUTS = (1023, 1024, 1025, 1026, 1027)
TAILS = (63, 64, 65, 255, 257)
CASES = (["seam", "axes", "steep", "near_origin", "thin_rows", "dense_bin", "two_shells", "duplicates"]
         + [f"n{n}" for n in N_CUTS] + [f"tails{n}" for n in TAILS])
SERVED_CASES = ["seam", "axes", "two_shells", "duplicates"] + [f"n{n}" for n in N_CUTS[1:]] + [f"tails{n}" for n in TAILS]
BASE_ONLY = ["duplicates"] + [f"n{n}" for n in N_CUTS[1:]]      # nothing but beams of the base scan: rings in zeta

NEAR_O, POLAR, WIDE, LONG, WRAP, SERVED = range(6)
CLASS_NAMES = ("near-O", "polar", "wide", "long window", "wrapping", "served")
# case -> the class it is there for (at least 100 queries of it in one iteration >= 1, default bins)
INTENDED = {"seam": WRAP, "axes": SERVED, "steep": POLAR, "near_origin": NEAR_O, "thin_rows": SERVED, "dense_bin": LONG,
            "two_shells": SERVED, "duplicates": SERVED}


# ------------------------------------------------------------------------------------------------ normals

def _hash01(idx, salt):
    """Two uniforms in [0, 1) per point from its index (splitmix64 finaliser): the per-point seed of the tilt."""
    z = (np.asarray(idx, np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def tilt(normals, first_index=0):
    """Unit normals (n, 3) float64 -> float32: each rotated by 0.2-2 degrees about an axis of its tangent plane, angle and
    axis from the point's index; renormalised in float64, then rounded."""
    n = np.asarray(normals, np.float64)
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    idx = np.arange(len(n)) + first_index
    ang = np.deg2rad(0.2 + 1.8 * _hash01(idx, 1))
    phi = 2 * np.pi * _hash01(idx, 2)
    helper = np.where(np.abs(n[:, [2]]) < 0.9, [[0.0, 0.0, 1.0]], [[1.0, 0.0, 0.0]])
    t1 = np.cross(n, helper)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(n, t1)
    axis = t1 * np.cos(phi)[:, None] + t2 * np.sin(phi)[:, None]
    out = n * np.cos(ang)[:, None] + np.cross(axis, n) * np.sin(ang)[:, None]
    out /= np.linalg.norm(out, axis=1, keepdims=True)
    return out.astype(F)


def scene_normals(xyz_sensor, scene):
    """Geometric normal of the primitive of synth.Scene a return lies on (ground, street walls, box faces, cylinder
    sides): the nearest one -- a return is its ray's hit moved by 2 cm of range noise."""
    p = np.asarray(xyz_sensor, np.float64)[:, :3] + np.array([0.0, 0.0, synth.SENSOR_HEIGHT])
    n = len(p)
    best = np.abs(p[:, 2]).copy()
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1))

    def take(d, nn):
        m = d < best
        best[m] = d[m]
        nrm[m] = nn[m] if nn.ndim == 2 else nn

    for wy in (scene.wall_y, -scene.wall_y):
        out = np.maximum(np.maximum(-p[:, 2], p[:, 2] - scene.wall_h), 0.0)
        take(np.hypot(p[:, 1] - wy, out), np.array([0.0, 1.0, 0.0]))
    for lo, hi in zip(scene.box_lo, scene.box_hi):
        outside = np.maximum(np.maximum(lo - p, p - hi), 0.0)           # per axis, distance outside the slab
        for ax in range(3):
            others = [a for a in range(3) if a != ax]
            off = np.hypot(outside[:, others[0]], outside[:, others[1]])
            for face in (lo[ax], hi[ax]):
                e = np.zeros(3)
                e[ax] = 1.0
                take(np.hypot(p[:, ax] - face, off), e)
    for c, r, h in zip(scene.cyl_c, scene.cyl_r, scene.cyl_h):
        v = p[:, :2] - c
        rad = np.linalg.norm(v, axis=1)
        out = np.maximum(np.maximum(-p[:, 2], p[:, 2] - h), 0.0)
        nn = np.zeros((n, 3))
        nn[:, :2] = v / np.maximum(rad, 1e-12)[:, None]
        take(np.hypot(rad - r, out), nn)
    return nrm


# ------------------------------------------------------------------------------------------------ clouds

_cache = {}


def base_scene():
    """-> (xyz1 float32 (4096, 4), geometric normals float64)."""
    if "base" not in _cache:
        ref = synth.scan_pair(64)[0]
        _cache["base"] = (ref, scene_normals(ref, synth.Scene(1234)))
    return _cache["base"]


def _xyz1(xyz):
    out = np.ones((len(xyz), 4), F)
    out[:, :3] = np.asarray(xyz, np.float64).astype(F)
    return out


def _wall(rng, n, axis, at, lo, hi):
    """n points on the plane coordinate[axis] == at, the two other coordinates uniform in [lo, hi] (pairs, in axis order)."""
    p = np.empty((n, 3))
    p[:, axis] = at
    for k, a in enumerate([a for a in range(3) if a != axis]):
        p[:, a] = rng.uniform(lo[k], hi[k], n)
    e = np.zeros(3)
    e[axis] = 1.0
    return p, np.tile(e, (n, 1))


def thin_rows_cloud(rng, wave=THIN_WAVE, n=3000):
    """The one-elevation cloud of test_direction_index_on_clouds_it_is_not_made_for, 3000 points: z = -0.1 rho plus
    `wave` x sin(3 az) x rho / 30, and the surface's own normal.  rho starts at 1 m, not at 3 m as there: with 3 m the
    frame's origin lies more than a tenth of the z extent above the cloud's box, the handle builds no direction index
    (origin_inside) and the cloud never reaches k_knn_cone."""
    az = rng.uniform(0, 2 * np.pi, n)
    r = rng.uniform(1, 30, n)
    p = np.stack([r * np.cos(az), r * np.sin(az), -0.1 * r + wave * np.sin(3 * az) * r / 30], 1)
    # z = r g(az), g = -0.1 + wave sin(3 az) / 30:  dz/dr = g, dz/d(az) / r = g'
    g = -0.1 + wave * np.sin(3 * az) / 30
    dg = wave * 3 * np.cos(3 * az) / 30
    er = np.stack([np.cos(az), np.sin(az), np.zeros(n)], 1)
    ea = np.stack([-np.sin(az), np.cos(az), np.zeros(n)], 1)
    nrm = np.array([0.0, 0.0, 1.0]) - g[:, None] * er - dg[:, None] * ea
    return p, nrm


def _patch(name, rng):
    """-> (points (n, 3) float64, geometric normals) of the patch a case adds to the base scene."""
    if name == "seam":            # the wall x = 6 m across azimuth 0: pa exactly 0 (y = +-0), and 4 + t rounding to 4.0f
        p, nr = _wall(rng, 600, 0, 6.0, (-0.3, -1.0), (0.3, 1.0))
        p[0:50, 1] = 0.0
        p[50:100, 1] = -0.0
        p[100:150, 1] = -1e-9 * p[100:150, 0]
        return p, nr
    if name == "axes":            # the quadrant joins pa = 1, 2, 3
        parts = [_wall(rng, 300, 1, 5.0, (-0.3, -1.0), (0.3, 1.0)), _wall(rng, 300, 1, -5.0, (-0.3, -1.0), (0.3, 1.0)),
                 _wall(rng, 300, 0, -6.0, (-0.3, -1.0), (0.3, 1.0))]
        parts[0][0][:30, 0] = 0.0
        parts[1][0][:30, 0] = -0.0
        parts[2][0][:30, 1] = 0.0
        parts[2][0][30:60, 1] = -0.0
        return np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts])
    if name == "steep":           # above and beneath the sensor; one point on the polar axis itself
        top = _wall(rng, 1500, 2, 2.5, (-0.6, -0.6), (0.6, 0.6))
        bot = _wall(rng, 1500, 2, -1.7, (-0.6, -0.6), (0.6, 0.6))
        top[0][0, :2] = 0.0
        return np.concatenate([top[0], bot[0]]), np.concatenate([top[1], bot[1]])
    if name == "near_origin":     # a 5 cm ball around O, O itself among its points; "surface": the sphere through the point
        v = rng.normal(size=(300, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        p = v * (0.05 * rng.uniform(0, 1, 300) ** (1 / 3))[:, None]
        p[0] = 0.0
        return p, v
    if name == "dense_bin":       # 2500 points in a handful of bins, 40 m out
        return _wall(rng, 2500, 0, 40.0, (3.0, 0.0), (3.1, 0.1))
    if name == "two_shells":      # a wall with holes 5 m out and a second one 15 cm behind it
        front = _wall(rng, 1400, 0, 5.0, (1.0, -0.5), (2.0, 0.5))
        cell = (np.floor(front[0][:, 1] * 10).astype(np.int64) * 31 + np.floor(front[0][:, 2] * 10 + 100).astype(np.int64))
        keep = _hash01(cell, 7) >= 0.3                         # 30 % of the 10 cm squares are holes
        back = _wall(rng, 1000, 0, 5.15, (1.0, -0.5), (2.0, 0.5))
        return np.concatenate([front[0][keep], back[0]]), np.concatenate([front[1][keep], back[1]])
    raise KeyError(name)


def origin_inside(ref):
    """k_ref_stats_final's rule (test_grid_geometry.predict_geometry restates all of it): the frame's origin lies in the
    cloud's box widened by a tenth of its extent and a millimetre -- without that no direction index is built."""
    p = np.ascontiguousarray(ref, F)[:, :3]
    lo, hi = p.min(0), p.max(0)
    m = (F(0.1) * (hi - lo).astype(F)).astype(F) + F(1e-3)
    return bool(((lo - m).astype(F) <= 0).all() and ((hi + m).astype(F) >= 0).all())


def reading_of(cloud, T_off, rng):
    """test_grid_geometry._reading_of: the cloud itself, every second point, moved rigidly, plus 5 mm of noise; and the
    guess that goes with it."""
    rd = cloud[::2].copy()
    rd[:, :3] = (rd[:, :3].astype(np.float64) @ T_off[:3, :3].T + T_off[:3, 3] + rng.normal(0, 0.005, (rd.shape[0], 3))).astype(F)
    T_init = np.linalg.inv(T_off) @ synth.se3(0.03, 0.02, -0.01, yaw=np.deg2rad(0.4))
    return rd, T_init


def case(name):
    """-> dict(ref (n, 4) f32, nrm (n, 3) f32, rd (m, 4) f32, T_init 4x4 f64, patch: slice of the patch's points in ref)."""
    if name in _cache:
        return _cache[name]
    base, base_n = base_scene()
    rng = np.random.default_rng(1000 + CASES.index(name))
    c = dict(name=name)
    if name.startswith("tails"):
        s = case("seam")
        m = int(name[5:])
        c.update(ref=s["ref"], nrm=s["nrm"], T_init=s["T_init"], patch=s["patch"])
        c["rd"] = np.ascontiguousarray(s["rd"][(np.arange(m) * len(s["rd"])) // m])
    else:
        if name == "thin_rows":
            p, nr = thin_rows_cloud(rng)
            c["ref"], geo, c["patch"] = _xyz1(p), nr, slice(0, len(p))
        elif name == "duplicates":
            c["ref"], geo, c["patch"] = np.repeat(base, 2, axis=0), base_n, slice(0, 0)
        elif name[0] == "n" and name[1:].isdigit():
            idx = (np.arange(int(name[1:])) * len(base)) // int(name[1:])
            c["ref"], geo, c["patch"] = np.ascontiguousarray(base[idx]), base_n[idx], slice(0, 0)
        else:
            p, nr = _patch(name, rng)
            c["ref"] = np.concatenate([base, _xyz1(p)])
            geo = np.concatenate([base_n, nr])
            c["patch"] = slice(len(base), len(base) + len(p))
        c["nrm"] = tilt(geo)
        if name == "duplicates":
            c["nrm"] = np.repeat(c["nrm"], 2, axis=0)          # twins share one normal
        c["rd"], c["T_init"] = reading_of(c["ref"], T_OFF, rng)
    _cache[name] = c
    return c


# ------------------------------------------------------------------------------------------------ the oracle's loop

def oracle_config(oracle, ratio):
    return oracle.config_yaml(accum_double=1, min_diff_rot=MIN_DIFF_ROT, min_diff_trans=MIN_DIFF_TRANS, trim_ratio=ratio)


def oracle_run(oracle, name, ratio):
    """-> (rc, T 4x4 f64, stats, trace), once per case and ratio."""
    key = ("oracle", name, ratio)
    if key not in _cache:
        c = case(name)
        rc, To, sto, tro = oracle.icp_compute(oracle_config(oracle, ratio), c["rd"], c["ref"], c["nrm"],
                                              synth.colmajor(c["T_init"]), 40)
        _cache[key] = (rc, synth.from_colmajor(To), sto, tro)
    return _cache[key]


def mean_frame(c):
    """The loop's own coordinates (ICP::compute steps 2-5 as the oracle takes them): reference minus its mean, the
    reading under T_init in that frame.  -> (mean f32, ref_c (n, 4) f32, T_refMean_dataIn 16 column-major f32)."""
    ref = c["ref"]
    mean = (np.add.accumulate(ref[:, :3].astype(np.float64), axis=0)[-1] / len(ref)).astype(F)
    ref_c = ref.copy()
    ref_c[:, :3] = ref[:, :3] - mean
    T = np.asarray(c["T_init"], F).copy()
    T[:3, 3] = T[:3, 3] - mean
    return mean, ref_c, synth.colmajor(T)


def queries(oracle, c, trace, k):
    """The reading as iteration k of the oracle's loop searches it (mean frame, (m, 4) f32)."""
    _mean, _ref_c, T0 = mean_frame(c)
    reading = oracle.transform_points(T0, c["rd"])
    return reading if k == 0 else oracle.transform_points(trace[k - 1]["T_iter"], reading)


def pair_rows(p, q, n):
    """Rows J = [p x n; n] and residuals r = (p - q) . n of point-to-plane pairs as PointToPlaneErrorMinimizer forms them,
    in float32; returned as float64."""
    p, q, n = p[:, :3].astype(F), q[:, :3].astype(F), n.astype(F)
    J = np.empty((len(p), 6), F)
    J[:, 0] = p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1]
    J[:, 1] = p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2]
    J[:, 2] = p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]
    J[:, 3:] = n
    r = ((p[:, 0] - q[:, 0]) * n[:, 0] + (p[:, 1] - q[:, 1]) * n[:, 1] + (p[:, 2] - q[:, 2]) * n[:, 2]).astype(F)
    return J.astype(np.float64), r.astype(np.float64)


def sums64(p, ref_c, nrm, ids):
    """Normal equations of the pairs (p[i], ref_c[ids[i]]): products and sums in float64.
    -> (A 6x6, b 6, S 6): S[a] = sum |J[a] r|, the scale of b's rounding (near convergence b itself cancels)."""
    J, r = pair_rows(p, ref_c[ids], nrm[ids])
    return J.T @ J, -(J * r[:, None]).sum(0), np.abs(J * r[:, None]).sum(0)


def iteration_sums(oracle, brute, name, ratio, k):
    """Iteration k of the oracle's loop recomputed from brute-force matches: (inliers, A, b, S)."""
    key = ("sums", name, ratio, k)
    if key not in _cache:
        c = case(name)
        tro = oracle_run(oracle, name, ratio)[3]
        ids3, d3 = matches(oracle, brute, name, ratio, k)
        inl = np.flatnonzero(d3[:, 0] <= F(tro[k]["limit"]))
        _mean, ref_c, _T0 = mean_frame(c)
        q = queries(oracle, c, tro, k)
        _cache[key] = (inl,) + sums64(q[inl], ref_c, c["nrm"], ids3[inl, 0])
    return _cache[key]


TOL_A = 1e-9      # relative, Frobenius: the project's bar on the normal matrix
TOL_B = 1e-9      # per component, times S


def swap_sensitivity(oracle, brute, name, ratio, k, n_swaps=200):
    """What one wrong match does to iteration k's sums, in units of the bars the GPU comparison uses: for n_swaps sampled
    inliers the match is replaced by the query's second-nearest reference point (duplicates: the nearest that is not the
    match's twin); per swap max(|dA|_F / |A|_F / TOL_A, max_a |db_a| / (S_a TOL_B)).  -> array of those ratios."""
    c = case(name)
    tro = oracle_run(oracle, name, ratio)[3]
    ids3, _d3 = matches(oracle, brute, name, ratio, k)
    inl, A, _b, S = iteration_sums(oracle, brute, name, ratio, k)
    _mean, ref_c, _T0 = mean_frame(c)
    q = queries(oracle, c, tro, k)
    rng = np.random.default_rng(5 + k)
    pick = rng.choice(inl, min(n_swaps, len(inl)), replace=False)
    old = ids3[pick, 0]
    new = ids3[pick, 1]
    if name == "duplicates":
        new = np.where(new // 2 == old // 2, ids3[pick, 2], new)
        assert (new // 2 != old // 2).all()
    Jo, ro = pair_rows(q[pick], ref_c[old], c["nrm"][old])
    Jn, rn = pair_rows(q[pick], ref_c[new], c["nrm"][new])
    dA = np.einsum("na,nc->nac", Jn, Jn) - np.einsum("na,nc->nac", Jo, Jo)
    db = Jn * rn[:, None] - Jo * ro[:, None]
    ra = np.sqrt((dA * dA).sum((1, 2))) / np.linalg.norm(A) / TOL_A
    rb = (np.abs(db) / (S * TOL_B)).max(1)
    return np.maximum(ra, rb)


# ------------------------------------------------------------------------------------------------ the CPU model

def cone_dir(v):
    """cone_dir of lsgpu_cone.hip.h on rows of v = point - O, float32 (reciprocals correctly rounded here, 1 ulp on the
    device).  -> inv_rho, zeta, pa, rxy, inv_h"""
    with np.errstate(all="ignore"):
        vx, vy, vz = v[:, 0].astype(F), v[:, 1].astype(F), v[:, 2].astype(F)
        r2 = (vy * vy + vx * vx).astype(F)
        inv_rho = (F(1) / np.sqrt((vz * vz + r2).astype(F))).astype(F)
        rxy = np.sqrt(r2).astype(F)
        zeta = (vz * inv_rho).astype(F)
        inv_h = (F(1) / (np.abs(vx) + np.abs(vy)).astype(F)).astype(F)
        t = (vy * inv_h).astype(F)
        pa = np.where(vx >= 0, np.where(vy >= 0, t, F(4) + t), F(2) - t).astype(F)
    return inv_rho, zeta, pa, rxy, inv_h


def _clampu(t, hi):
    """cone_clampu: floor already applied; NaN -> 0."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(t), 0, np.clip(t, 0, hi)).astype(np.int64)


class Index:
    """The build: k_ref_stats' zeta range of the raw points, k_cone_keys' bins of the centred ones, k_cone_rows' records."""

    def __init__(self, ref, rows=ROWS, cols=COLS):
        raw = np.ascontiguousarray(ref, F)[:, :3]
        self.rows, self.cols = rows, cols
        with np.errstate(all="ignore"):
            r2 = (raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1] + raw[:, 2] * raw[:, 2]).astype(F)
            zraw = (raw[:, 2] / np.sqrt(r2)).astype(F)[r2 > 0]
        self.zeta_lo, self.zeta_hi = F(zraw.min()), F(zraw.max())
        self.mean = (np.add.accumulate(raw.astype(np.float64), axis=0)[-1] / len(raw)).astype(F)
        self.O = (-self.mean).astype(F)
        refc = (raw - self.mean).astype(F)
        zr = max(F(self.zeta_hi - self.zeta_lo), F(1e-3))
        self.z0 = F(self.zeta_lo - F(1e-5) - F(1e-4) * zr)
        self.rs = F(F(rows) / F(zr * F(1.0002) + F(2e-5)))
        self.cs = F(cols * 0.25)
        _ir, zeta, pa, _rxy, _ih = cone_dir((refc - self.O).astype(F))
        self.nan_zeta = int((~(np.abs(zeta) <= 1.5)).sum())           # the point that IS O
        self.nan_pa = int((~((pa >= 0) & (pa <= 4))).sum())           # points on the polar axis
        zeta = np.where(np.abs(zeta) <= 1.5, zeta, F(0)).astype(F)
        pa = np.where((pa >= 0) & (pa <= 4), pa, F(0)).astype(F)
        self.row = _clampu(np.floor(((zeta - self.z0) * self.rs).astype(F)), rows - 1)
        self.col = _clampu(np.floor((pa * self.cs).astype(F)), cols - 1)
        self.pa, self.zeta = pa, zeta
        self.rzmin = np.full(rows, np.inf, F)
        self.rzmax = np.full(rows, -np.inf, F)
        np.minimum.at(self.rzmin, self.row, zeta)
        np.maximum.at(self.rzmax, self.row, zeta)
        self.occupied = np.flatnonzero(self.rzmin <= self.rzmax)
        zm = np.maximum(np.abs(self.rzmin), np.abs(self.rzmax))
        with np.errstate(all="ignore"):
            cep = (np.sqrt(np.maximum(F(1) - zm * zm, F(0))).astype(F) * F(1.0 - 1e-5)).astype(F)
            self.rz_z = (F(1) / (F(4) * cep) * F(1.0 + 1e-6)).astype(F)
        self.row_cols = {int(r): np.sort(self.col[self.row == r]) for r in self.occupied}
        self.occupied_bins = len(np.unique(self.row * cols + self.col))

    def count(self, r, a0, a1):
        """points of row r in columns [a0, a1] (arrays)"""
        cs = self.row_cols[int(r)]
        return np.searchsorted(cs, a1, "right") - np.searchsorted(cs, a0, "left")


def classify(ix, q, ub, cap2s):
    """The searching lane of k_knn_cone<.., false> for every query q (mean frame, f32) whose warm-start point lies at
    squared distance ub: the class of what becomes of it (rows in ascending order as the kernel takes them; the first
    hand-off ends the lane's walk).  -> (classes int8, crosses: served / wrapping lanes one of whose windows spans a
    quadrant join pa = 1, 2, 3)."""
    n = len(q)
    E, A = ix.rows, ix.cols
    with np.errstate(all="ignore"):
        ub = np.asarray(ub, F)
        lim0 = np.minimum(((F(2 * GAP) * np.sqrt(ub)).astype(F) + ub).astype(F) + F(GAP * GAP), F(cap2s)).astype(F)
        R = (np.sqrt(lim0) * F(1 + 1e-5) + F(1e-7)).astype(F)
        inv_rho, zeta, pa, rxy, inv_h = cone_dir((q[:, :3] - ix.O).astype(F))
        s = (R * inv_rho * F(1 + 1e-5) + F(4e-6)).astype(F)
        ce = (rxy * inv_rho).astype(F)
        cone = (s <= 0.5) & (ce > 0) & (ce <= 1.5)
        alpha = (s * (F(1) + F(0.2) * s * s) + F(2e-6)).astype(F)
        alpha2 = (alpha * alpha).astype(F)
        dz = ((ce * s + np.abs(zeta) * s * s).astype(F) + F(2e-6)).astype(F)
        gq = ((rxy * inv_h) * (rxy * inv_h) * F(1 + 1e-6)).astype(F)
        inv_ce = ((F(1) / ce) * F(1 + 1e-6)).astype(F)
        r_lo = _clampu(np.floor(((zeta - dz - ix.z0) * ix.rs).astype(F)), E - 1)
        r_hi = _clampu(np.floor(((zeta + dz - ix.z0) * ix.rs).astype(F)), E - 1)
        cls = np.full(n, SERVED, np.int8)
        cls[~cone] = NEAR_O
        alive = cone.copy()
        wrapped = np.zeros(n, bool)
        crosses = np.zeros(n, bool)
        for r in ix.occupied:
            dzr = np.maximum(np.maximum(np.maximum(ix.rzmin[r] - zeta, zeta - ix.rzmax[r]), F(0)) - F(1e-6), F(0)).astype(F)
            m = alive & (r_lo <= r) & (r <= r_hi) & (dzr <= alpha)
            if not m.any():
                continue
            u2 = ((alpha2 - dzr * dzr).astype(F) * inv_ce * ix.rz_z[r]).astype(F)
            polar = m & ~(u2 <= 0.25)
            u = (np.sqrt(np.maximum(u2, F(0))) * F(1 + 1e-6)).astype(F)
            da = (F(2) * u * (F(1) + F(0.2) * u * u)).astype(F)
            dp = ((gq * da + F(1.42) * da * da).astype(F) + F(4e-6)).astype(F)
            clo = np.floor(((pa - dp) * ix.cs).astype(F))
            chi = np.floor(((pa + dp) * ix.cs).astype(F))
            clo = np.where(m & ~polar, clo, 0).astype(np.int64)
            chi = np.where(m & ~polar, chi, 0).astype(np.int64)
            wide = m & ~polar & (chi - clo >= (A >> 2))
            cls[polar] = POLAR
            cls[wide] = WIDE
            alive &= ~(polar | wide)
            m &= alive
            wraps = m & ((clo < 0) | (chi >= A))
            cnt = ix.count(r, np.maximum(clo, 0), np.minimum(chi, A - 1))
            wl = clo < 0
            cnt1 = ix.count(r, np.where(wl, clo + A, 0), np.where(wl, A - 1, chi - A))
            long_ = m & ((cnt > MAX_WIN) | (wraps & (cnt1 > MAX_WIN)))
            cls[long_] = LONG
            alive &= ~long_
            m &= alive
            wrapped |= m & wraps
            for join in (1.0, 2.0, 3.0):
                crosses |= m & ((pa - dp) < join) & ((pa + dp) >= join)
        cls[alive & wrapped] = WRAP
    return cls, crosses & alive


def model_iterations(oracle, brute, name, ratio, rows=ROWS, cols=COLS):
    """The model over the oracle's loop: for every iteration k >= 1, every reading point as a searching lane -- its
    warm-start point is its exact match of iteration k - 1, the cap 1.1 x that iteration's limit.
    -> (Index, [per iteration k >= 1: (classes, crosses)])."""
    key = ("model", name, ratio, rows, cols)
    if key in _cache:
        return _cache[key]
    c = case(name)
    _rc, _T, _st, tro = oracle_run(oracle, name, ratio)
    ikey = ("index", id(c["ref"]), rows, cols)
    if ikey not in _cache:
        _cache[ikey] = Index(c["ref"], rows, cols)
    ix = _cache[ikey]
    _mean, ref_c, _T0 = mean_frame(c)
    out = []
    prev = matches(oracle, brute, name, ratio, 0)[0][:, 0]
    for k in range(1, len(tro)):
        q = queries(oracle, c, tro, k)
        d = (q[:, :3] - ref_c[prev, :3]).astype(F)
        ub = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
        cap2s = F(F(F(tro[k - 1]["limit"]) * F(CAP_FACTOR)) * F(CAP_MARGIN2))
        out.append(classify(ix, q, ub, cap2s))
        prev = matches(oracle, brute, name, ratio, k)[0][:, 0]
    _cache[key] = (ix, out)
    return _cache[key]


def matches(oracle, brute, name, ratio, k):
    """Exact three nearest reference points (device arithmetic, tests/cpp/knn_brute.c) of iteration k's queries."""
    key = ("nn", name, ratio, k)
    if key not in _cache:
        c = case(name)
        _mean, ref_c, _T0 = mean_frame(c)
        _cache[key] = brute(ref_c, queries(oracle, c, oracle_run(oracle, name, ratio)[3], k), 3)
    return _cache[key]
