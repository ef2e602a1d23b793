"""What tests/test_module_rules.py and tests/cpp/modules_check.cpp share: the module variants, the handle configurations and the
order in which the rules of csrc/lsgpu_modules.h are asked.  tests/golden/module_rules_parent.json holds what the eight setters
and lsgpu_icp_comm_init of the library answered to drive() before the rule set existed (its "with_comm" part, which needs a live
communicator, is the rule function's own print, read against the setters' former `if (h->comm)` lines)."""
import ctypes as C

from laser_slam_amd import _lib

# the module variants that behave differently, in the fixture's order (tests/cpp/modules_check.cpp has the same table).
# "normals_knn_only" is what the issue names: normal_angle::check refuses it on every handle (reading normals that no outlier
# filter reads), so "normals_angle_knn" is here as well: the one variant behind which a module on the reading is accepted.
VARIANTS = ["robust", "normals_angle", "normals_knn_only", "normals_angle_knn", "covariance", "cuts", "max_density", "shadow_reading",
            "shadow_reference", "cov_sampling_reading", "cov_sampling_reference", "force2d", "force4dof", "bound_only"]
CONFIGS = ["plane_knn1", "point", "knn2", "chain_threshold"]
SETTER = {"robust": "lsgpu_icp_set_robust_filter", "normals": "lsgpu_icp_set_normals", "covariance": "lsgpu_icp_set_covariance",
          "cuts": "lsgpu_icp_set_chain_cuts", "max_density": "lsgpu_icp_set_max_density", "shadow": "lsgpu_icp_set_shadow",
          "cov_sampling": "lsgpu_icp_set_cov_sampling", "motion": "lsgpu_icp_set_motion"}
RESET_ORDER = ["shadow", "cov_sampling", "robust", "normals", "covariance", "cuts", "max_density", "motion"]   # never refused


def icp_config(name):
    L = _lib.lib()
    c = _lib.IcpConfig()
    L.lsgpu_icp_config_yaml(C.byref(c))
    if name == "point":
        c.error_minimizer = _lib.MINIMIZER_POINT_TO_POINT
    elif name == "knn2":
        c.matcher_knn = 2
    elif name == "chain_threshold":
        c.outlier_max_dist = 1.0
    return c


def variant(name):
    """(setter key, its config) of a variant."""
    L = _lib.lib()
    if name == "robust":
        c = _lib.RobustCfg()
        L.lsgpu_robust_config_default(C.byref(c))
        return "robust", c
    if name.startswith("normals"):
        c = _lib.NormalsCfg()
        L.lsgpu_normals_config_default(C.byref(c))
        if name == "normals_angle":
            c.max_angle, c.reading_normals_given = 0.5, 1
        elif name == "normals_knn_only":
            c.reading_sn_knn = 5
        else:
            c.max_angle, c.reading_sn_knn = 0.5, 5
        return "normals", c
    if name == "covariance":
        c = _lib.CovarianceCfg()
        L.lsgpu_covariance_config_default(C.byref(c))
        return "covariance", c
    if name == "cuts":
        c = _lib.ChainCuts()
        c.n_reading = 1
        c.reading[0].type, c.reading[0].dim = _lib.FILTER_MAX_DIST, -1
        c.reading[0].v[0] = 10.0
        return "cuts", c
    if name == "max_density":
        c = _lib.MaxDensityCfg()
        L.lsgpu_max_density_config_default(C.byref(c))
        return "max_density", c
    if name.startswith("shadow"):
        c = _lib.ShadowCfg()
        L.lsgpu_shadow_config_default(C.byref(c))
        c.reading_eps, c.reference_eps = (0.1, -1.0) if name == "shadow_reading" else (-1.0, 0.1)
        return "shadow", c
    if name.startswith("cov_sampling"):
        c = _lib.CovSamplingCfg()
        L.lsgpu_cov_sampling_config_default(C.byref(c))
        c.reading_nb_sample, c.reference_nb_sample = (100, 0) if name == "cov_sampling_reading" else (0, 100)
        return "cov_sampling", c
    c = _lib.MotionCfg()
    L.lsgpu_motion_config_default(C.byref(c))
    if name == "bound_only":
        c.bound = 1
    else:
        c.dof = _lib.MOTION_DOF_3 if name == "force2d" else _lib.MOTION_DOF_4
    return "motion", c


class Handle:
    """One handle of a configuration, its setters called raw: (return code, lsgpu_last_error) of every call."""

    def __init__(self, config):
        self.L = _lib.lib()
        self.config = config
        self.h = C.c_void_p()
        cfg = icp_config(config)
        rc = self.L.lsgpu_icp_create(C.byref(cfg), 0, C.byref(self.h))
        assert rc == _lib.OK, rc

    def close(self):
        self.L.lsgpu_icp_destroy(self.h)

    def _said(self, rc):
        return rc, self.L.lsgpu_last_error(self.h).decode()

    def set(self, name):
        key, cfg = variant(name)
        return self._said(getattr(self.L, SETTER[key])(self.h, C.byref(cfg)))

    def remove(self, key):
        return self._said(getattr(self.L, SETTER[key])(self.h, None))

    def reset(self):
        for key in RESET_ORDER:
            assert self.remove(key) == (_lib.OK, ""), key

    def comm_init(self):
        # (asked only of states that are refused in front of RCCL: the id is never read)
        return self._said(self.L.lsgpu_icp_comm_init(self.h, 0, 1, bytes(128)))


def drive(make_handle):
    """The recording: what every call answered, per configuration.
    pairs[i][j]: (first VARIANTS[i] set on an empty handle, then VARIANTS[j]); comm_init[i]: lsgpu_icp_comm_init behind
    VARIANTS[i] alone (None: not asked: nothing is on that is refused before a communicator would be opened); removals[m]:
    normals_angle_knn, m on the reading, lsgpu_icp_set_normals(NULL), normals_angle."""
    out = {}
    for config in CONFIGS:
        h = make_handle(config)
        try:
            pairs = []
            for a in VARIANTS:
                row = []
                for b in VARIANTS:
                    h.reset()
                    row.append((h.set(a), h.set(b)))
                pairs.append(row)
            comm = []
            for a in VARIANTS:
                h.reset()
                rc, _ = h.set(a)
                comm.append(h.comm_init() if rc == _lib.OK or config == "chain_threshold" else None)
            removals = {}
            for m in ("shadow_reading", "cov_sampling_reading"):
                h.reset()
                removals[m] = [h.set("normals_angle_knn"), h.set(m), h.remove("normals"), h.set("normals_angle")]
            h.reset()
            out[config] = dict(pairs=pairs, comm_init=comm, removals=removals)
        finally:
            h.close()
    return out


def encode(recording, texts):
    """The recording as the fixture keeps it: every (code, text) as the text's index in `texts` (0: "", LSGPU_OK), which grows."""
    def ix(said):
        if said is None:
            return -1
        rc, text = said
        assert (rc == _lib.OK) == (text == "") and rc in (_lib.OK, _lib.BAD_CONFIG), said
        if text not in texts:
            texts.append(text)
        return texts.index(text)
    out = {}
    for config, r in recording.items():
        out[config] = dict(pairs=[[[ix(a), ix(b)] for a, b in row] for row in r["pairs"]],
                           comm_init=[ix(c) for c in r["comm_init"]],
                           removals={m: [ix(s) for s in seq] for m, seq in r["removals"].items()})
    return out
