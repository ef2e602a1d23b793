// lsgpu_chain_loader.cpp -- lsgpu_chain_load: THE rule set of PointMatcher::ICP::loadFromYaml (laser_slam/src/laser_track.cpp:17)
// for the device path.  Host only, no HIP.  The C++ facade (cpp/include/laser_slam_amd/icp.hpp) and the Python facade
// (icp.py) parse the YAML syntax and hand the modules over as text; which modules exist, their parameters, defaults and
// ranges, what may be given once, the order inside the two filter sections and what the device loop cannot run without are
// decided here and nowhere else.
//
// A new module is one row of kRows and one handler.  The row gives the refusal of an unknown parameter, of a second
// instance and (by its absence) "is not implemented on the HIP path"; the handler reads the parameters with num() / whole()
// and writes the ABI structs.  What needs more than one module is checked in finish().
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <string>

#include "../../include/lsgpu_icp.h"
#include "lsgpu_normal_angle.h"
#include "lsgpu_robust.h"
#include "lsgpu_shadow.h"
#include "lsgpu_cov_sampling.h"
#include "lsgpu_modules.h"

namespace {

struct Refusal { std::string why; };
[[noreturn]] void refuse(const std::string& why) { throw Refusal{why}; }

const char* const kPair = " is implemented only as the pair ObservationDirectionDataPointsFilter, OrientNormalsDataPointsFilter "
                          "directly behind the module that produces the normals";
const char* const kOneReference = "referenceDataPointsFilters: one module at most (SamplingSurfaceNormalDataPointsFilter or "
                                  "SurfaceNormalDataPointsFilter)";
const char* const kSurfaceNormalParams = "knn epsilon maxDist keepNormals keepDensities keepEigenValues keepEigenVectors "
                                         "keepMatchedIds keepMeanDist sortEigen smoothNormals";

const char* const kDensitiesAlone = "referenceDataPointsFilters: SurfaceNormalDataPointsFilter: keepDensities 1 is implemented only with "
                                    "MaxDensityDataPointsFilter directly behind it (no other module reads the densities)";

const char* const kBoundingBoxParams = "xMin xMax yMin yMax zMin zMax removeInside";

bool listed(const char* list, const char* word) {   // is `word` one of the space-separated words of `list`?
  const size_t n = std::strlen(word);
  for (const char* p = list; *p;) {
    const char* e = std::strchr(p, ' ');
    const size_t len = e ? (size_t)(e - p) : std::strlen(p);
    if (len == n && std::strncmp(p, word, n) == 0) return true;
    p += len + (e ? 1 : 0);
  }
  return false;
}

struct Load {
  lsgpu_loaded_chain out;
  lsgpu_chain_cuts cuts;                  // the cut modules of the two filter sections (lsgpu_chain_load_cuts)
  const lsgpu_yaml_module* m = nullptr;   // the module being read
  // where a filter section has got to: 1 RandomSampling (reading) / the module that gives the normals (reference),
  // 2 SurfaceNormal on the reading, 3 ObservationDirection, 4 OrientNormals
  int stage[2] = {0, 0};
  bool matcher = false, minimizer = false, counter = false, robust = false, with_cov = false;
  bool ref_densities = false, max_density = false;   // the reference's SurfaceNormal has keepDensities 1; MaxDensity stands behind it
  lsgpu_shadow_config shadow;             // ShadowDataPointsFilter of the two sections (lsgpu_chain_load_shadow): beside stage[], not in it
  lsgpu_cov_sampling_config cov_sampling; // CovarianceSamplingDataPointsFilter of the two sections (lsgpu_chain_load_cov_sampling): likewise
  lsgpu_motion_config motion;             // force2D / force4DOF of PointToPlaneErrorMinimizer, BoundTransformationChecker (lsgpu_chain_load_motion)
  // lsgpu_chain_load_carried: the caller's clouds carry normals (LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE).
  // ref_module: the reference's section has a normals module of its own (stage[1] may also come from a carried pair)
  unsigned carried = 0;
  bool ref_module = false;

  std::string name() const { return m->name; }
  int side() const { return std::strcmp(m->section, "readingDataPointsFilters") == 0 ? 0 : 1; }
  const char* text(const char* key) const {   // (a key given twice: the last one, as in a map)
    const char* v = nullptr;
    for (int i = 0; i < m->n_params; ++i)
      if (std::strcmp(m->params[i].key, key) == 0) v = m->params[i].value;
    return v;
  }
  std::string word(const char* key, const char* def) const { const char* v = text(key); return v ? v : def; }
  // A number: the whole token, "inf" and YAML's .inf / .Inf / .INF (signed or not) included, never NaN.  Any other leading
  // dot is a plain float (.5 is 0.5)
  double num(const char* key, double def) const {
    const char* v = text(key);
    if (!v) return def;
    std::string s(v);
    const size_t sign = (!s.empty() && (s[0] == '+' || s[0] == '-')) ? 1 : 0;
    const std::string rest = s.substr(sign);
    if (rest == ".inf" || rest == ".Inf" || rest == ".INF") s = s.substr(0, sign) + "inf";
    char* end = nullptr;
    const double x = s.empty() || std::isspace((unsigned char)s[0]) ? NAN : std::strtod(s.c_str(), &end);
    if (std::isnan(x) || *end != '\0') refuse(name() + ": " + key + " is not a number");
    return x;
  }
  double finite(const char* key, double def) const {
    const double x = num(key, def);
    if (std::isinf(x)) refuse(name() + ": " + key + " must be finite");
    return x;
  }
  // An integer parameter of the modules of icp_default.yaml (knn of the sampling filter, the checkers' counts): digits, and
  // a fraction that is dropped -- both facades always took 7.5 as 7 there, and neither an exponent or an infinity
  int truncated(const char* key, int def) const {
    const char* v = text(key);
    const double x = num(key, def);
    if ((v && v[std::strspn(v, "+-.0123456789")] != '\0') || !(std::fabs(x) < 2147483648.0)) refuse(name() + ": " + key + " is not an integer");
    return (int)x;
  }
  bool whole(double x) const { return std::fabs(x) < 2147483648.0 && x == (double)(int)x; }
};

// CovarianceSamplingDataPointsFilter runs as its section's last thinning step: the section's MaxDensity- or
// ShadowDataPointsFilter behind it is refused
const char* const kCovSampling = "CovarianceSamplingDataPointsFilter";
void not_behind_cov_sampling(const Load& l) {
  const int s = l.side();
  if ((s == 0 ? l.cov_sampling.reading_nb_sample : l.cov_sampling.reference_nb_sample) > 0)
    refuse(std::string(l.m->section) + ": " + kCovSampling + " in front of " + l.name() + " is not implemented (the module runs as the section's last thinning step)");
}

// SurfaceNormalDataPointsFilter's parameters (either side): keepNormals 1, exact (epsilon 0), no maxDist -> knn.
// keep_densities: where keepDensities (0 or 1) goes -- the reference's module; nullptr (the reading's): 1 is refused
int surface_normal_knn(const Load& l, bool* keep_densities) {
  const std::string n = l.name();
  const double k = l.num("knn", 5);
  if (!(k >= 3 && k <= 32) || !l.whole(k)) refuse(n + ": knn must be an integer in [3, 32]");
  if (l.num("epsilon", 0.0) != 0.0) refuse(n + ": epsilon must be 0 (the search is exact)");
  const double md = l.num("maxDist", INFINITY);
  if (!(std::isinf(md) && md > 0.0)) refuse(n + ": maxDist must be absent or inf");
  if (l.num("keepNormals", 1) != 1.0) refuse(n + ": keepNormals must be 1 (the module is there for the normals)");
  const double kd = l.num("keepDensities", 0);
  if (kd != 0.0 && kd != 1.0) refuse(n + ": keepDensities must be 0 or 1");
  if (kd == 1.0 && !keep_densities) refuse(std::string(l.m->section) + ": " + n + ": keepDensities 1: reading densities are not computed");
  if (keep_densities) *keep_densities = kd == 1.0;
  for (const char* key : {"keepEigenValues", "keepEigenVectors", "keepMatchedIds", "keepMeanDist",
                          "sortEigen", "smoothNormals"})
    if (l.num(key, 0) != 0.0) refuse(n + ": " + key + " must be 0 or absent");
  return (int)k;
}

void random_sampling(Load& l) {
  if (l.stage[0] >= 2)
    refuse("readingDataPointsFilters: SurfaceNormalDataPointsFilter before RandomSamplingDataPointsFilter is not "
           "implemented (the normals would have to be gathered through the sampling)");
  l.out.chain.reading_prob = (float)l.finite("prob", 0.75);
  l.cuts.reading_sampling_at = l.cuts.n_reading;   // the cut modules so far stand in front of it
  l.stage[0] = 1;
}
// The cut modules (MaxDist-, MinDist-, BoundingBox-, RemoveNaNDataPointsFilter) of a filter section: any number up to
// LSGPU_CHAIN_CUT_MAX, any order, around RandomSampling on the reading, and in front of whatever produces or reads normals
lsgpu_point_filter& cut_slot(Load& l) {
  const int s = l.side();
  if (l.stage[s] >= (s == 0 ? 2 : 1))
    refuse(std::string(l.m->section) + ": " + l.name() + " behind the module that produces the normals is not implemented: the "
           "normals would have to be gathered through the cut");
  int& n = s == 0 ? l.cuts.n_reading : l.cuts.n_reference;
  if (n == LSGPU_CHAIN_CUT_MAX)
    refuse(std::string(l.m->section) + ": " + l.name() + " is a ninth cut module (at most " + std::to_string(LSGPU_CHAIN_CUT_MAX) +
           " of MaxDist-, MinDist-, BoundingBox- and RemoveNaNDataPointsFilter in a section)");
  return (s == 0 ? l.cuts.reading : l.cuts.reference)[n++];   // (zero-filled by load())
}
int cut_dim(const Load& l) {
  const double d = l.num("dim", -1);
  if (!l.whole(d) || d < -1.0 || d > 2.0) refuse(l.name() + ": dim must be an integer in [-1, 2]");
  return (int)d;
}
void cut_max_dist(Load& l) {
  const int dim = cut_dim(l);
  const float v = (float)l.num("maxDist", 1.0);
  lsgpu_point_filter& f = cut_slot(l);
  f.type = LSGPU_FILTER_MAX_DIST; f.dim = dim; f.v[0] = v;
}
void cut_min_dist(Load& l) {
  const int dim = cut_dim(l);
  const float v = (float)l.num("minDist", 1.0);
  lsgpu_point_filter& f = cut_slot(l);
  f.type = LSGPU_FILTER_MIN_DIST; f.dim = dim; f.v[0] = v;
}
void cut_bounding_box(Load& l) {
  const char* keys[6] = {"xMin", "xMax", "yMin", "yMax", "zMin", "zMax"};
  float v[6];
  for (int i = 0; i < 6; ++i) v[i] = (float)l.num(keys[i], (i & 1) ? 1.0 : -1.0);
  const double ri = l.num("removeInside", 1);
  if (ri != 0.0 && ri != 1.0) refuse(l.name() + ": removeInside must be 0 or 1");
  lsgpu_point_filter& f = cut_slot(l);
  f.type = LSGPU_FILTER_BOUNDING_BOX; f.flag = (int)ri;
  for (int i = 0; i < 6; ++i) f.v[i] = v[i];
}
void cut_remove_nan(Load& l) { cut_slot(l).type = LSGPU_FILTER_REMOVE_NAN; }

void reading_normals(Load& l) { l.out.normals.reading_sn_knn = surface_normal_knn(l, nullptr); l.stage[0] = 2; }
void sampling_surface_normal(Load& l) {
  if (l.stage[1]) refuse(kOneReference);
  l.out.chain.ssn_knn = l.truncated("knn", 7);
  l.out.chain.ssn_ratio = (float)l.finite("ratio", 0.5);
  if (l.truncated("samplingMethod", 0) != 0) refuse(l.name() + ": samplingMethod != 0 is not implemented");
  l.stage[1] = 1; l.ref_module = true;
}
void reference_normals(Load& l) {
  if (l.stage[1]) refuse(kOneReference);
  l.out.chain.sn_knn = surface_normal_knn(l, &l.ref_densities);
  l.stage[1] = 1; l.ref_module = true;
}
// MaxDensityDataPointsFilter: directly behind the reference's SurfaceNormalDataPointsFilter with keepDensities 1, in front of the
// orientation pair, once.  The two slots of lsgpu_loaded_chain.reserved
void max_density_filter(Load& l) {
  not_behind_cov_sampling(l);
  const std::string n = l.name();
  const char* const where = " may stand only in referenceDataPointsFilters, directly behind SurfaceNormalDataPointsFilter with "
                            "keepDensities 1 and in front of ObservationDirectionDataPointsFilter / OrientNormalsDataPointsFilter";
  if (l.side() == 0) refuse("readingDataPointsFilters: " + n + ": reading densities are not computed (the module" + where + ")");
  if (l.stage[1] == 1 && l.out.chain.ssn_knn > 0)
    refuse("referenceDataPointsFilters: " + n + " behind SamplingSurfaceNormalDataPointsFilter: no densities (the module" + where + ")");
  if (l.stage[1] != 1 || !l.ref_densities || l.max_density) refuse("referenceDataPointsFilters: " + n + where);
  const double md = l.num("maxDensity", 10.0);
  const float f = (float)md;
  if (!(md > 0.0) || !(f > 0.f)) refuse(n + ": maxDensity must be > 0");
  l.out.reserved[4] = 1;
  std::memcpy(&l.out.reserved[5], &f, sizeof(f));
  l.max_density = true;
}
// ShadowDataPointsFilter {eps}: behind the section's normals module (and behind MaxDensityDataPointsFilter, which load() sees to),
// not inside the orientation pair, once (the row).  stage[] stays as it is: the pair may still follow
void shadow_filter(Load& l) {
  not_behind_cov_sampling(l);
  const std::string n = l.name();
  const int s = l.side();
  const std::string sec = std::string(l.m->section) + ": ";
  if (l.stage[s] < (s == 0 ? 2 : 1) || (s == 1 && !l.ref_module))   // (carried normals do not count: the module's own)
    refuse(sec + n + " needs the normals: it may stand only behind " +
           (s == 0 ? "the reading's SurfaceNormalDataPointsFilter" : "SamplingSurfaceNormalDataPointsFilter or SurfaceNormalDataPointsFilter") +
           " (a chain with no such module in the section cannot run it)");
  if (l.stage[s] == 3)
    refuse(sec + n + " may not stand between ObservationDirectionDataPointsFilter and OrientNormalsDataPointsFilter (the pair is implemented as one step)");
  const double e = l.finite("eps", 0.1);
  const float f = (float)e;
  if (!(e >= 0.0 && e <= 3.1416) || !lsgpu::shadow::eps_ok(f)) refuse(n + ": eps must be in [0, 3.1416]");
  (s == 0 ? l.shadow.reading_eps : l.shadow.reference_eps) = f;
}
// CovarianceSamplingDataPointsFilter {nbSample, torqueNorm}: behind the section's normals module, behind its MaxDensity- and
// ShadowDataPointsFilter (their handlers see to that), not inside the orientation pair, once (the row).  stage[] stays as it
// is: the pair may still follow (the module does not read the normals' signs)
void cov_sampling_filter(Load& l) {
  const std::string n = l.name();
  const int s = l.side();
  const std::string sec = std::string(l.m->section) + ": ";
  if (l.stage[s] < (s == 0 ? 2 : 1) || (s == 1 && !l.ref_module))   // (carried normals do not count: the module's own)
    refuse(sec + n + " needs the normals: it may stand only behind " +
           (s == 0 ? "the reading's SurfaceNormalDataPointsFilter" : "SamplingSurfaceNormalDataPointsFilter or SurfaceNormalDataPointsFilter") +
           " (a chain with no such module in the section cannot run it)");
  if (l.stage[s] == 3)
    refuse(sec + n + " may not stand between ObservationDirectionDataPointsFilter and OrientNormalsDataPointsFilter (the pair is implemented as one step)");
  const double nb = l.num("nbSample", 5000);
  if (!l.whole(nb) || !lsgpu::covs::nb_sample_ok((long long)nb)) refuse(n + ": nbSample must be an integer in [1, 2147483632]");
  const double tn = l.num("torqueNorm", 1);
  if (tn != 0.0 && tn != 1.0 && tn != 2.0) refuse(n + ": torqueNorm must be 0, 1 or 2");
  (s == 0 ? l.cov_sampling.reading_nb_sample : l.cov_sampling.reference_nb_sample) = (int)nb;
  (s == 0 ? l.cov_sampling.reading_torque_norm : l.cov_sampling.reference_torque_norm) = (int)tn;
}
void observation_direction(Load& l) {
  const int s = l.side();
  // (a carried reference: the pair may stand without a module, on the normals the cloud brings along)
  const bool on_carried = s == 1 && l.stage[1] == 0 && (l.carried & LSGPU_CARRIED_REFERENCE) != 0;
  if (l.stage[s] != (s == 0 ? 2 : 1) && !on_carried) refuse(std::string(l.m->section) + ": " + l.name() + kPair);
  float* sensor = s == 0 ? l.out.normals.reading_sensor : l.out.normals.reference_sensor;
  const char* keys[3] = {"x", "y", "z"};
  for (int i = 0; i < 3; ++i) {
    sensor[i] = (float)l.finite(keys[i], 0.0);
  }
  l.stage[s] = 3;
}
void orient_normals(Load& l) {
  const int s = l.side();
  if (l.stage[s] != 3) refuse(std::string(l.m->section) + ": " + l.name() + kPair);
  const double tc = l.num("towardCenter", 1);
  if (tc != 0.0 && tc != 1.0) refuse(l.name() + ": towardCenter must be 0 or 1");
  (s == 0 ? l.out.normals.reading_orient : l.out.normals.reference_orient) = tc == 1.0 ? 1 : 2;
  l.stage[s] = 4;
}
// knn 1..LSGPU_MATCHER_KNN_MAX, exact search only, maxDist; searchType is accepted and not read.  The one module that may be
// given again (the last one counts): both facades always took it so
void kd_tree_matcher(Load& l) {
  const double md = l.num("maxDist", INFINITY);
  if (!(md > 0.0)) refuse("KDTreeMatcher: maxDist must be > 0");
  l.out.icp.matcher_max_dist = std::isinf(md) ? 0.f : (float)md;
  const double k = l.num("knn", 1);
  if (!(k >= 1 && k <= LSGPU_MATCHER_KNN_MAX) || !l.whole(k) || l.num("epsilon", 0) != 0.0)
    refuse("KDTreeMatcher: knn 1.." + std::to_string(LSGPU_MATCHER_KNN_MAX) + " with epsilon 0 is implemented");
  l.out.icp.matcher_knn = (int)k;
  l.matcher = true;
}
void trimmed_dist(Load& l) {
  const double r = l.num("ratio", 0.85);
  if (!(r > 0.0 && r <= 1.0)) refuse(l.name() + ": ratio must be in (0, 1]");
  l.out.icp.trim_ratio = (float)r;
}
void max_dist(Load& l) {
  const double md = l.num("maxDist", 1.0);
  if (!(md > 0.0)) refuse(l.name() + ": maxDist must be > 0");
  l.out.icp.outlier_max_dist = std::isinf(md) ? 0.f : (float)md;
}
void min_dist(Load& l) {
  const double md = l.finite("minDist", 1.0);
  if (!(md >= 0.0)) refuse(l.name() + ": minDist must be >= 0");
  l.out.icp.outlier_min_dist = (float)md;
}
void median_dist(Load& l) {
  const double f = l.finite("factor", 3.0);
  if (!(f > 0.0)) refuse(l.name() + ": factor must be > 0");
  l.out.icp.outlier_median_factor = (float)f;
}
void robust_outlier(Load& l) {
  const std::string n = l.name();
  auto pick = [&](const char* key, const std::string& v, std::initializer_list<const char*> names) {
    int i = 0;
    for (const char* s : names) { if (v == s) return i; ++i; }
    refuse(n + ": unknown " + key + " " + v);
  };
  const std::string fct = l.word("robustFct", "cauchy"), est = l.word("scaleEstimator", "mad");
  if (fct == "welsch" || fct == "student")
    refuse(n + ": robustFct " + fct + " is not implemented on the HIP path (exp / pow are not bit-identical between host and device)");
  if (est == "berg" || est == "std") refuse(n + ": scaleEstimator " + est + " is not implemented on the HIP path (none and mad are)");
  lsgpu_robust_config& rb = l.out.robust;
  rb.robust_fct = pick("robustFct", fct, {"cauchy", "huber", "tukey", "gm", "sc", "L1"});
  rb.scale_estimator = pick("scaleEstimator", est, {"none", "mad"});
  rb.distance_type = pick("distanceType", l.word("distanceType", "point2point"), {"point2point", "point2plane"});
  const double nb = l.num("nbIterationForScale", 0);
  if (!(nb >= 0.0) || !l.whole(nb)) refuse(n + ": nbIterationForScale must be an integer >= 0");
  rb.tuning = (float)l.num("tuning", 1.0);
  rb.approximation = (float)l.num("approximation", INFINITY);
  rb.nb_iteration_for_scale = (int)nb;
  l.robust = true;   // (tuning / approximation: robust::check in finish())
}
void surface_normal_outlier(Load& l) {
  const double a = l.num("maxAngle", 1.57);
  if (!(a >= 0.0 && a <= 3.1416)) refuse(l.name() + ": maxAngle must be in [0, 3.1416]");
  l.out.normals.max_angle = (float)a;
}
// force2D / force4DOF: 0 or 1 each, read on PointToPlaneErrorMinimizer; PointToPointErrorMinimizer is refused either one by
// name.  Every other parameter of the two modules stays not looked at (the row)
int flag01(const Load& l, const char* key) {
  const double v = l.num(key, 0);
  if (v != 0.0 && v != 1.0) refuse(l.name() + ": " + key + " must be 0 or 1");
  return (int)v;
}
void error_minimizer(Load& l) {
  if (l.minimizer) refuse("errorMinimizer: one module at most (" + l.name() + " is a second one)");
  const bool p2p = l.name() == "PointToPointErrorMinimizer";
  l.out.icp.error_minimizer = p2p ? LSGPU_MINIMIZER_POINT_TO_POINT : LSGPU_MINIMIZER_POINT_TO_PLANE;
  l.minimizer = true;
  if (l.name() == "PointToPlaneWithCovErrorMinimizer") return;   // (its row refuses the two parameters as unknown)
  if (p2p) {
    for (const char* key : {"force2D", "force4DOF"})
      if (l.text(key)) refuse(l.name() + ": " + key + " is not implemented on the HIP path (the constrained steps are those of PointToPlaneErrorMinimizer)");
    return;
  }
  const int f2 = flag01(l, "force2D"), f4 = flag01(l, "force4DOF");
  if (f2 && f4) refuse(l.name() + ": force2D 1 together with force4DOF 1 is not implemented (what upstream does with both is not restated)");
  l.motion.dof = f2 ? LSGPU_MOTION_DOF_3 : f4 ? LSGPU_MOTION_DOF_4 : LSGPU_MOTION_DOF_6;
}
// the step of PointToPlaneErrorMinimizer plus the covariance of the result: the two slots of lsgpu_loaded_chain.reserved
void error_minimizer_with_cov(Load& l) {
  error_minimizer(l);
  const double sd = l.finite("sensorStdDev", 0.01);
  if (!(sd >= 0.0)) refuse(l.name() + ": sensorStdDev must be >= 0");
  const float f = (float)sd;
  l.out.reserved[0] = 1;
  std::memcpy(&l.out.reserved[1], &f, sizeof(f));
  l.with_cov = true;
}
void counter_checker(Load& l) { l.out.icp.max_iterations = l.truncated("maxIterationCount", 40); l.counter = true; }
void differential_checker(Load& l) {
  l.out.icp.min_diff_rot = (float)l.finite("minDiffRotErr", 0.001);
  l.out.icp.min_diff_trans = (float)l.finite("minDiffTransErr", 0.001);
  l.out.icp.smooth_length = l.truncated("smoothLength", 3);
}

// BoundTransformationChecker {maxRotationNorm, maxTranslationNorm}: once (the row); where it stands relative to the counter
// decides whether the counter's last iteration is checked
void bound_checker(Load& l) {
  const double r = l.num("maxRotationNorm", 1.0), t = l.num("maxTranslationNorm", 1.0);
  if (!(r >= 0.0) || std::isinf(r) || std::isinf((float)r)) refuse(l.name() + ": maxRotationNorm must be finite and >= 0");
  if (!(t >= 0.0) || std::isinf(t) || std::isinf((float)t)) refuse(l.name() + ": maxTranslationNorm must be finite and >= 0");
  l.motion.bound = 1;
  l.motion.max_rotation_norm = (float)r; l.motion.max_translation_norm = (float)t;
  l.motion.bound_before_counter = l.counter ? 0 : 1;
}

struct Row {
  const char* section;
  const char* name;
  const char* params;   // the parameters the module has, space-separated; nullptr: not looked at
  bool once;            // a second instance in the section is refused here (false: the handler says what may come twice)
  void (*load)(Load&);
};
const Row kRows[] = {
    {"readingDataPointsFilters", "RandomSamplingDataPointsFilter", "prob", true, random_sampling},
    {"readingDataPointsFilters", "SurfaceNormalDataPointsFilter", kSurfaceNormalParams, true, reading_normals},
    {"readingDataPointsFilters", "ObservationDirectionDataPointsFilter", "x y z", true, observation_direction},
    {"readingDataPointsFilters", "OrientNormalsDataPointsFilter", "towardCenter", true, orient_normals},
    {"referenceDataPointsFilters", "SamplingSurfaceNormalDataPointsFilter", "knn ratio samplingMethod", false, sampling_surface_normal},
    {"referenceDataPointsFilters", "SurfaceNormalDataPointsFilter", kSurfaceNormalParams, false, reference_normals},
    {"referenceDataPointsFilters", "MaxDensityDataPointsFilter", "maxDensity", false, max_density_filter},
    {"readingDataPointsFilters", "MaxDensityDataPointsFilter", "maxDensity", false, max_density_filter},
    {"referenceDataPointsFilters", "ShadowDataPointsFilter", "eps", true, shadow_filter},
    {"readingDataPointsFilters", "ShadowDataPointsFilter", "eps", true, shadow_filter},
    {"referenceDataPointsFilters", "CovarianceSamplingDataPointsFilter", "nbSample torqueNorm", true, cov_sampling_filter},
    {"readingDataPointsFilters", "CovarianceSamplingDataPointsFilter", "nbSample torqueNorm", true, cov_sampling_filter},
    {"referenceDataPointsFilters", "ObservationDirectionDataPointsFilter", "x y z", true, observation_direction},
    {"referenceDataPointsFilters", "OrientNormalsDataPointsFilter", "towardCenter", true, orient_normals},
    {"readingDataPointsFilters", "MaxDistDataPointsFilter", "dim maxDist", false, cut_max_dist},
    {"readingDataPointsFilters", "MinDistDataPointsFilter", "dim minDist", false, cut_min_dist},
    {"readingDataPointsFilters", "BoundingBoxDataPointsFilter", kBoundingBoxParams, false, cut_bounding_box},
    {"readingDataPointsFilters", "RemoveNaNDataPointsFilter", "", false, cut_remove_nan},
    {"referenceDataPointsFilters", "MaxDistDataPointsFilter", "dim maxDist", false, cut_max_dist},
    {"referenceDataPointsFilters", "MinDistDataPointsFilter", "dim minDist", false, cut_min_dist},
    {"referenceDataPointsFilters", "BoundingBoxDataPointsFilter", kBoundingBoxParams, false, cut_bounding_box},
    {"referenceDataPointsFilters", "RemoveNaNDataPointsFilter", "", false, cut_remove_nan},
    {"matcher", "KDTreeMatcher", "knn epsilon searchType maxDist", false, kd_tree_matcher},
    {"outlierFilters", "TrimmedDistOutlierFilter", "ratio", true, trimmed_dist},
    {"outlierFilters", "MaxDistOutlierFilter", "maxDist", true, max_dist},
    {"outlierFilters", "MinDistOutlierFilter", "minDist", true, min_dist},
    {"outlierFilters", "MedianDistOutlierFilter", "factor", true, median_dist},
    {"outlierFilters", "RobustOutlierFilter", "robustFct tuning scaleEstimator nbIterationForScale distanceType approximation", true, robust_outlier},
    {"outlierFilters", "SurfaceNormalOutlierFilter", "maxAngle", true, surface_normal_outlier},
    {"errorMinimizer", "PointToPlaneErrorMinimizer", nullptr, false, error_minimizer},
    {"errorMinimizer", "PointToPointErrorMinimizer", nullptr, false, error_minimizer},
    {"errorMinimizer", "PointToPlaneWithCovErrorMinimizer", "sensorStdDev", false, error_minimizer_with_cov},
    {"transformationCheckers", "CounterTransformationChecker", "maxIterationCount", true, counter_checker},
    {"transformationCheckers", "DifferentialTransformationChecker", "minDiffRotErr minDiffTransErr smoothLength", true, differential_checker},
    {"transformationCheckers", "BoundTransformationChecker", "maxRotationNorm maxTranslationNorm", true, bound_checker},
};
constexpr int kNumRows = (int)(sizeof(kRows) / sizeof(kRows[0]));

// What the device loop needs: a matcher, a minimiser, a stopping rule, normals for whoever reads them.  (Absent reading
// filter: every point; absent outlier filter: every pair; absent reference filter with the point-to-point minimiser, which
// reads no normals: the reference as given; absent differential checker: the counter stops the loop.)
void finish(Load& l) {
  lsgpu_loaded_chain& o = l.out;
  if (l.ref_densities && !l.max_density) refuse(kDensitiesAlone);
  const int have_normals = l.stage[1] != 0 || (l.carried & LSGPU_CARRIED_REFERENCE) != 0;
  if ((l.carried & LSGPU_CARRIED_READING) && o.normals.max_angle >= 0.f && o.normals.reading_sn_knn == 0) o.normals.reading_normals_given = 1;
  if (!l.matcher) refuse("matcher: KDTreeMatcher is required");
  if (!l.minimizer) refuse("errorMinimizer: PointToPlaneErrorMinimizer, PointToPlaneWithCovErrorMinimizer or PointToPointErrorMinimizer is required");
  if (!have_normals && o.icp.error_minimizer != LSGPU_MINIMIZER_POINT_TO_POINT)
    refuse("referenceDataPointsFilters: SamplingSurfaceNormalDataPointsFilter or SurfaceNormalDataPointsFilter is required (it "
           "provides the normals of PointToPlaneErrorMinimizer)");
  const char* why = nullptr;
  if (l.robust && lsgpu::robust::check(&o.robust, o.icp.error_minimizer, have_normals, &why) != LSGPU_OK) refuse(why);
  for (int s = 0; s < 2; ++s)
    if (l.stage[s] == 3)
      refuse(std::string(s == 0 ? "readingDataPointsFilters" : "referenceDataPointsFilters") + ": ObservationDirectionDataPointsFilter" + kPair);
  const bool shadow = l.shadow.reading_eps >= 0.f || l.shadow.reference_eps >= 0.f;
  if (l.shadow.reading_eps >= 0.f && !(o.normals.max_angle >= 0.f))   // (in front of the rule below, whose text does not name the module)
    refuse("readingDataPointsFilters: ShadowDataPointsFilter without SurfaceNormalOutlierFilter is not implemented (reading normals that "
           "no outlier filter reads are refused, and the module alone does not change that)");
  const bool cov_sampling = l.cov_sampling.reading_nb_sample > 0 || l.cov_sampling.reference_nb_sample > 0;
  if (l.cov_sampling.reading_nb_sample > 0 && !(o.normals.max_angle >= 0.f))   // (likewise)
    refuse(std::string("readingDataPointsFilters: ") + kCovSampling + " without SurfaceNormalOutlierFilter is not implemented (reading normals that "
           "no outlier filter reads are refused, and the module alone does not change that)");
  if (lsgpu::normal_angle::check(&o.normals, o.icp.error_minimizer, have_normals, &why) != LSGPU_OK) refuse(why);
  if (!l.counter) refuse("transformationCheckers: CounterTransformationChecker is required (the loop would not stop)");
  {   // what the covariance pass and the constrained steps do not cover: the rule set's verdict on what is loaded (lsgpu_modules.h)
    lsgpu::modules::State s;
    s.robust_on = l.robust; s.normals_on = true; s.normals = o.normals; s.cov_on = l.with_cov; s.md_on = l.max_density;
    s.sh_on = shadow; s.cs_on = cov_sampling; s.mo_on = true; s.mo_cfg = l.motion;
    lsgpu::modules::Facts f;
    f.matcher_knn = o.icp.matcher_knn;
    const std::string refused = lsgpu::modules::refusal(s, f, lsgpu::modules::kLoader);
    if (!refused.empty()) refuse(refused);
  }
  if (o.chain.reading_prob < 0.f) l.cuts.reading_sampling_at = l.cuts.n_reading;   // (no RandomSampling: not read)
  o.reserved[2] = l.cuts.n_reading; o.reserved[3] = l.cuts.n_reference;
  o.has_robust = l.robust ? 1 : 0;
  o.has_normals = o.normals.max_angle >= 0.f || o.normals.reading_sn_knn != 0 || o.normals.reading_orient != 0 || o.normals.reference_orient != 0;
}

void load(const lsgpu_yaml_module* mods, int n_mods, Load& l, unsigned carried) {
  l.carried = carried;
  // libpointmatcher's loadFromYaml starts from EMPTY chains: a section the file does not mention means "no such module",
  // not "the default module"
  std::memset(&l.out, 0, sizeof(l.out));
  std::memset(&l.cuts, 0, sizeof(l.cuts));
  std::memset(&l.shadow, 0, sizeof(l.shadow));
  l.shadow.reading_eps = -1.f; l.shadow.reference_eps = -1.f;
  std::memset(&l.cov_sampling, 0, sizeof(l.cov_sampling));   // (= lsgpu_cov_sampling_config_default)
  l.cov_sampling.reading_torque_norm = 1; l.cov_sampling.reference_torque_norm = 1;
  std::memset(&l.motion, 0, sizeof(l.motion));   // (= lsgpu_motion_config_default: this file stands alone in one of the tests)
  l.motion.max_rotation_norm = 1.f; l.motion.max_translation_norm = 1.f;
  lsgpu_icp_config_default(&l.out.icp);
  l.out.icp.trim_ratio = 1.0f;
  l.out.icp.min_diff_rot = -1.f; l.out.icp.min_diff_trans = -1.f; l.out.icp.smooth_length = 1;   // never satisfied
  lsgpu_chain_config_default(&l.out.chain);
  l.out.chain.reading_prob = -1.0f;   // no reading filter: every point, no draws
  l.out.chain.ssn_knn = 0;
  lsgpu_robust_config_default(&l.out.robust);
  lsgpu_normals_config_default(&l.out.normals);
  bool seen[kNumRows] = {};
  for (int i = 0; i < n_mods; ++i) {
    const lsgpu_yaml_module& m = mods[i];
    if (!std::strcmp(m.section, "inspector") || !std::strcmp(m.section, "logger")) continue;   // debug output only (yaml:32-44)
    int r = 0;
    while (r < kNumRows && (std::strcmp(kRows[r].section, m.section) || std::strcmp(kRows[r].name, m.name))) ++r;
    if (r == kNumRows) refuse(std::string(m.section) + ": module " + m.name + " is not implemented on the HIP path");
    if (seen[r] && kRows[r].once) refuse(std::string(m.section) + ": " + m.name + " given twice");
    seen[r] = true;
    for (int p = 0; kRows[r].params && p < m.n_params; ++p)
      if (!listed(kRows[r].params, m.params[p].key)) refuse(std::string(m.name) + ": unknown parameter " + m.params[p].key);
    l.m = &m;
    if (l.ref_densities && !l.max_density && kRows[r].load == cov_sampling_filter && l.side() == 1)   // (the reference's own module; in front of the rule below, whose text does not name the module)
      refuse(std::string(m.section) + ": " + kCovSampling + " in front of MaxDensityDataPointsFilter is not implemented (keepDensities 1 needs "
             "MaxDensityDataPointsFilter directly behind SurfaceNormalDataPointsFilter; the module runs as the section's last thinning step)");
    if (l.ref_densities && !l.max_density && kRows[r].load != max_density_filter) refuse(kDensitiesAlone);
    kRows[r].load(l);
  }
  finish(l);
}

}  // namespace

extern "C" {

// the entry points: the one walk over the modules, then what the caller asked for (all of it: lsgpu_chain_load_modules; `chain`,
// `cuts`, `shadow`, `motion` or `cov_sampling`, the others NULL: the part loaders)
static int load_into(const lsgpu_yaml_module* mods, int n_mods, lsgpu_loaded_chain* chain, lsgpu_chain_cuts* cuts, lsgpu_shadow_config* shadow,
                     char* why, int why_cap, lsgpu_motion_config* motion = nullptr, lsgpu_cov_sampling_config* cov_sampling = nullptr,
                     unsigned carried = 0) {
  if (why && why_cap > 0) why[0] = '\0';
  if ((!chain && !cuts && !shadow && !motion && !cov_sampling) || n_mods < 0 || (n_mods > 0 && !mods)) return LSGPU_BAD_ARG;
  for (int i = 0; i < n_mods; ++i) {
    if (!mods[i].section || !mods[i].name || mods[i].n_params < 0 || (mods[i].n_params > 0 && !mods[i].params)) return LSGPU_BAD_ARG;
    for (int p = 0; p < mods[i].n_params; ++p)
      if (!mods[i].params[p].key || !mods[i].params[p].value) return LSGPU_BAD_ARG;
  }
  try {
    Load l;
    load(mods, n_mods, l, carried);
    if (chain) *chain = l.out;
    if (cuts) *cuts = l.cuts;
    if (shadow) *shadow = l.shadow;
    if (motion) *motion = l.motion;
    if (cov_sampling) *cov_sampling = l.cov_sampling;
    return LSGPU_OK;
  } catch (const Refusal& r) {
    if (why && why_cap > 0) std::snprintf(why, (size_t)why_cap, "%s", r.why.c_str());
    return LSGPU_BAD_CONFIG;
  } catch (const std::exception&) {   // (no exception crosses the ABI)
    return LSGPU_BAD_ARG;
  }
}

int lsgpu_chain_load(const lsgpu_yaml_module* mods, int n_mods, lsgpu_loaded_chain* out, char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  return out ? load_into(mods, n_mods, out, nullptr, nullptr, why, why_cap) : LSGPU_BAD_ARG;
}

int lsgpu_chain_load_cuts(const lsgpu_yaml_module* mods, int n_mods, lsgpu_chain_cuts* out, char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  return out ? load_into(mods, n_mods, nullptr, out, nullptr, why, why_cap) : LSGPU_BAD_ARG;
}

int lsgpu_chain_load_shadow(const lsgpu_yaml_module* mods, int n_mods, lsgpu_shadow_config* out, char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  return out ? load_into(mods, n_mods, nullptr, nullptr, out, why, why_cap) : LSGPU_BAD_ARG;
}

int lsgpu_chain_load_motion(const lsgpu_yaml_module* mods, int n_mods, lsgpu_motion_config* out, char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  return out ? load_into(mods, n_mods, nullptr, nullptr, nullptr, why, why_cap, out) : LSGPU_BAD_ARG;
}

int lsgpu_chain_load_cov_sampling(const lsgpu_yaml_module* mods, int n_mods, lsgpu_cov_sampling_config* out, char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  return out ? load_into(mods, n_mods, nullptr, nullptr, nullptr, why, why_cap, nullptr, out) : LSGPU_BAD_ARG;
}

int lsgpu_chain_load_carried(const lsgpu_yaml_module* mods, int n_mods, unsigned carried, lsgpu_loaded_chain* out, char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  if (!out || (carried & ~(unsigned)(LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE))) return LSGPU_BAD_ARG;
  return load_into(mods, n_mods, out, nullptr, nullptr, why, why_cap, nullptr, nullptr, carried);
}

int lsgpu_chain_load_parts_carried(const lsgpu_yaml_module* mods, int n_mods, unsigned carried, lsgpu_chain_cuts* cuts,
                                   lsgpu_shadow_config* shadow, lsgpu_motion_config* motion, lsgpu_cov_sampling_config* cov_sampling,
                                   char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  if (carried & ~(unsigned)(LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE)) return LSGPU_BAD_ARG;
  return load_into(mods, n_mods, nullptr, cuts, shadow, why, why_cap, motion, cov_sampling, carried);
}

int lsgpu_chain_load_modules(const lsgpu_yaml_module* mods, int n_mods, unsigned carried, lsgpu_chain_modules* out, char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  if (!out || (carried & ~(unsigned)(LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE))) return LSGPU_BAD_ARG;
  lsgpu_chain_modules m;
  std::memset(&m, 0, sizeof(m));
  m.carried = carried;
  const int rc = load_into(mods, n_mods, &m.chain, &m.cuts, &m.shadow, why, why_cap, &m.motion, &m.cov_sampling, carried);
  if (rc == LSGPU_OK) *out = m;
  return rc;
}

int lsgpu_surface_normal_params_check(const lsgpu_yaml_param* params, int n_params, int* knn, char* why, int why_cap) {
  if (why && why_cap > 0) why[0] = '\0';
  if (n_params < 0 || (n_params > 0 && !params)) return LSGPU_BAD_ARG;
  for (int p = 0; p < n_params; ++p)
    if (!params[p].key || !params[p].value) return LSGPU_BAD_ARG;
  const lsgpu_yaml_module m = {"readingDataPointsFilters", "SurfaceNormalDataPointsFilter", params, n_params, 0};
  try {
    for (int p = 0; p < n_params; ++p)
      if (!listed(kSurfaceNormalParams, params[p].key)) refuse(std::string(m.name) + ": unknown parameter " + params[p].key);
    Load l;
    l.m = &m;
    const int k = surface_normal_knn(l, nullptr);
    if (knn) *knn = k;
    return LSGPU_OK;
  } catch (const Refusal& r) {
    if (why && why_cap > 0) std::snprintf(why, (size_t)why_cap, "%s", r.why.c_str());
    return LSGPU_BAD_CONFIG;
  } catch (const std::exception&) {
    return LSGPU_BAD_ARG;
  }
}

int lsgpu_loaded_chain_max_density(const lsgpu_loaded_chain* c, float* max_density) {
  if (!c || c->reserved[4] != 1) return 0;
  if (max_density) std::memcpy(max_density, &c->reserved[5], sizeof(float));
  return 1;
}

int lsgpu_loaded_chain_covariance(const lsgpu_loaded_chain* c, float* sensor_std_dev) {
  if (!c || c->reserved[0] != 1) return 0;
  if (sensor_std_dev) std::memcpy(sensor_std_dev, &c->reserved[1], sizeof(float));
  return 1;
}

}  // extern "C"
