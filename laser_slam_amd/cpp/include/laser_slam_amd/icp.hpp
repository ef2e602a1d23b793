// icp.hpp -- C++ host-side mirror of the ICP object the reference owns (SURVEY.md §8b seam B2).
//
// The reference's `PointMatcher::ICP icp_` (laser_slam/include/laser_slam/laser_track.hpp:217,
// incremental_estimator.hpp:70) is used through three members only:
//     icp_.loadFromYaml(std::istream&)      laser_slam/src/laser_track.cpp:17
//     icp_.setDefault()                     laser_slam/src/laser_track.cpp:20
//     icp_.compute(reading, reference, T)   laser_slam/src/laser_track.cpp:496,
//                                           laser_slam/src/incremental_estimator.cpp:108
// laser_slam_amd::ICP keeps those names, argument meaning and error behaviour (ConvergenceError)
// over the C ABI of include/lsgpu_icp.h.  No libpointmatcher / Eigen / yaml-cpp dependency: clouds
// are plain float vectors in PointMatcher's own memory layout.
#pragma once
#include <array>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <istream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "lsgpu_icp.h"

namespace laser_slam_amd {

// PointMatcher<float>::DataPoints, reduced to what the path uses: features = (dim+1) x N column major
// (x,y,z,1 per point), optional "normals" descriptor 3 x N (laser_slam/.../common.hpp:14-15).
struct DataPoints {
  std::vector<float> features;  // 4 * N
  std::vector<float> normals;   // 3 * N or empty
  int64_t getNbPoints() const { return (int64_t)(features.size() / 4); }
  // DataPoints::concatenate (laser_track.cpp:485)
  void concatenate(const DataPoints& o) {
    const bool both = !normals.empty() && !o.normals.empty();
    features.insert(features.end(), o.features.begin(), o.features.end());
    if (both) normals.insert(normals.end(), o.normals.begin(), o.normals.end());
    else normals.clear();
  }
};

using TransformationParameters = std::array<float, 16>;  // 4x4 float, column major

inline TransformationParameters identityTransformation() {
  TransformationParameters T{};
  T[0] = T[5] = T[10] = T[15] = 1.f;
  return T;
}

// PointMatcher::ConvergenceError (caught at laser_track.cpp:499)
struct ConvergenceError : std::runtime_error {
  explicit ConvergenceError(const std::string& w) : std::runtime_error(w) {}
};
// PointMatcher::TransformationError: RigidTransformation::compute on a matrix that fails checkParameters -- also what
// ICP::compute throws for a non-rigid initial guess (its step 5 moves the reading with RigidTransformation)
struct TransformationError : std::runtime_error {
  explicit TransformationError(const std::string& w) : std::runtime_error(w) {}
};
struct ConfigError : std::runtime_error {
  explicit ConfigError(const std::string& w) : std::runtime_error(w) {}
};
struct DeviceError : std::runtime_error {
  explicit DeviceError(const std::string& w) : std::runtime_error(w) {}
};

// RigidTransformation (laser_track.cpp:33): compute / checkParameters / correctParameters
class RigidTransformation {
 public:
  static bool checkParameters(const TransformationParameters& T) { return lsgpu_check_rigid(T.data()) != 0; }
  static TransformationParameters correctParameters(const TransformationParameters& T) {
    TransformationParameters o;
    lsgpu_correct_rigid(T.data(), o.data());
    return o;
  }
  // features' = T * features; the "normals" descriptor is rotated.  Host arithmetic identical to the
  // device kernel (fma chain), so clouds built on either side agree bit for bit.
  static DataPoints compute(const DataPoints& in, const TransformationParameters& T) {
    if (!checkParameters(T)) throw TransformationError("RigidTransformation: matrix is not rigid");
    DataPoints out;
    const int64_t n = in.getNbPoints();
    out.features.resize((size_t)n * 4);
    auto M = [&](int r, int c) { return T[c * 4 + r]; };
    for (int64_t i = 0; i < n; ++i) {
      const float x = in.features[4 * i], y = in.features[4 * i + 1], z = in.features[4 * i + 2];
      for (int r = 0; r < 3; ++r)
        out.features[4 * i + r] = std::fma(M(r, 2), z, std::fma(M(r, 1), y, std::fma(M(r, 0), x, M(r, 3))));
      out.features[4 * i + 3] = in.features[4 * i + 3];
    }
    if (!in.normals.empty()) {
      out.normals.resize((size_t)n * 3);
      for (int64_t i = 0; i < n; ++i) {
        const float x = in.normals[3 * i], y = in.normals[3 * i + 1], z = in.normals[3 * i + 2];
        for (int r = 0; r < 3; ++r)
          out.normals[3 * i + r] = std::fma(M(r, 2), z, std::fma(M(r, 1), y, M(r, 0) * x));
      }
    }
    return out;
  }
};

// correctTransformationMatrix (laser_slam/include/laser_slam/common.hpp:136-149)
inline void correctTransformationMatrix(TransformationParameters* T) {
  if (!RigidTransformation::checkParameters(*T)) *T = RigidTransformation::correctParameters(*T);
}

namespace detail {

struct YamlModule { std::string section, name; std::map<std::string, std::string> params; };

inline std::string trim(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b && std::isspace((unsigned char)s[a])) ++a;
  while (b > a && std::isspace((unsigned char)s[b - 1])) --b;
  return s.substr(a, b - a);
}
inline void parseInline(const std::string& body, std::map<std::string, std::string>* out) {  // {k: v, k: v}
  std::stringstream ss(body);
  std::string kv;
  while (std::getline(ss, kv, ',')) {
    const size_t c = kv.find(':');
    if (c != std::string::npos) (*out)[trim(kv.substr(0, c))] = trim(kv.substr(c + 1));
  }
}
// A libpointmatcher DataPointsFilters file: a top-level YAML sequence of modules, `- Name` / `- Name:` followed by an
// indented `key: value` block, or `- Name: {key: value, ...}`; `#` comments.  An empty document is an empty chain.
inline std::vector<YamlModule> parseYamlList(std::istream& in) {
  std::vector<YamlModule> mods;
  std::string line;
  int item_indent = -1;
  while (std::getline(in, line)) {
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line = line.substr(0, hash);
    std::string t = trim(line);
    if (t.empty() || t == "---" || t == "[]") continue;
    int indent = 0;
    while (indent < (int)line.size() && line[indent] == ' ') ++indent;
    const bool item = t[0] == '-';
    if (item) t = trim(t.substr(1));
    const size_t c = t.find(':');
    const std::string key = trim(c == std::string::npos ? t : t.substr(0, c));
    const std::string val = c == std::string::npos ? "" : trim(t.substr(c + 1));
    if (item) {
      YamlModule m{"", key, {}};
      if (!val.empty() && val.front() == '{' && val.back() == '}') parseInline(val.substr(1, val.size() - 2), &m.params);
      else if (!val.empty()) throw std::runtime_error("input filters yaml: unexpected scalar after " + key);
      mods.push_back(m);
      item_indent = indent;
    } else {
      if (mods.empty() || indent <= item_indent) throw std::runtime_error("input filters yaml: a sequence of modules is expected");
      mods.back().params[key] = val;
    }
  }
  return mods;
}

}  // namespace detail

// PointMatcher::DataPointsFilters as LaserTrack uses it: built from a YAML stream (laser_slam/src/laser_track.cpp:27),
// applied in place to every incoming scan (laser_track.cpp:81, :146).  The supported modules run on the device
// (lsgpu_apply_point_filters); any other module is a configuration error, like an unknown name is for
// PointMatcher's registrar.  FixStepSampling keeps its step between calls, as the upstream object does.
// The chain may END with the modules that give a scan its normals -- SurfaceNormalDataPointsFilter, optionally followed
// directly by ObservationDirectionDataPointsFilter + OrientNormalsDataPointsFilter: apply() runs them on what the point
// modules kept (lsgpu_icp_reading_normals), the cloud's `normals` hold the result and travel with the scan from then on
// (include/lsgpu_icp.h, "carried normals").  A point module behind that tail is a configuration error.  The tail is read only
// where the caller asks for it (normals_tail; LaserTrack does): a caller that does not hand the normals on keeps the refusal.
class ICP;
class DataPointsFilters {
 public:
  DataPointsFilters() = default;
  explicit DataPointsFilters(std::istream& in, int device = 0, bool normals_tail = false) : device_(device) {
    int tail = 0;   // 1: SurfaceNormalDataPointsFilter seen, 2: ObservationDirection behind it, 3: OrientNormals behind that
    for (const auto& m : detail::parseYamlList(in)) {
      auto num = [&](const char* key, double def) {
        auto it = m.params.find(key);
        return it == m.params.end() ? def : std::stod(it->second);
      };
      auto only = [&](std::initializer_list<const char*> keys) {
        for (const auto& kv : m.params) {
          bool known = false;
          for (const char* k : keys) known = known || kv.first == k;
          if (!known) throw ConfigError(m.name + ": unknown parameter " + kv.first);
        }
      };
      if (!normals_tail) {
        // (the three modules of the tail fall through to the refusal of an unknown module below)
      } else if (m.name == "SurfaceNormalDataPointsFilter") {
        // the parameters are judged by the rule the ICP chain's loader applies to the reading's module
        if (tail) throw ConfigError("input filters: SurfaceNormalDataPointsFilter given twice");
        std::vector<lsgpu_yaml_param> ps;
        for (const auto& kv : m.params) ps.push_back({kv.first.c_str(), kv.second.c_str()});
        char why[512];
        if (lsgpu_surface_normal_params_check(ps.data(), (int)ps.size(), &normals_knn_, why, (int)sizeof(why)) != LSGPU_OK)
          throw ConfigError(std::string("input filters: ") + why);
        tail = 1;
        continue;
      } else if (m.name == "ObservationDirectionDataPointsFilter") {
        if (tail != 1) throw ConfigError("input filters: ObservationDirectionDataPointsFilter is implemented only as the pair "
                                         "ObservationDirectionDataPointsFilter, OrientNormalsDataPointsFilter directly behind SurfaceNormalDataPointsFilter");
        only({"x", "y", "z"});
        const char* keys[3] = {"x", "y", "z"};
        for (int a = 0; a < 3; ++a) {
          sensor_[a] = (float)num(keys[a], 0.0);
          if (!std::isfinite(sensor_[a])) throw ConfigError(m.name + ": x, y, z must be finite");
        }
        tail = 2;
        continue;
      } else if (m.name == "OrientNormalsDataPointsFilter") {
        if (tail != 2) throw ConfigError("input filters: OrientNormalsDataPointsFilter is implemented only as the pair "
                                         "ObservationDirectionDataPointsFilter, OrientNormalsDataPointsFilter directly behind SurfaceNormalDataPointsFilter");
        only({"towardCenter"});
        const double tc = num("towardCenter", 1);
        if (tc != 0 && tc != 1) throw ConfigError(m.name + ": towardCenter must be 0 or 1");
        orient_ = tc == 1 ? 1 : 2;
        tail = 3;
        continue;
      }
      if (tail) throw ConfigError("input filters: " + m.name + " behind SurfaceNormalDataPointsFilter is not implemented (the normals "
                                  "modules are the chain's last: the normals would have to be gathered through the module)");
      lsgpu_point_filter f;
      std::memset(&f, 0, sizeof(f));
      if (m.name == "MaxDistDataPointsFilter") {
        only({"dim", "maxDist"});
        f.type = LSGPU_FILTER_MAX_DIST; f.dim = (int)num("dim", -1); f.v[0] = (float)num("maxDist", 1.0);
      } else if (m.name == "MinDistDataPointsFilter") {
        only({"dim", "minDist"});
        f.type = LSGPU_FILTER_MIN_DIST; f.dim = (int)num("dim", -1); f.v[0] = (float)num("minDist", 1.0);
      } else if (m.name == "BoundingBoxDataPointsFilter") {
        only({"xMin", "xMax", "yMin", "yMax", "zMin", "zMax", "removeInside"});
        f.type = LSGPU_FILTER_BOUNDING_BOX;
        f.v[0] = (float)num("xMin", -1.0); f.v[1] = (float)num("xMax", 1.0);
        f.v[2] = (float)num("yMin", -1.0); f.v[3] = (float)num("yMax", 1.0);
        f.v[4] = (float)num("zMin", -1.0); f.v[5] = (float)num("zMax", 1.0);
        f.flag = (int)num("removeInside", 1);
      } else if (m.name == "FixStepSamplingDataPointsFilter") {
        only({"startStep", "endStep", "stepMult"});
        f.type = LSGPU_FILTER_FIX_STEP_SAMPLING;
        f.v[0] = (float)num("startStep", 10); f.v[1] = (float)num("endStep", 10); f.v[2] = (float)num("stepMult", 1);
      } else if (m.name == "RandomSamplingDataPointsFilter") {
        only({"prob"});
        f.type = LSGPU_FILTER_RANDOM_SAMPLING; f.v[0] = (float)num("prob", 0.75);
      } else if (m.name == "RemoveNaNDataPointsFilter") {
        only({});
        f.type = LSGPU_FILTER_REMOVE_NAN;
      } else if (m.name == "VoxelGridDataPointsFilter") {
        // libpointmatcher's voxel grid (include/lsgpu_icp.h, "the input filter chain"): flag = useCentroid, dim =
        // averageExistingDescriptors; the values are judged here as lsgpu_apply_point_filters judges them
        only({"vSizeX", "vSizeY", "vSizeZ", "useCentroid", "averageExistingDescriptors"});
        f.type = LSGPU_FILTER_VOXEL_GRID;
        f.v[0] = (float)num("vSizeX", 1.0); f.v[1] = (float)num("vSizeY", 1.0); f.v[2] = (float)num("vSizeZ", 1.0);
        const double uc = num("useCentroid", 1), avg = num("averageExistingDescriptors", 1);
        for (int a = 0; a < 3; ++a)
          if (!(f.v[a] > 0.f) || !std::isfinite(f.v[a])) throw ConfigError(m.name + ": vSizeX / vSizeY / vSizeZ must be finite and > 0");
        if ((uc != 0 && uc != 1) || (avg != 0 && avg != 1)) throw ConfigError(m.name + ": useCentroid and averageExistingDescriptors take 0 or 1");
        f.flag = (int)uc; f.dim = (int)avg;
      } else if (m.name == "OctreeGridDataPointsFilter") {
        // libpointmatcher's octree (include/lsgpu_icp.h, "the input filter chain"): v[0] = maxSizeByNode, v[1] =
        // maxPointByNode, dim = samplingMethod, flag = buildParallel; judged here as lsgpu_apply_point_filters judges them
        only({"buildParallel", "maxPointByNode", "maxSizeByNode", "samplingMethod"});
        f.type = LSGPU_FILTER_OCTREE_GRID;
        const double bp = num("buildParallel", 1), mp = num("maxPointByNode", 1), ms = num("maxSizeByNode", 0), sm = num("samplingMethod", 0);
        f.v[0] = (float)ms;
        if (!(f.v[0] >= 0.f) || !std::isfinite(f.v[0])) throw ConfigError(m.name + ": maxSizeByNode must be finite and >= 0");
        if (!(mp >= 1 && mp <= 16777216.0) || mp != std::floor(mp)) throw ConfigError(m.name + ": maxPointByNode must be an integer in [1, 2^24]");
        if (sm != 0 && sm != 1 && sm != 2 && sm != 3) throw ConfigError(m.name + ": samplingMethod must be 0 (FirstPts), 1 (RandomPts), 2 (Centroid) or 3 (Medoid)");
        if (bp != 0 && bp != 1) throw ConfigError(m.name + ": buildParallel must be 0 or 1");
        f.v[1] = (float)mp; f.dim = (int)sm; f.flag = (int)bp;
      } else {
        throw ConfigError("input filters: module " + m.name + " is not implemented on the HIP path");
      }
      filters_.push_back(f);
    }
    if (tail == 2) throw ConfigError("input filters: ObservationDirectionDataPointsFilter is implemented only as the pair "
                                     "ObservationDirectionDataPointsFilter, OrientNormalsDataPointsFilter directly behind SurfaceNormalDataPointsFilter");
  }
  ~DataPointsFilters() { if (h_) lsgpu_icp_destroy(h_); }
  DataPointsFilters(const DataPointsFilters&) = delete;
  DataPointsFilters& operator=(const DataPointsFilters&) = delete;
  DataPointsFilters(DataPointsFilters&& o) noexcept { *this = std::move(o); }
  DataPointsFilters& operator=(DataPointsFilters&& o) noexcept {
    if (this != &o) {
      if (h_) lsgpu_icp_destroy(h_);
      filters_ = std::move(o.filters_); h_ = o.h_; o.h_ = nullptr; device_ = o.device_; seed_ = o.seed_;
      normals_knn_ = o.normals_knn_; orient_ = o.orient_;
      for (int a = 0; a < 3; ++a) sensor_[a] = o.sensor_[a];
    }
    return *this;
  }

  size_t size() const { return filters_.size(); }
  bool empty() const { return filters_.empty() && !producesNormals(); }
  // the chain ends with SurfaceNormalDataPointsFilter: every cloud apply() leaves carries normals
  bool producesNormals() const { return normals_knn_ > 0; }
  int normalsKnn() const { return normals_knn_; }
  int normalsOrientation() const { return orient_; }   // 0: no pair, 1: towardCenter 1, 2: towardCenter 0
  const std::vector<lsgpu_point_filter>& modules() const { return filters_; }
  void setSeed(int64_t seed) { seed_ = seed; }  // >= 0: reseed the draw stream at every apply(); < 0: continue it

  // DataPointsFilters::apply: in place; throws ConvergenceError if a filter is handed an empty cloud.
  void apply(DataPoints& cloud);

 private:
  friend class ICP;   // ICP::ingestCloud runs this chain on the ICP's handle: the modules' state, the seed and the tail are these
  void applyPointModules(DataPoints& cloud, int64_t n);
  std::vector<lsgpu_point_filter> filters_;
  lsgpu_icp* h_ = nullptr;
  int device_ = 0;
  int64_t seed_ = -1;
  int normals_knn_ = 0, orient_ = 0;   // the tail: SurfaceNormalDataPointsFilter's knn (0: none), the pair's orientation
  float sensor_[3] = {0.f, 0.f, 0.f};
};

class ICP {
 public:
  ICP() { setDefault(); }
  explicit ICP(int device) : device_(device) { setDefault(); }
  ~ICP() { release(); }
  ICP(const ICP&) = delete;
  ICP& operator=(const ICP&) = delete;

  // ICP::setDefault(): RandomSampling 0.75 / SamplingSurfaceNormal knn 7 / KDTree 1,0 / TrimmedDist 0.85 /
  // PointToPlane / Counter 40 + Differential 1e-3, 1e-3, 3
  void setDefault() {
    std::memset(&mods_, 0, sizeof(mods_));
    lsgpu_icp_config_default(&mods_.chain.icp);
    lsgpu_chain_config_default(&mods_.chain.chain);
    lsgpu_shadow_config_default(&mods_.shadow);
    lsgpu_motion_config_default(&mods_.motion);
    lsgpu_cov_sampling_config_default(&mods_.cov_sampling);
    release();
  }

  // The syntax is read here (parseYaml), the modules are handed to lsgpu_chain_load_modules as text: which modules the device path
  // has, their parameters, ranges and order are the library's rule set (csrc/lsgpu_chain_loader.cpp), shared with the Python
  // facade.  Any other module is a configuration error (PointMatcher's registrar throws on unknown names as well).
  // carried: which of compute()'s clouds carry normals (LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE): the chain may then
  // read normals it has no module for, and compute(), uploadCloud() and the slot calls hand over the normals of a declared side.
  void loadFromYaml(std::istream& in, unsigned carried = 0) {
    const auto mods = parseYaml(in);
    std::vector<std::vector<lsgpu_yaml_param>> params(mods.size());
    std::vector<lsgpu_yaml_module> list(mods.size());
    for (size_t i = 0; i < mods.size(); ++i) {
      for (const auto& kv : mods[i].params) params[i].push_back({kv.first.c_str(), kv.second.c_str()});
      list[i] = {mods[i].section.c_str(), mods[i].name.c_str(), params[i].data(), (int)params[i].size(), 0};
    }
    char why[512];   // the one walk: every part of the document, under the declaration (a refusal leaves mods_ as it was)
    if (lsgpu_chain_load_modules(list.data(), (int)list.size(), carried, &mods_, why, (int)sizeof(why)) != LSGPU_OK) throw ConfigError(why);
    release();
  }
  unsigned carried() const { return mods_.carried; }
  // does a module behind the reference's section read its normals (include/lsgpu_icp.h, "carried normals", rule 3)?
  bool readsReferenceNormals() const {
    return mods_.chain.icp.error_minimizer != LSGPU_MINIMIZER_POINT_TO_POINT ||
           (mods_.chain.has_robust && mods_.chain.robust.distance_type == LSGPU_ROBUST_DIST_POINT2PLANE) ||
           (mods_.chain.has_normals && mods_.chain.normals.max_angle >= 0.f);
  }

  static void requireRigid(const TransformationParameters& T_init) {
    if (!RigidTransformation::checkParameters(T_init)) throw TransformationError("ICP::compute: the initial guess is not a rigid transformation");
  }

  // T with p_reference = T * p_reading.  Throws ConvergenceError exactly where PointMatcher would.
  TransformationParameters compute(const DataPoints& reading, const DataPoints& reference,
                                   const TransformationParameters& T_init) {
    // step 5 of ICP::compute moves the reading by T_refMean_dataIn with RigidTransformation::compute, which refuses a
    // matrix that is not rigid; neither call site corrects its guess (laser_track.cpp:489-496, incremental_estimator.cpp:
    // 92-108: only the sub-map transforms go through correctTransformationMatrix) and neither catches this exception.
    // Upstream throws at its step 5, AFTER both filters have consumed their rand() draws.  So does the C ABI
    // (lsgpu_icp_align rejects the guess behind the filters), and so does this facade: a guess that is not rigid is handed
    // to the device all the same, whose filters run and whose step 5 refuses it; only then the exception is thrown.  A
    // caller that catches it and goes on sees the draws a libpointmatcher process would see.  (Without a device there is
    // no draw stream to keep in step: the exception is thrown at once.)
    const bool rigid = RigidTransformation::checkParameters(T_init);
#ifdef LSGPU_TEST_SEAMS
    if (override_) { requireRigid(T_init); return override_(*this, reading, reference, T_init); }
#endif
    if (!rigid) {
      try { ensureHandle(); } catch (const DeviceError&) { requireRigid(T_init); }
    } else {
      ensureHandle();
    }
    const int64_t nr = reference.getNbPoints(), nq = reading.getNbPoints();
    if (nr <= 0 || nq <= 0) { requireRigid(T_init); throw ConvergenceError("empty cloud"); }
    // ICP::compute steps 1-7 on the device: referenceDataPointsFilters, centring + grid,
    // readingDataPointsFilters, the loop (lsgpu_icp_compute)
    lsgpu_chain_config chain = mods_.chain.chain;
    chain.seed = seed_;
    TransformationParameters T = T_init;
    // the normals of a side travel iff loadFromYaml declared that side as carrying some
    const float* rd_n = carriedNormals(reading, LSGPU_CARRIED_READING);
    const float* ref_n = carriedNormals(reference, LSGPU_CARRIED_REFERENCE);
    if ((mods_.carried & LSGPU_CARRIED_REFERENCE) && !ref_n && readsReferenceNormals() && mods_.chain.chain.ssn_knn == 0 && mods_.chain.chain.sn_knn == 0)
      throw ConfigError("ICP::compute: the reference was declared to carry normals and carries none, and the chain reads them");
    const int rc = mods_.carried ? lsgpu_icp_compute_normals(h_, reading.features.data(), rd_n, nq, reference.features.data(), ref_n, nr,
                                                        T_init.data(), &chain, T.data(), &stats_)
                            : lsgpu_icp_compute(h_, reading.features.data(), nq, reference.features.data(), nr, T_init.data(),
                                                &chain, T.data(), &stats_);
    if (!rigid) requireRigid(T_init);          // (rc is LSGPU_BAD_ARG from step 5, the filters have run)
    check(rc, mods_.carried ? "lsgpu_icp_compute_normals" : "lsgpu_icp_compute");
#ifdef LSGPU_TEST_SEAMS
    if (observer_) observer_(*this, reading, reference, T_init, T);
#endif
    return T;
  }

  // ---- scans kept in HBM: upload once, match many times
  // Slots live in the handle; loadFromYaml / setDefault drop them (generation() changes).
  void uploadCloud(int slot, const DataPoints& cloud) {
    ensureHandle();
    // (a stored scan serves as the reading once and as a sub-map member afterwards: its normals travel if either side is declared)
    const float* nrm = carriedNormals(cloud, LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE);
    if (nrm) check(lsgpu_cloud_upload_normals(h_, slot, cloud.features.data(), nrm, cloud.getNbPoints()), "lsgpu_cloud_upload_normals");
    else check(lsgpu_cloud_upload(h_, slot, cloud.features.data(), cloud.getNbPoints()), "lsgpu_cloud_upload");
    ++traffic_.uploads;
  }
  // filters.apply(cloud) + uploadCloud(slot, cloud) with the raw scan crossing to the device once (lsgpu_cloud_ingest): the
  // chain's point modules and its normals tail run on THIS handle, the kept cloud stays in `slot` with its normals and comes
  // back into `cloud` -- features, normals, `filters`' sampling state, seed and draws as apply() leaves them, its exception
  // classes and texts.  Three cases go the old way, apply() then uploadCloud(): an empty chain; a cloud that arrives with
  // normals and a chain without a normals tail (the tagged path, with its VoxelGrid / Octree refusals); a chain with a tail
  // under a loadFromYaml that declared no side as carrying normals (uploadCloud stores no normals then, an ingest would).
  void ingestCloud(int slot, DataPoints& cloud, DataPointsFilters& filters) {
    const bool tail = filters.producesNormals();
    if (filters.empty() || (!tail && !cloud.normals.empty()) ||
        (tail && !(mods_.carried & (LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE)))) {
      filters.apply(cloud);
      uploadCloud(slot, cloud);
      return;
    }
    ensureHandle();
    if (tail) cloud.normals.clear();   // (a cloud that arrives with normals has them overwritten)
    const int64_t n = cloud.getNbPoints();
    std::vector<float> out((size_t)std::max<int64_t>(n, 1) * 4), nrm(tail ? (size_t)std::max<int64_t>(n, 1) * 3 : 0);
    int64_t m = 0;
    const int rc = lsgpu_cloud_ingest(h_, slot, filters.filters_.data(), (int)filters.filters_.size(), cloud.features.data(), n,
                                      filters.seed_, filters.normals_knn_, filters.orient_, filters.sensor_, out.data(),
                                      tail ? nrm.data() : nullptr, &m);
    if (rc != LSGPU_OK) {
      const std::string why = lsgpu_last_error(h_);
      const bool in_tail = why.compare(0, 17, "reading_normals: ") == 0;
      if (rc == LSGPU_NO_CONVERGENCE || (in_tail && m <= 0)) throw ConvergenceError("no points to filter");
      if (rc == LSGPU_BAD_CONFIG) throw ConfigError("input filters: " + why);
      throw DeviceError(std::string(in_tail ? "lsgpu_icp_reading_normals: " : "lsgpu_apply_point_filters: ") + lsgpu_strerror(rc) + " [" + why + "]");
    }
    out.resize((size_t)m * 4);
    cloud.features.swap(out);
    if (tail) { nrm.resize((size_t)m * 3); cloud.normals.swap(nrm); }
    ++traffic_.ingests;
  }
  // how scans reached the slots of this ICP so far:uploadCloud / computeCloudsUploading copies, ingestCloud runs on the device
  struct SlotTraffic { uint64_t uploads = 0, ingests = 0; };
  SlotTraffic slotTraffic() const { return traffic_; }
  void releaseCloud(int slot) { if (h_) lsgpu_cloud_release(h_, slot); }
  bool hasCloud(int slot) {
    if (!h_) return false;
    int64_t n = -1;
    lsgpu_cloud_size(h_, slot, &n);
    return n >= 0;
  }
  unsigned generation() const { return generation_; }
  // compute() with reading = slot `reading` and reference = concat_i(T_i * slot refs[i]) assembled on the
  // device: what localScanToSubMap builds on the host at laser_track.cpp:474-486
  TransformationParameters computeClouds(int reading, const std::vector<int>& refs,
                                         const std::vector<TransformationParameters>& ref_T,
                                         const TransformationParameters& T_init) {
    const bool rigid = RigidTransformation::checkParameters(T_init);   // (refused at step 5, behind the filters: see compute())
    if (!rigid) {
      try { ensureHandle(); } catch (const DeviceError&) { requireRigid(T_init); }
    } else {
      ensureHandle();
    }
    if (refs.size() != ref_T.size()) throw std::logic_error("one transform per reference cloud");
    lsgpu_chain_config chain = mods_.chain.chain;
    chain.seed = seed_;
    std::vector<float> flat(16 * refs.size());
    for (size_t i = 0; i < refs.size(); ++i) std::memcpy(&flat[16 * i], ref_T[i].data(), 16 * sizeof(float));
    TransformationParameters T = T_init;
    const int rc = lsgpu_icp_compute_clouds(h_, reading, refs.data(), flat.data(), (int)refs.size(), T_init.data(), &chain,
                                            T.data(), &stats_);
    if (!rigid) requireRigid(T_init);
    check(rc, "lsgpu_icp_compute_clouds");
    return T;
  }

  // uploadCloud(reading, cloud) + computeClouds(reading, ...) in one call: the new scan crosses PCIe while the sub-map is
  // assembled and filtered (lsgpu_icp_compute_clouds_upload).  The slot holds the scan afterwards, also when this throws.
  TransformationParameters computeCloudsUploading(int reading, const DataPoints& cloud, const std::vector<int>& refs,
                                                  const std::vector<TransformationParameters>& ref_T,
                                                  const TransformationParameters& T_init) {
    const bool rigid = RigidTransformation::checkParameters(T_init);   // (refused at step 5, behind the filters: see compute())
    if (!rigid) {
      try { ensureHandle(); } catch (const DeviceError&) { requireRigid(T_init); }
    } else {
      ensureHandle();
    }
    if (refs.size() != ref_T.size()) throw std::logic_error("one transform per reference cloud");
    lsgpu_chain_config chain = mods_.chain.chain;
    chain.seed = seed_;
    std::vector<float> flat(16 * refs.size());
    for (size_t i = 0; i < refs.size(); ++i) std::memcpy(&flat[16 * i], ref_T[i].data(), 16 * sizeof(float));
    TransformationParameters T = T_init;
    const float* nrm = carriedNormals(cloud, LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE);
    const int rc = nrm ? lsgpu_icp_compute_clouds_upload_normals(h_, reading, cloud.features.data(), nrm, cloud.getNbPoints(), refs.data(),
                                                                 flat.data(), (int)refs.size(), T_init.data(), &chain, T.data(), &stats_)
                       : lsgpu_icp_compute_clouds_upload(h_, reading, cloud.features.data(), cloud.getNbPoints(), refs.data(),
                                                         flat.data(), (int)refs.size(), T_init.data(), &chain, T.data(), &stats_);
    if (!rigid) requireRigid(T_init);
    ++traffic_.uploads;   // (the slot holds the scan whatever the registration's outcome)
    check(rc, nrm ? "lsgpu_icp_compute_clouds_upload_normals" : "lsgpu_icp_compute_clouds_upload");
    return T;
  }

  // >= 0: reseed the filters' draw stream at every compute() (reproducible runs); < 0: continue it
  void setSeed(int64_t seed) { seed_ = seed; }
  int64_t seed() const { return seed_; }

#ifdef LSGPU_TEST_SEAMS
  // (compiled only into the parity-test drivers, tests/cpp/*: -DLSGPU_TEST_SEAMS; the shipped header has no hook)
  // Test seam: replaces compute() by another implementation of the same call (the parity tests inject the CPU
  // oracle here, so that LaserTrack / IncrementalEstimator run unchanged on either ICP).  Never set by the
  // product; with an override in place nothing touches the GPU (no handle is created).
  using ComputeOverride = std::function<TransformationParameters(const ICP&, const DataPoints& reading,
                                                                 const DataPoints& reference,
                                                                 const TransformationParameters& T_init)>;
  void setComputeOverride(ComputeOverride f) { override_ = std::move(f); }
  // Test seam: called after every successful device compute() with its inputs and its result (the parity tests run
  // the CPU oracle on exactly the clouds the facade handed to the device).  Never set by the product.
  using ComputeObserver = std::function<void(const ICP&, const DataPoints& reading, const DataPoints& reference,
                                             const TransformationParameters& T_init, const TransformationParameters& T)>;
  void setComputeObserver(ComputeObserver f) { observer_ = std::move(f); }
  bool hasComputeObserver() const { return (bool)observer_; }
  // the resident-scan path (computeClouds) never sees the assembled sub-map on the host; LaserTrack assembles it for the
  // observer's benefit when (and only when) one is set
  void notifyObserver(const DataPoints& reading, const DataPoints& reference, const TransformationParameters& T_init,
                      const TransformationParameters& T) const { if (observer_) observer_(*this, reading, reference, T_init, T); }
  bool hasComputeOverride() const { return (bool)override_; }
#else
  bool hasComputeOverride() const { return false; }
#endif

  // Steps 2-7 on already filtered clouds (device or host pointers).
  TransformationParameters computeFiltered(const float* reading_xyz1, int64_t nq, const float* ref_xyz1,
                                           const float* ref_normals, int64_t nr,
                                           const TransformationParameters& T_init) {
    ensureHandle();
    check(lsgpu_icp_set_reference(h_, ref_xyz1, ref_normals, nr), "lsgpu_icp_set_reference");
    TransformationParameters T = T_init;
    check(lsgpu_icp_align(h_, reading_xyz1, nq, T_init.data(), T.data(), &stats_), "lsgpu_icp_align");
    return T;
  }

  // PointToPlaneWithCovErrorMinimizer (errorMinimizer->getCovariance() upstream): the quality record of the last compute --
  // the 6x6 covariance (row major; x y z, then the rotations about x y z), the squared plane residual, the pair count and
  // the used ratio.  ConfigError if the chain does not name the module; ConvergenceError before a successful compute or
  // for a singular H.
  lsgpu_icp_quality quality() {
    ensureHandle();
    lsgpu_icp_quality q;
    check(lsgpu_icp_get_quality(h_, &q), "lsgpu_icp_get_quality");
    return q;
  }
  std::array<double, 36> covariance() {
    const lsgpu_icp_quality q = quality();
    std::array<double, 36> c;
    std::memcpy(c.data(), q.covariance, sizeof(q.covariance));
    return c;
  }
  // sensorStdDev of the loaded chain's PointToPlaneWithCovErrorMinimizer; false: the chain does not name the module
  bool covarianceConfig(float* sensor_std_dev) const { return lsgpu_loaded_chain_covariance(&mods_.chain, sensor_std_dev) != 0; }

  // maxDensity of the loaded chain's MaxDensityDataPointsFilter (behind SurfaceNormalDataPointsFilter keepDensities 1 in the
  // reference section); false: the chain does not name the module
  bool maxDensityConfig(float* max_density) const { return lsgpu_loaded_chain_max_density(&mods_.chain, max_density) != 0; }

  const lsgpu_icp_stats& lastStats() const { return stats_; }
  const lsgpu_icp_config& config() const { return mods_.chain.icp; }
  lsgpu_icp* handle() { ensureHandle(); return h_; }  // the C-ABI handle (device conversions of ros_msgs.hpp)
  float readingSamplingProb() const { return mods_.chain.chain.reading_prob; }
  int surfaceNormalKnn() const { return mods_.chain.chain.ssn_knn; }      // SamplingSurfaceNormalDataPointsFilter's knn (0: no such module)
  int referenceNormalKnn() const { return mods_.chain.chain.sn_knn; }     // SurfaceNormalDataPointsFilter's knn (0: no such module)
  float surfaceNormalRatio() const { return mods_.chain.chain.ssn_ratio; }
  const lsgpu_robust_config* robustFilter() const { return mods_.chain.has_robust ? &mods_.chain.robust : nullptr; }   // RobustOutlierFilter (nullptr: no such module)
  // SurfaceNormalOutlierFilter / reading normals / the orientation pairs (nullptr: none of these modules)
  const lsgpu_normals_config* normalsConfig() const { return mods_.chain.has_normals ? &mods_.chain.normals : nullptr; }
  // the cut modules of the two filter sections (nullptr: none)
  const lsgpu_chain_cuts* chainCuts() const { return mods_.cuts.n_reading || mods_.cuts.n_reference ? &mods_.cuts : nullptr; }
  // ShadowDataPointsFilter's eps of the two filter sections (nullptr: no such module; an eps < 0: none on that side)
  const lsgpu_shadow_config* shadowConfig() const { return mods_.shadow.reading_eps >= 0.f || mods_.shadow.reference_eps >= 0.f ? &mods_.shadow : nullptr; }
  // CovarianceSamplingDataPointsFilter's nbSample / torqueNorm of the two filter sections (nullptr: no such module; nbSample 0: none on that side)
  const lsgpu_cov_sampling_config* covSamplingConfig() const { return mods_.cov_sampling.reading_nb_sample > 0 || mods_.cov_sampling.reference_nb_sample > 0 ? &mods_.cov_sampling : nullptr; }
  // PointToPlaneErrorMinimizer's force2D / force4DOF and BoundTransformationChecker (nullptr: neither)
  const lsgpu_motion_config* motionConfig() const { return mods_.motion.dof || mods_.motion.bound ? &mods_.motion : nullptr; }
  const lsgpu_loaded_chain& loadedChain() const { return mods_.chain; }
  const lsgpu_chain_modules& modules() const { return mods_; }   // the whole record, as lsgpu_icp_set_modules takes it

 private:
  using Module = detail::YamlModule;
  static std::string trim(const std::string& s) { return detail::trim(s); }
  static void parseInline(const std::string& body, std::map<std::string, std::string>* out) { detail::parseInline(body, out); }
  // The YAML subset libpointmatcher configurations use: top-level `section:`, module either as a list
  // item `- Name:` / `- Name` or as a mapping `Name:` / scalar `section: Name`, parameters as an
  // indented `key: value` block or an inline `{...}` map; `#` comments.
  static std::vector<Module> parseYaml(std::istream& in) {
    std::vector<Module> mods;
    std::string line, section;
    int mod_indent = -1;
    while (std::getline(in, line)) {
      const size_t hash = line.find('#');
      if (hash != std::string::npos) line = line.substr(0, hash);
      if (trim(line).empty()) continue;
      int indent = 0;
      while (indent < (int)line.size() && line[indent] == ' ') ++indent;
      std::string t = trim(line);
      bool item = false;
      if (t[0] == '-') { item = true; t = trim(t.substr(1)); }
      const size_t c = t.find(':');
      std::string key = trim(c == std::string::npos ? t : t.substr(0, c));
      std::string val = c == std::string::npos ? "" : trim(t.substr(c + 1));
      if (indent == 0 && !item) {  // section
        section = key;
        mod_indent = -1;
        if (!val.empty() && val[0] != '{') { mods.push_back({section, val, {}}); }
        continue;
      }
      if (section.empty()) throw ConfigError("yaml: content before the first section");
      const bool is_param = mod_indent >= 0 && indent > mod_indent && !item;
      if (is_param) {
        mods.back().params[key] = val;
      } else {  // a module
        Module m{section, key, {}};
        if (!val.empty() && val.front() == '{' && val.back() == '}') parseInline(val.substr(1, val.size() - 2), &m.params);
        mods.push_back(m);
        mod_indent = indent;
      }
    }
    return mods;
  }

  void ensureHandle() {
    if (h_) return;
    const int rc = lsgpu_icp_create(&mods_.chain.icp, device_, &h_);
    if (rc == LSGPU_BAD_CONFIG) throw ConfigError("lsgpu_icp_create: bad configuration");
    if (rc != LSGPU_OK) throw DeviceError("lsgpu_icp_create failed (no ROCm GPU visible?)");
    if (lsgpu_icp_set_modules(h_, &mods_) != LSGPU_OK) {   // all of the chain's modules, or none and the refusal
      const std::string msg = std::string("lsgpu_icp_set_modules: ") + lsgpu_last_error(h_);
      release();
      throw ConfigError(msg);
    }
  }
  void release() { if (h_) { lsgpu_icp_destroy(h_); h_ = nullptr; ++generation_; } }
  // the cloud's normals if one of `sides` was declared at load and the cloud carries one normal per point, else nullptr
  const float* carriedNormals(const DataPoints& cloud, unsigned sides) const {
    if (!(mods_.carried & sides) || cloud.normals.empty() || cloud.normals.size() != (size_t)cloud.getNbPoints() * 3) return nullptr;
    return cloud.normals.data();
  }
  void check(int rc, const char* what) {
    if (rc == LSGPU_OK) return;
    const std::string msg = std::string(what) + ": " + lsgpu_strerror(rc) + " [" + lsgpu_last_error(h_) + "]";
    if (rc == LSGPU_NO_CONVERGENCE) throw ConvergenceError(msg);
    if (rc == LSGPU_BAD_CONFIG) throw ConfigError(msg);
    throw DeviceError(msg);
  }

  int device_ = 0;
  // what loadFromYaml / setDefault left: the handle's config, the filters of compute(), every module of the chain and which of
  // compute()'s clouds were declared as carrying normals (lsgpu_chain_load_modules)
  lsgpu_chain_modules mods_{};
  lsgpu_icp* h_ = nullptr;
  lsgpu_icp_stats stats_{};
  int64_t seed_ = -1;
  unsigned generation_ = 0;
  SlotTraffic traffic_;
#ifdef LSGPU_TEST_SEAMS
  ComputeOverride override_;
  ComputeObserver observer_;
#endif
};

inline void DataPointsFilters::apply(DataPoints& cloud) {
  if (filters_.empty() && !producesNormals()) return;
  if (producesNormals()) cloud.normals.clear();   // (a cloud that arrives with normals has them overwritten)
  // VoxelGridDataPointsFilter writes new points: the tag it hands on is the voxel's first point's, so the normal picked
  // further down is that point's (averageExistingDescriptors 0).  Averaging the descriptors of a voxel is not implemented.
  if (!cloud.normals.empty())
    for (const auto& f : filters_)
      if (f.type == LSGPU_FILTER_VOXEL_GRID && f.dim != 0)
        throw ConfigError("VoxelGridDataPointsFilter: averageExistingDescriptors 1 on a cloud with descriptors is not implemented "
                          "(set averageExistingDescriptors: 0 to keep the first point's)");
  // OctreeGridDataPointsFilter likewise: FirstPts, RandomPts and Medoid return an input point, whose tag picks its normal;
  // Centroid would have to average the leaf's descriptors.
  if (!cloud.normals.empty())
    for (const auto& f : filters_)
      if (f.type == LSGPU_FILTER_OCTREE_GRID && f.dim == 2)
        throw ConfigError("OctreeGridDataPointsFilter: samplingMethod 2 (Centroid) on a cloud with descriptors is not implemented "
                          "(averaging descriptors; samplingMethod 0, 1 and 3 keep the chosen point's)");
  if (!h_) {
    lsgpu_icp_config c;
    lsgpu_icp_config_default(&c);
    if (lsgpu_icp_create(&c, device_, &h_) != LSGPU_OK) throw DeviceError("lsgpu_icp_create failed (no ROCm GPU visible?)");
  }
  const int64_t n = cloud.getNbPoints();
  if (!filters_.empty()) applyPointModules(cloud, n);
  if (!producesNormals()) return;
  // the tail, on what the point modules kept: SurfaceNormalDataPointsFilter and the orientation pair
  const int64_t kept = cloud.getNbPoints();
  if (kept <= 0) throw ConvergenceError("no points to filter");
  cloud.normals.assign((size_t)kept * 3, 0.f);
  const int rc = lsgpu_icp_reading_normals(h_, cloud.features.data(), kept, normals_knn_, orient_, sensor_, cloud.normals.data());
  if (rc != LSGPU_OK) {
    cloud.normals.clear();
    throw DeviceError(std::string("lsgpu_icp_reading_normals: ") + lsgpu_strerror(rc) + " [" + lsgpu_last_error(h_) + "]");
  }
}

inline void DataPointsFilters::applyPointModules(DataPoints& cloud, int64_t n) {
  std::vector<float> out((size_t)std::max<int64_t>(n, 1) * 4);
  int64_t m = 0;
  // A cloud with descriptors (normals): the device filters look at x, y, z only and carry the 4th component through, so
  // the point's index travels in it and the descriptor columns of the survivors are picked afterwards -- the filters keep
  // or drop whole columns, features and descriptors alike, as upstream's do.
  const bool tagged = !cloud.normals.empty();
  std::vector<float> in_tagged;
  if (tagged) {
    in_tagged = cloud.features;
    for (int64_t i = 0; i < n; ++i) { const uint32_t tag = (uint32_t)i; std::memcpy(&in_tagged[(size_t)(4 * i + 3)], &tag, 4); }
  }
  const int rc = lsgpu_apply_point_filters(h_, filters_.data(), (int)filters_.size(), tagged ? in_tagged.data() : cloud.features.data(),
                                           n, seed_, out.data(), &m);
  if (rc == LSGPU_NO_CONVERGENCE) throw ConvergenceError("no points to filter");
  if (rc == LSGPU_BAD_CONFIG) throw ConfigError(std::string("input filters: ") + lsgpu_last_error(h_));
  if (rc != LSGPU_OK) throw DeviceError(std::string("lsgpu_apply_point_filters: ") + lsgpu_strerror(rc) + " [" + lsgpu_last_error(h_) + "]");
  out.resize((size_t)m * 4);
  if (tagged) {
    std::vector<float> nrm((size_t)m * 3);
    for (int64_t j = 0; j < m; ++j) {
      uint32_t tag;
      std::memcpy(&tag, &out[(size_t)(4 * j + 3)], 4);
      out[(size_t)(4 * j + 3)] = cloud.features[(size_t)(4 * (int64_t)tag + 3)];
      for (int d = 0; d < 3; ++d) nrm[(size_t)(3 * j + d)] = cloud.normals[(size_t)(3 * (int64_t)tag + d)];
    }
    cloud.normals.swap(nrm);
  }
  cloud.features.swap(out);
}

}  // namespace laser_slam_amd
