// lsgpu_icp_shim.hpp -- the drop-in a laser_slam maintainer puts where `PointMatcher::ICP icp_` and
// `PointMatcher::DataPointsFilters input_filters_` are declared today:
//     laser_slam/include/laser_slam/laser_track.hpp:217,220        incremental_estimator.hpp:70
//   - PointMatcher::ICP icp_;                    + LsgpuICP<PointMatcher> icp_;
//   - PointMatcher::DataPointsFilters input_filters_;   + LsgpuDataPointsFilters<PointMatcher> input_filters_;
// Nothing else changes: loadFromYaml / setDefault / compute keep their signatures (laser_track.cpp:17,20,496,
// incremental_estimator.cpp:108), ConvergenceError is the PointMatcher one (caught at laser_track.cpp:499),
// input_filters_ = LsgpuDataPointsFilters<PointMatcher>(ifs) and .apply(scan.scan) read as before (:27,:81,:146).
//
// The header is a template over the PointMatcher type so that the SAME code is compiled and tested in this
// repository against the dependency-free mirror types (LsgpuMirrorPM below, tests/cpp/shim_check.cpp) and compiles
// against the real `PointMatcher<float>` (Eigen matrices) through LsgpuCloudTraits: the only operations it needs from
// a cloud are "pointer to the (dim+1) x N column-major features", "number of points", "has descriptors" and "keep these
// columns".
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <istream>
#include <stdexcept>
#include <string>
#include <vector>

#include "laser_slam_amd/icp.hpp"   // YAML subset parser + module -> device configuration (no GPU touched by parsing)
#include "lsgpu_icp.h"

// ---- how the shim looks at a cloud.  Primary template: the real libpointmatcher (Eigen) types.
template <class PM>
struct LsgpuCloudTraits {
  using DataPoints = typename PM::DataPoints;
  static const float* features(const DataPoints& d) { return d.features.data(); }      // 4 x N, column major
  static int64_t size(const DataPoints& d) { return (int64_t)d.features.cols(); }
  static bool hasDescriptors(const DataPoints& d) { return d.descriptors.cols() > 0; }
  // The normals the cloud carries, 3 floats per point: the rows labelled `normals` of `descriptors` (any other descriptor
  // stays where it is).  false, and *out empty: the cloud carries none
  static bool normals(const DataPoints& d, std::vector<float>* out) {
    out->clear();
    if (d.descriptors.cols() == 0 || !d.descriptorExists("normals")) return false;
    const auto rows = d.getDescriptorViewByName("normals");
    if (rows.rows() != 3) return false;
    out->resize((size_t)rows.cols() * 3);
    for (Eigen_Index i = 0; i < (Eigen_Index)rows.cols(); ++i)
      for (int r = 0; r < 3; ++r) (*out)[3 * (size_t)i + r] = rows(r, i);
    return true;
  }
  // keep the listed columns (ascending) of features and of every descriptor, drop the others
  static void keepColumns(DataPoints& d, const std::vector<int64_t>& cols) {
    for (size_t j = 0; j < cols.size(); ++j) {
      if ((int64_t)j == cols[j]) continue;
      d.features.col((Eigen_Index)j) = d.features.col((Eigen_Index)cols[j]);
      if (d.descriptors.cols() > 0) d.descriptors.col((Eigen_Index)j) = d.descriptors.col((Eigen_Index)cols[j]);
    }
    d.features.conservativeResize(d.features.rows(), (Eigen_Index)cols.size());
    if (d.descriptors.cols() > 0) d.descriptors.conservativeResize(d.descriptors.rows(), (Eigen_Index)cols.size());
  }
  // the cloud's features become these m points (x, y, z, pad per point); for a cloud without descriptors
  static void setFeatures(DataPoints& d, const float* xyz1, int64_t m) {
    d.features.conservativeResize(d.features.rows(), (Eigen_Index)m);
    if (m) std::memcpy(d.features.data(), xyz1, (size_t)m * 16);
  }
  // the 6 x 6 matrix errorMinimizer->getCovariance() returns (PointMatcher<float>::Matrix) from 36 doubles, row major
  using Matrix = typename PM::Matrix;
  static Matrix matrix6(const double* c) {
    Matrix m(6, 6);
    for (int r = 0; r < 6; ++r)
      for (int k = 0; k < 6; ++k) m(r, k) = (float)c[r * 6 + k];
    return m;
  }
 private:
  using Eigen_Index = decltype(std::declval<DataPoints>().features.cols());
};

// ---- the in-tree mirror types (what the tests instantiate the shim with)
struct LsgpuMirrorPM {
  using DataPoints = laser_slam_amd::DataPoints;
  using TransformationParameters = laser_slam_amd::TransformationParameters;
  using ConvergenceError = laser_slam_amd::ConvergenceError;
};
template <>
struct LsgpuCloudTraits<LsgpuMirrorPM> {
  using DataPoints = laser_slam_amd::DataPoints;
  static const float* features(const DataPoints& d) { return d.features.data(); }
  static int64_t size(const DataPoints& d) { return d.getNbPoints(); }
  static bool hasDescriptors(const DataPoints& d) { return !d.normals.empty(); }
  static bool normals(const DataPoints& d, std::vector<float>* out) {   // the vector itself
    *out = d.normals;
    return !out->empty();
  }
  static void keepColumns(DataPoints& d, const std::vector<int64_t>& cols) {
    const bool nrm = !d.normals.empty();
    for (size_t j = 0; j < cols.size(); ++j) {
      if ((int64_t)j == cols[j]) continue;
      std::memcpy(&d.features[4 * j], &d.features[4 * (size_t)cols[j]], 4 * sizeof(float));
      if (nrm) std::memcpy(&d.normals[3 * j], &d.normals[3 * (size_t)cols[j]], 3 * sizeof(float));
    }
    d.features.resize(4 * cols.size());
    if (nrm) d.normals.resize(3 * cols.size());
  }
  static void setFeatures(DataPoints& d, const float* xyz1, int64_t m) { d.features.assign(xyz1, xyz1 + 4 * (size_t)m); }
  using Matrix = std::array<float, 36>;   // row major
  static Matrix matrix6(const double* c) {
    Matrix m;
    for (int i = 0; i < 36; ++i) m[i] = (float)c[i];
    return m;
  }
};

template <class PM> class LsgpuDataPointsFilters;

// ---- PointMatcher::ICP stand-in
template <class PM>
class LsgpuICP {
 public:
  using DataPoints = typename PM::DataPoints;
  using TransformationParameters = typename PM::TransformationParameters;
  using Traits = LsgpuCloudTraits<PM>;

  explicit LsgpuICP(int device = 0) : device_(device) { setDefault(); }
  ~LsgpuICP() { reset(); }
  LsgpuICP(const LsgpuICP&) = delete;
  LsgpuICP& operator=(const LsgpuICP&) = delete;

  void setDefault() {                                   // laser_track.cpp:20
    laser_slam_amd::ICP parsed;                         // == ICP::setDefault() values
    take(parsed);
  }
  // carried: which of compute()'s clouds carry a `normals` descriptor that the chain may read without a module of its own
  // (LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE; include/lsgpu_icp.h, "carried normals"): the input filters computed them
  void loadFromYaml(std::istream& in, unsigned carried = 0) {   // laser_track.cpp:17
    laser_slam_amd::ICP parsed;
    try {
      parsed.loadFromYaml(in, carried);                        // the module chain of icp_default.yaml; anything else throws
    } catch (const laser_slam_amd::ConfigError& e) {
      throw std::runtime_error(std::string("LsgpuICP::loadFromYaml: ") + e.what());   // PointMatcher: InvalidModuleType
    }
    take(parsed);
  }
  void setSeed(int64_t seed) { seed_ = seed; }          // >= 0: reproducible filter draws per compute()

  // T with p_reference = T * p_reading (laser_track.cpp:496, incremental_estimator.cpp:108).  The whole chain runs on
  // the device: reference filter, centring + grid, reading filter, the loop.  features are (dim+1) x N column major ==
  // x,y,z,1 per point and TransformationParameters is a 4x4 column-major float matrix: both are passed as they are.
  TransformationParameters compute(const DataPoints& reading, const DataPoints& reference,
                                   const TransformationParameters& T_init) {
    ensureHandle();
    lsgpu_chain_config chain = mods_.chain.chain;
    chain.seed = seed_;
    TransformationParameters T = T_init;
    // the normals of a side travel iff loadFromYaml declared that side
    const bool rd_n = (mods_.carried & LSGPU_CARRIED_READING) && Traits::normals(reading, &rd_normals_) && (int64_t)rd_normals_.size() == 3 * Traits::size(reading);
    const bool ref_n = (mods_.carried & LSGPU_CARRIED_REFERENCE) && Traits::normals(reference, &ref_normals_) && (int64_t)ref_normals_.size() == 3 * Traits::size(reference);
    const int rc = mods_.carried ? lsgpu_icp_compute_normals(h_, Traits::features(reading), rd_n ? rd_normals_.data() : nullptr, Traits::size(reading),
                                                        Traits::features(reference), ref_n ? ref_normals_.data() : nullptr, Traits::size(reference),
                                                        T_init.data(), &chain, T.data(), &stats_)
                            : lsgpu_icp_compute(h_, Traits::features(reading), Traits::size(reading), Traits::features(reference),
                                                Traits::size(reference), T_init.data(), &chain, T.data(), &stats_);
    if (rc == LSGPU_NO_CONVERGENCE) throw typename PM::ConvergenceError(lsgpu_last_error(h_));
    if (rc != LSGPU_OK) throw std::runtime_error(std::string("LsgpuICP::compute: ") + lsgpu_strerror(rc) + " [" + lsgpu_last_error(h_) + "]");
    return T;
  }
  const lsgpu_icp_stats& lastStats() const { return stats_; }

  // ---- scans kept on the device (include/lsgpu_icp.h, lsgpu_cloud_*): not PointMatcher calls, for a LaserTrack that keeps
  // its recent scans in slots of this handle (lsgpu_icp_compute_clouds through handle()).
  // uploadCloud: the cloud's points into `slot`, with its `normals` descriptor if loadFromYaml declared a side as carrying some.
  void uploadCloud(int slot, const DataPoints& cloud) {
    ensureHandle();
    const bool nrm = mods_.carried && Traits::normals(cloud, &rd_normals_) && (int64_t)rd_normals_.size() == 3 * Traits::size(cloud);
    const int rc = lsgpu_cloud_upload_normals(h_, slot, Traits::features(cloud), nrm ? rd_normals_.data() : nullptr, Traits::size(cloud));
    if (rc != LSGPU_OK) throw std::runtime_error(std::string("LsgpuICP::uploadCloud: ") + lsgpu_strerror(rc) + " [" + lsgpu_last_error(h_) + "]");
  }
  // filters.apply(cloud) + uploadCloud(slot, cloud) with one upload of the raw scan (lsgpu_cloud_ingest): the chain runs on
  // this handle, the kept cloud stays in `slot` and its features come back into `cloud`; draws, seed and FixStepSampling's
  // state move as apply() moves them.  A cloud with descriptors goes the old way (apply() thins their columns on the host
  // through a tag in the pad row, which must not reach the slot), and so does an empty chain.
  void ingestCloud(int slot, DataPoints& cloud, LsgpuDataPointsFilters<PM>& filters) {
    if (filters.filters_.empty() || Traits::hasDescriptors(cloud)) {
      filters.apply(cloud);
      uploadCloud(slot, cloud);
      return;
    }
    const int64_t n = Traits::size(cloud);
    if (n == 0) throw typename PM::ConvergenceError("no points to filter");
    ensureHandle();
    std::vector<float> out((size_t)n * 4);
    int64_t m = 0;
    const int rc = lsgpu_cloud_ingest(h_, slot, filters.filters_.data(), (int)filters.filters_.size(), Traits::features(cloud), n,
                                      filters.seed_, 0, 0, nullptr, out.data(), nullptr, &m);
    if (rc == LSGPU_NO_CONVERGENCE) throw typename PM::ConvergenceError("no points to filter");
    if (rc != LSGPU_OK) throw std::runtime_error(std::string("LsgpuDataPointsFilters::apply: ") + lsgpu_strerror(rc));
    Traits::setFeatures(cloud, out.data(), m);
  }
  int64_t cloudSize(int slot) {   // -1: the slot holds nothing
    int64_t n = -1;
    if (h_) lsgpu_cloud_size(h_, slot, &n);
    return n;
  }
  lsgpu_icp* handle() { ensureHandle(); return h_; }
  // icp.errorMinimizer->getCovariance() becomes icp.getCovariance(): the 6 x 6 covariance of the last compute() of a chain
  // with PointToPlaneWithCovErrorMinimizer, in the PointMatcher matrix type (float).  Throws ConvergenceError before a
  // successful compute() and for a singular H, std::runtime_error if the chain does not name the module.
  typename Traits::Matrix getCovariance() {
    lsgpu_icp_quality q;
    const int rc = h_ ? lsgpu_icp_get_quality(h_, &q) : (lsgpu_loaded_chain_covariance(&mods_.chain, nullptr) ? LSGPU_NO_CONVERGENCE : LSGPU_BAD_CONFIG);
    if (rc == LSGPU_NO_CONVERGENCE) throw typename PM::ConvergenceError(h_ ? lsgpu_last_error(h_) : "getCovariance: no compute() yet");
    if (rc != LSGPU_OK) throw std::runtime_error(std::string("LsgpuICP::getCovariance: ") + lsgpu_strerror(rc) + (h_ ? std::string(" [") + lsgpu_last_error(h_) + "]" : std::string()));
    return Traits::matrix6(q.covariance);
  }

 private:
  void take(const laser_slam_amd::ICP& parsed) {
    mods_ = parsed.modules();
    reset();
  }
  void reset() { if (h_) { lsgpu_icp_destroy(h_); h_ = nullptr; } }
  void ensureHandle() {
    if (h_) return;
    if (lsgpu_icp_create(&mods_.chain.icp, device_, &h_) != LSGPU_OK)
      throw std::runtime_error("LsgpuICP: lsgpu_icp_create failed (no ROCm GPU visible?)");
    if (lsgpu_icp_set_modules(h_, &mods_) != LSGPU_OK) {   // every module of the loaded chain, or none and the refusal
      const std::string why = lsgpu_last_error(h_);
      reset();
      throw std::runtime_error("LsgpuICP: lsgpu_icp_set_modules: " + why);
    }
  }
  int device_ = 0;
  lsgpu_chain_modules mods_{};                          // the loaded chain: its configs, every module, the declaration of carried normals
  lsgpu_icp* h_ = nullptr;
  lsgpu_icp_stats stats_{};
  int64_t seed_ = -1;
  std::vector<float> rd_normals_, ref_normals_;         // the normals handed to the last compute()
};

// ---- PointMatcher::DataPointsFilters stand-in (laser_track.cpp:24-30, :81, :146)
template <class PM>
class LsgpuDataPointsFilters {
 public:
  using DataPoints = typename PM::DataPoints;
  using Traits = LsgpuCloudTraits<PM>;
  LsgpuDataPointsFilters() = default;
  explicit LsgpuDataPointsFilters(std::istream& in, int device = 0) : device_(device) {
    try {
      laser_slam_amd::DataPointsFilters parsed(in, device);
      filters_ = parsed.modules();
    } catch (const laser_slam_amd::ConfigError& e) {
      throw std::runtime_error(std::string("LsgpuDataPointsFilters: ") + e.what());
    }
  }
  ~LsgpuDataPointsFilters() { if (h_) lsgpu_icp_destroy(h_); }
  LsgpuDataPointsFilters(const LsgpuDataPointsFilters&) = delete;
  LsgpuDataPointsFilters& operator=(const LsgpuDataPointsFilters&) = delete;
  LsgpuDataPointsFilters(LsgpuDataPointsFilters&& o) noexcept { *this = std::move(o); }
  LsgpuDataPointsFilters& operator=(LsgpuDataPointsFilters&& o) noexcept {
    if (this != &o) { if (h_) lsgpu_icp_destroy(h_); filters_ = std::move(o.filters_); h_ = o.h_; o.h_ = nullptr; device_ = o.device_; seed_ = o.seed_; }
    return *this;
  }
  void setSeed(int64_t seed) { seed_ = seed; }
  size_t size() const { return filters_.size(); }

  // In place.  The device filters only look at x, y, z and carry the 4th component through untouched, so the column
  // index travels in it: what comes back tells which columns survived, and the descriptors are thinned accordingly.
  void apply(DataPoints& cloud) {
    if (filters_.empty()) return;
    const int64_t n = Traits::size(cloud);
    if (n == 0) throw typename PM::ConvergenceError("no points to filter");   // as DataPointsFilters::apply does upstream
    // VoxelGridDataPointsFilter writes new points (below); of the descriptors it can only hand on the first point's
    bool writes_points = false;
    for (const auto& f : filters_) {
      // (OctreeGridDataPointsFilter: Centroid writes a new point as well; its other methods return the tagged point itself,
      //  for which the copy below changes nothing)
      writes_points = writes_points || f.type == LSGPU_FILTER_VOXEL_GRID || f.type == LSGPU_FILTER_OCTREE_GRID;
      if (f.type == LSGPU_FILTER_OCTREE_GRID && f.dim == 2 && Traits::hasDescriptors(cloud))
        throw std::runtime_error("LsgpuDataPointsFilters: OctreeGridDataPointsFilter: samplingMethod 2 (Centroid) on a cloud with "
                                 "descriptors is not implemented (averaging descriptors; samplingMethod 0, 1 and 3 keep the chosen point's)");
      if (f.type == LSGPU_FILTER_VOXEL_GRID && f.dim != 0 && Traits::hasDescriptors(cloud))
        throw std::runtime_error("LsgpuDataPointsFilters: VoxelGridDataPointsFilter: averageExistingDescriptors 1 on a cloud with "
                                 "descriptors is not implemented (set averageExistingDescriptors: 0 to keep the first point's)");
    }
    if (!h_) {
      lsgpu_icp_config c;
      lsgpu_icp_config_default(&c);
      if (lsgpu_icp_create(&c, device_, &h_) != LSGPU_OK) throw std::runtime_error("LsgpuDataPointsFilters: no ROCm GPU visible");
    }
    std::vector<float> tagged((size_t)n * 4), out((size_t)n * 4);
    std::memcpy(tagged.data(), Traits::features(cloud), (size_t)n * 16);
    for (int64_t i = 0; i < n; ++i) { const uint32_t tag = (uint32_t)i; std::memcpy(&tagged[4 * (size_t)i + 3], &tag, 4); }
    int64_t m = 0;
    const int rc = lsgpu_apply_point_filters(h_, filters_.data(), (int)filters_.size(), tagged.data(), n, seed_, out.data(), &m);
    if (rc == LSGPU_NO_CONVERGENCE) throw typename PM::ConvergenceError("no points to filter");
    if (rc != LSGPU_OK) throw std::runtime_error(std::string("LsgpuDataPointsFilters::apply: ") + lsgpu_strerror(rc));
    std::vector<int64_t> cols((size_t)m);
    for (int64_t j = 0; j < m; ++j) { uint32_t tag; std::memcpy(&tag, &out[4 * (size_t)j + 3], 4); cols[(size_t)j] = (int64_t)tag; }
    Traits::keepColumns(cloud, cols);
    if (writes_points) {   // the surviving column is the voxel's first point (pad row and descriptors); x, y, z are the voxel's point
      float* feat = const_cast<float*>(Traits::features(cloud));
      for (int64_t j = 0; j < m; ++j) std::memcpy(feat + 4 * (size_t)j, &out[4 * (size_t)j], 3 * sizeof(float));
    }
  }

 private:
  template <class> friend class LsgpuICP;   // LsgpuICP::ingestCloud runs this chain on the ICP's handle
  std::vector<lsgpu_point_filter> filters_;
  lsgpu_icp* h_ = nullptr;
  int device_ = 0;
  int64_t seed_ = -1;
};
