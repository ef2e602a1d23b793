// lsgpu_host_filters.cpp -- host-side modules of the chain (the reference runs them on the CPU
// inside PointMatcher::ICP::compute, laser_slam/src/laser_track.cpp:496):
//   RandomSamplingDataPointsFilter           laser_slam/configurations/icp_default.yaml:1-3
//   SamplingSurfaceNormalDataPointsFilter    laser_slam/configurations/icp_default.yaml:5-7
//   SurfaceNormalDataPointsFilter            (a user's chain; the contract is in include/lsgpu_icp.h)
//   VoxelGridDataPointsFilter                (the input filter chain; the contract is in include/lsgpu_icp.h)
//   RigidTransformation check / correct      laser_slam/include/laser_slam/common.hpp:136-149
// GPU versions of the two filters are SURVEY.md §8f row N1/N3 ("next").
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <unordered_map>
#include <utility>
#include <vector>

#include "lsgpu_host_math.h"

#include "../../include/lsgpu_icp.h"
#include "lsgpu_box_normal.h"
#include "lsgpu_density.h"
#include "lsgpu_robust.h"
#include "lsgpu_shadow.h"
#include "lsgpu_cov_sampling.h"
#include "lsgpu_normal_angle.h"
#include "lsgpu_rand.h"
#include "lsgpu_voxel_filter.h"
#include "lsgpu_octree_filter.h"
#include "lsgpu_cov.h"

namespace {

struct SurfaceNormalBuilder {
  const float* xyz1;
  std::vector<int32_t> idx;
  std::vector<std::pair<float, int32_t>> scratch;
  int knn;
  float ratio;
  float* out_xyz1;
  float* out_nrm;
  int64_t n_out = 0;
  std::vector<unsigned char> keep;   // per ORIGINAL index: kept (the draws are taken in box-traversal order)
  std::vector<float> nrm_of;         // per original index: its box's normal

  // upstream sorts indicesToKeep ascending before it compacts the cloud in place: the output is in original index order
  void emit(int64_t n) {
    for (int64_t i = 0; i < n; ++i)
      if (keep[(size_t)i]) {
        const int64_t o = n_out++;
        std::memcpy(out_xyz1 + 4 * o, xyz1 + 4 * i, 16);
        std::memcpy(out_nrm + 3 * o, nrm_of.data() + 3 * i, 12);
      }
  }

  float coord(int32_t i, int d) const { return xyz1[4 * (int64_t)i + d]; }

  void fuse(int64_t first, int64_t last) {
    const int64_t cnt = last - first;
    if (cnt <= 0) return;
    float n[3];
    if (!lsgpu::boxnormal::box_normal((int)cnt, [&](int i, int d) { return coord(idx[first + i], d); }, n))
      return;  // degenerate box: dropped
    float draws[64];
    for (int64_t i = first; i < last; ++i) {  // samplingMethod 0: random subset keeps the box normal
      const int64_t k = (i - first) % 64;
      if (k == 0) lsgpu::DrawStream::global().take(-1, (size_t)std::min<int64_t>(64, last - i), draws);
      const float r = draws[k];
      if (r < ratio) {   // indicesToKeep.push_back(k); normals->col(k) = normal: compacted by original index in emit()
        const int64_t k_orig = idx[i];
        keep[(size_t)k_orig] = 1;
        for (int d = 0; d < 3; ++d) nrm_of[3 * (size_t)k_orig + d] = n[d];
      }
    }
  }

  void build(int64_t first, int64_t last, const float* minb, const float* maxb) {
    const int64_t count = last - first;
    if (count <= knn) { fuse(first, last); return; }
    int cut = 0;
    for (int d = 1; d < 3; ++d)
      if (maxb[d] - minb[d] > maxb[cut] - minb[cut]) cut = d;
    const int64_t right = count / 2, left = count - right;
    // std::nth_element leaves ties and the order inside each half unspecified; a stable sort fixes both,
    // so that this filter and the device filter (lsgpu_ssn.hip.h, stable radix sort) build the same boxes
    // in the same order and draw the same rand() numbers for the same points.
    // (sorted as (coordinate, index) pairs: the comparisons then touch contiguous memory only)
    scratch.resize((size_t)count);
    for (int64_t i = 0; i < count; ++i) scratch[(size_t)i] = {coord(idx[first + i], cut), idx[first + i]};
    std::stable_sort(scratch.begin(), scratch.end(),
                     [](const std::pair<float, int32_t>& a, const std::pair<float, int32_t>& b) { return a.first < b.first; });
    for (int64_t i = 0; i < count; ++i) idx[first + i] = scratch[(size_t)i].second;
    const float cutval = coord(idx[first + left], cut);
    float lmax[3] = {maxb[0], maxb[1], maxb[2]}, rmin[3] = {minb[0], minb[1], minb[2]};
    lmax[cut] = cutval; rmin[cut] = cutval;
    build(first, first + left, minb, lmax);
    build(first + left, last, rmin, maxb);
  }
};

// MaxDensityDataPointsFilter's parameter and its place behind SurfaceNormalDataPointsFilter (sn_knn: that module's knn, 0: absent)
const char* max_density_why(const lsgpu_max_density_config* c, int sn_knn) {
  if (!c) return "MaxDensityDataPointsFilter: no configuration";
  if (!(c->max_density > 0.f)) return "MaxDensityDataPointsFilter: maxDensity must be > 0 (inf allowed)";
  if (c->reserved[0] || c->reserved[1] || c->reserved[2]) return "MaxDensityDataPointsFilter: reserved fields must be 0";
  if (sn_knn <= 0) return "MaxDensityDataPointsFilter: needs the densities of SurfaceNormalDataPointsFilter with keepDensities 1 as the reference filter (sn_knn > 0)";
  return nullptr;
}

float det3(const float* T) {
  auto m = [&](int r, int c) { return T[c * 4 + r]; };
  return m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) -
         m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) +
         m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0));
}

}  // namespace

extern "C" {

int64_t lsgpu_filter_random_sampling(int64_t n, float prob, int64_t seed, int64_t* keep_idx) {
  if (seed >= 0) lsgpu::DrawStream::global().take(seed, 0, nullptr);
  if (n <= 0 || !keep_idx) return 0;
  int64_t m = 0;
  float draws[1024];
  for (int64_t i0 = 0; i0 < n; i0 += 1024) {
    const int64_t k = std::min<int64_t>(1024, n - i0);
    lsgpu::DrawStream::global().take(-1, (size_t)k, draws);
    for (int64_t i = 0; i < k; ++i)
      if (draws[i] < prob) keep_idx[m++] = i0 + i;
  }
  return m;
}

int64_t lsgpu_filter_sampling_surface_normal(const float* xyz1, int64_t n, int knn, float ratio,
                                             int64_t seed, float* out_xyz1, float* out_normals) {
  if (n <= 0 || !xyz1 || !out_xyz1 || !out_normals || knn < 3) return 0;
  if (seed >= 0) lsgpu::DrawStream::global().take(seed, 0, nullptr);
  SurfaceNormalBuilder b;
  b.xyz1 = xyz1; b.knn = knn; b.ratio = ratio; b.out_xyz1 = out_xyz1; b.out_nrm = out_normals;
  b.idx.resize((size_t)n);
  std::iota(b.idx.begin(), b.idx.end(), 0);
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int64_t i = 0; i < n; ++i)
    for (int d = 0; d < 3; ++d) {
      mn[d] = std::min(mn[d], xyz1[4 * i + d]);
      mx[d] = std::max(mx[d], xyz1[4 * i + d]);
    }
  b.keep.assign((size_t)n, 0);
  b.nrm_of.resize(3 * (size_t)n);
  b.build(0, n, mn, mx);
  b.emit(n);
  return b.n_out;
}

// VoxelGridDataPointsFilter: upstream's sequential loop -- every point in input order goes to its voxel, whose sums start
// as its first point and grow by one float addition per further point.  Upstream keeps a vector of numVox voxels; a map
// from the voxel index to the voxel's slot gives the same result without the memory, and the slots, made in input
// order, are already in the order of the first points.
int64_t lsgpu_filter_voxel_grid_points(const float* xyz1, int64_t n, const float vsize[3], int use_centroid,
                                       float* out_xyz1) {
  if (!vsize) return -LSGPU_BAD_ARG;
  if (lsgpu::voxelf::why_bad_params(vsize, use_centroid, 0)) return -LSGPU_BAD_CONFIG;
  if (n <= 0) return -LSGPU_NO_CONVERGENCE;
  if (!xyz1 || !out_xyz1 || n > 0x7FFFFFF0ll) return -LSGPU_BAD_ARG;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = hi[a] = xyz1[a];
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const float c = xyz1[4 * i + a];
      if (!std::isfinite(c)) return -LSGPU_BAD_ARG;
      lo[a] = std::min(lo[a], c); hi[a] = std::max(hi[a], c);
    }
  lsgpu::voxelf::Geom g;
  if (lsgpu::voxelf::make_geom(lo, hi, vsize, &g) != LSGPU_OK) return -LSGPU_BAD_CONFIG;
  struct Voxel { uint32_t key, count; float s[3], w; };
  std::vector<Voxel> voxels;
  std::unordered_map<uint32_t, uint32_t> slot_of;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz1 + 4 * i;
    const uint32_t key = lsgpu::voxelf::voxel_index(g, p[0], p[1], p[2]);
    const auto it = slot_of.find(key);
    if (it == slot_of.end()) {
      slot_of.emplace(key, (uint32_t)voxels.size());
      voxels.push_back(Voxel{key, 1u, {p[0], p[1], p[2]}, p[3]});
    } else {
      Voxel& v = voxels[it->second];
      for (int a = 0; a < 3; ++a) v.s[a] += p[a];
      ++v.count;
    }
  }
  for (size_t o = 0; o < voxels.size(); ++o) {
    const Voxel& v = voxels[o];
    float* q = out_xyz1 + 4 * o;
    if (use_centroid) {
      const float c = (float)v.count;
      for (int a = 0; a < 3; ++a) q[a] = v.s[a] / c;
    } else {
      const uint32_t nxy = g.ndiv[0] * g.ndiv[1];
      const uint32_t ck = v.key / nxy, rem = v.key - ck * nxy, cj = rem / g.ndiv[0], ci = rem - cj * g.ndiv[0];
      q[0] = lsgpu::voxelf::centre(g, 0, ci); q[1] = lsgpu::voxelf::centre(g, 1, cj); q[2] = lsgpu::voxelf::centre(g, 2, ck);
    }
    std::memcpy(q + 3, &v.w, 4);
  }
  return (int64_t)voxels.size();
}

}  // extern "C"

namespace {

// OctreeGridDataPointsFilter: the recursion.  A node is its points' input indices in ascending order; a leaf emits its point
// when it is reached, so the output is in depth-first leaf order and RandomPts draws once per non-empty leaf in that order.
struct OctreeSampler {
  const float* xyz1;
  float max_size;
  size_t max_point;
  int method;
  float* out;
  int64_t n_out = 0;

  void leaf(const std::vector<uint32_t>& idx) {
    float draw = 0.f;
    if (method == lsgpu::octreef::kRandomPts) lsgpu::DrawStream::global().take(-1, 1, &draw);
    const lsgpu::octreef::Pt r = lsgpu::octreef::leaf_point(
        [&](uint32_t j) { lsgpu::octreef::Pt v; std::memcpy(&v, xyz1 + 4 * (size_t)idx[j], 16); return v; }, (uint32_t)idx.size(), method, draw);
    std::memcpy(out + 4 * n_out++, &r, 16);
  }
  void node(const std::vector<uint32_t>& idx, const float c[3], float radius, int depth) {
    if (lsgpu::octreef::small_enough(radius, max_size) || idx.size() <= max_point || depth == lsgpu::octreef::kMaxDepth) { leaf(idx); return; }
    std::vector<uint32_t> child[8];
    for (const uint32_t i : idx) {
      const float* p = xyz1 + 4 * (size_t)i;
      child[lsgpu::octreef::octant(p[0], p[1], p[2], c)].push_back(i);
    }
    for (uint32_t o = 0; o < 8; ++o) {
      if (child[o].empty()) continue;
      float cc[3] = {c[0], c[1], c[2]}, r = radius;
      lsgpu::octreef::descend(cc, &r, o);
      node(child[o], cc, r, depth + 1);
    }
  }
};

}  // namespace

extern "C" {

int64_t lsgpu_filter_octree_grid_points(const float* xyz1, int64_t n, float max_size_by_node, int max_point_by_node,
                                        int sampling_method, int64_t seed, float* out_xyz1) {
  if (max_point_by_node > (1 << 24) ||   // (the float the descriptor carries would round the next integers to 2^24)
      lsgpu::octreef::why_bad_params(max_size_by_node, (float)max_point_by_node, sampling_method, 1)) return -LSGPU_BAD_CONFIG;
  if (seed >= 0) lsgpu::DrawStream::global().take(seed, 0, nullptr);
  if (n <= 0) return -LSGPU_NO_CONVERGENCE;
  if (!xyz1 || !out_xyz1 || n > 0x7FFFFFF0ll) return -LSGPU_BAD_ARG;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = hi[a] = xyz1[a];
  for (int64_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      const float c = xyz1[4 * i + a];
      if (!std::isfinite(c)) return -LSGPU_BAD_ARG;
      lo[a] = std::min(lo[a], c); hi[a] = std::max(hi[a], c);
    }
  lsgpu::octreef::Root g;
  lsgpu::octreef::make_root(lo, hi, max_size_by_node, &g);
  OctreeSampler s{xyz1, max_size_by_node, (size_t)max_point_by_node, sampling_method, out_xyz1};
  std::vector<uint32_t> all((size_t)n);
  std::iota(all.begin(), all.end(), 0u);
  s.node(all, g.c, g.radius, 0);
  return s.n_out;
}

// SurfaceNormalDataPointsFilter.  A checker: the exact search sweeps outwards from the point along the x-sorted cloud
// and stops where dx * dx alone exceeds the knn-th distance found so far (d2 = fma(dz,dz, fma(dy,dy, dx*dx)) >= dx * dx
// in float as well: adding a non-negative term never rounds below the other operand).
int lsgpu_filter_surface_normal(const float* xyz1, int64_t n, int knn, float* out_normals, int32_t* out_ids,
                                float* out_d2) {
  return lsgpu_filter_surface_normal_densities(xyz1, n, knn, out_normals, out_ids, out_d2, nullptr);
}

int lsgpu_filter_surface_normal_densities(const float* xyz1, int64_t n, int knn, float* out_normals, int32_t* out_ids,
                                          float* out_d2, float* out_densities) {
  if (!xyz1 || !out_normals || knn < 3 || knn > 32 || n < knn || n > 0x7FFFFFF0ll / knn || (out_d2 && !out_ids))
    return LSGPU_BAD_ARG;
  // centred as lsgpu_icp_set_reference centres the reference: float mean from double sums, one float subtraction
  double sum[3] = {0.0, 0.0, 0.0};
  for (int64_t i = 0; i < n; ++i)
    for (int d = 0; d < 3; ++d) sum[d] += (double)xyz1[4 * i + d];
  float mean[3];
  for (int d = 0; d < 3; ++d) mean[d] = (float)(sum[d] / (double)n);
  std::vector<float> c(3 * (size_t)n);
  for (int64_t i = 0; i < n; ++i)
    for (int d = 0; d < 3; ++d) c[3 * (size_t)i + d] = xyz1[4 * i + d] - mean[d];
  std::vector<int32_t> order((size_t)n), pos((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return c[3 * (size_t)a] < c[3 * (size_t)b]; });
  std::vector<float> sx((size_t)n);
  for (int64_t r = 0; r < n; ++r) { pos[(size_t)order[(size_t)r]] = (int32_t)r; sx[(size_t)r] = c[3 * (size_t)order[(size_t)r]]; }
  float D[32]; int32_t I[32];
  for (int64_t i = 0; i < n; ++i) {
    const float qx = c[3 * (size_t)i], qy = c[3 * (size_t)i + 1], qz = c[3 * (size_t)i + 2];
    int have = 0;
    auto offer = [&](int64_t r) {
      const int32_t t = order[(size_t)r];
      const float dx = qx - c[3 * (size_t)t], dy = qy - c[3 * (size_t)t + 1], dz = qz - c[3 * (size_t)t + 2];
      const float d = std::fmaf(dz, dz, std::fmaf(dy, dy, dx * dx));
      if (have == knn && !(d < D[knn - 1] || (d == D[knn - 1] && t < I[knn - 1]))) return;
      int s = have < knn ? have++ : knn - 1;
      for (; s > 0 && (d < D[s - 1] || (d == D[s - 1] && t < I[s - 1])); --s) { D[s] = D[s - 1]; I[s] = I[s - 1]; }
      D[s] = d; I[s] = t;
    };
    int64_t lo = pos[(size_t)i], hi = pos[(size_t)i] + 1;   // [lo, hi) has been offered once `lo` is
    offer(lo);
    bool left = lo > 0, right = hi < n;
    while (left || right) {
      if (left) {
        const float dx = qx - sx[(size_t)(lo - 1)];
        if (have == knn && dx * dx > D[knn - 1]) left = false;
        else { offer(--lo); left = lo > 0; }
      }
      if (right) {
        const float dx = qx - sx[(size_t)hi];
        if (have == knn && dx * dx > D[knn - 1]) right = false;
        else { offer(hi++); right = hi < n; }
      }
    }
    if (out_ids)
      for (int s = 0; s < knn; ++s) {
        out_ids[(size_t)i * (size_t)knn + s] = I[s];
        if (out_d2) out_d2[(size_t)i * (size_t)knn + s] = D[s];
      }
    float nv[3];
    if (!lsgpu::boxnormal::box_normal(knn, [&](int k, int d) { return c[3 * (size_t)I[k] + d]; }, nv)) {
      nv[0] = 0.f; nv[1] = 1.f; nv[2] = 0.f;   // upstream leaves the eigenvectors at identity: column 1
    }
    std::memcpy(out_normals + 3 * i, nv, 12);
    if (out_densities) out_densities[i] = lsgpu::density::of_neighbourhood(knn, [&](int k, int d) { return c[3 * (size_t)I[k] + d]; });
  }
  return LSGPU_OK;
}

// ---- MaxDensityDataPointsFilter behind SurfaceNormalDataPointsFilter keepDensities 1: upstream's sequential loop (csrc/lsgpu_density.h)
void lsgpu_max_density_config_default(lsgpu_max_density_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->max_density = 10.f;
}
int lsgpu_max_density_config_check(const lsgpu_max_density_config* c, int sn_knn) { return max_density_why(c, sn_knn) ? LSGPU_BAD_CONFIG : LSGPU_OK; }
const char* lsgpu_max_density_config_why(const lsgpu_max_density_config* c, int sn_knn) { return max_density_why(c, sn_knn); }

int lsgpu_filter_max_density(const float* xyz1, int64_t n, int knn, float max_density, int64_t seed, float* out_xyz1,
                             float* out_normals, float* out_densities, int64_t* n_out, int64_t* n_dense) {
  if (!out_xyz1 || !out_normals || !n_out || !n_dense) return LSGPU_BAD_ARG;
  *n_out = 0; *n_dense = 0;
  lsgpu_max_density_config mc;
  lsgpu_max_density_config_default(&mc);
  mc.max_density = max_density;
  if (max_density_why(&mc, knn)) return LSGPU_BAD_CONFIG;
  std::vector<float> nrm(3 * (size_t)std::max<int64_t>(n, 0)), dens((size_t)std::max<int64_t>(n, 0));
  const int rc = lsgpu_filter_surface_normal_densities(xyz1, n, knn, nrm.data(), nullptr, nullptr, dens.data());
  if (rc) return rc;
  if (seed >= 0) lsgpu::DrawStream::global().take(seed, 0, nullptr);
  // last: the largest non-NaN density; sat: 0 iff every point's density equals it
  float last = 0.f;
  bool any = false, all_equal = true;
  for (int64_t i = 0; i < n; ++i)
    if (dens[(size_t)i] == dens[(size_t)i] && (!any || dens[(size_t)i] > last)) { last = dens[(size_t)i]; any = true; }
  for (int64_t i = 0; i < n; ++i) all_equal = all_equal && dens[(size_t)i] == last;
  const int sat = all_equal ? 0 : 1;
  int64_t kept = 0, dense = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float d = dens[(size_t)i];
    bool keep = true;
    if (lsgpu::density::is_dense(d, max_density)) {
      float draw;
      lsgpu::DrawStream::global().take(-1, 1, &draw);
      ++dense;
      keep = lsgpu::density::keeps(d, max_density, last, sat, draw);
    }
    if (keep) {
      std::memcpy(out_xyz1 + 4 * kept, xyz1 + 4 * i, 16);
      std::memcpy(out_normals + 3 * kept, nrm.data() + 3 * i, 12);
      ++kept;
    }
  }
  if (out_densities) std::memcpy(out_densities, dens.data(), (size_t)n * sizeof(float));
  *n_out = kept; *n_dense = dense;
  return kept > 0 ? LSGPU_OK : LSGPU_NO_CONVERGENCE;
}

// ---- ShadowDataPointsFilter: the predicate of csrc/lsgpu_shadow.h over the cloud in its order
void lsgpu_shadow_config_default(lsgpu_shadow_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->reading_eps = -1.f; c->reference_eps = -1.f;
}
const char* lsgpu_shadow_config_why(const lsgpu_shadow_config* c) {
  if (!c) return "ShadowDataPointsFilter: no configuration";
  // (eps < 0: no module on that side; a NaN is neither)
  if (!(c->reading_eps < 0.f) && !lsgpu::shadow::eps_ok(c->reading_eps)) return "ShadowDataPointsFilter: the reading's eps must be in [0, 3.1416] (or < 0: no module)";
  if (!(c->reference_eps < 0.f) && !lsgpu::shadow::eps_ok(c->reference_eps)) return "ShadowDataPointsFilter: the reference's eps must be in [0, 3.1416] (or < 0: no module)";
  if (c->reserved[0] || c->reserved[1]) return "ShadowDataPointsFilter: reserved fields must be 0";
  return nullptr;
}
int lsgpu_shadow_config_check(const lsgpu_shadow_config* c) { return lsgpu_shadow_config_why(c) ? LSGPU_BAD_CONFIG : LSGPU_OK; }

int lsgpu_filter_shadow(const float* xyz1, const float* normals, int64_t n, float eps, float* out_xyz1, float* out_normals,
                        int64_t* n_out) {
  if (!n_out) return LSGPU_BAD_ARG;
  *n_out = 0;
  if (n < 0 || (n > 0 && (!xyz1 || !normals || !out_xyz1 || !out_normals)) || out_xyz1 == xyz1 || out_normals == normals) return LSGPU_BAD_ARG;
  if (!lsgpu::shadow::eps_ok(eps)) return LSGPU_BAD_CONFIG;
  int64_t kept = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz1 + 4 * i;
    const float* v = normals + 3 * i;
    if (!lsgpu::shadow::keeps(p[0], p[1], p[2], v[0], v[1], v[2], eps)) continue;
    std::memcpy(out_xyz1 + 4 * kept, p, 16);
    std::memcpy(out_normals + 3 * kept, v, 12);
    ++kept;
  }
  *n_out = kept;
  return kept > 0 ? LSGPU_OK : LSGPU_NO_CONVERGENCE;
}

// ---- CovarianceSamplingDataPointsFilter: the steps of include/lsgpu_icp.h in their order, the arithmetic of
// csrc/lsgpu_cov_sampling.h; with sums_in the sums are the caller's (the device's), everything behind them is computed here
void lsgpu_cov_sampling_config_default(lsgpu_cov_sampling_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->reading_torque_norm = 1; c->reference_torque_norm = 1;
}
const char* lsgpu_cov_sampling_config_why(const lsgpu_cov_sampling_config* c) {
  if (!c) return "CovarianceSamplingDataPointsFilter: no configuration";
  // (nbSample 0: no module on that side)
  if (c->reading_nb_sample != 0 && !lsgpu::covs::nb_sample_ok(c->reading_nb_sample)) return "CovarianceSamplingDataPointsFilter: the reading's nbSample must be in [1, 2147483632] (or 0: no module)";
  if (c->reference_nb_sample != 0 && !lsgpu::covs::nb_sample_ok(c->reference_nb_sample)) return "CovarianceSamplingDataPointsFilter: the reference's nbSample must be in [1, 2147483632] (or 0: no module)";
  if (!lsgpu::covs::torque_norm_ok(c->reading_torque_norm)) return "CovarianceSamplingDataPointsFilter: the reading's torqueNorm must be 0, 1 or 2";
  if (!lsgpu::covs::torque_norm_ok(c->reference_torque_norm)) return "CovarianceSamplingDataPointsFilter: the reference's torqueNorm must be 0, 1 or 2";
  for (int r : c->reserved)
    if (r) return "CovarianceSamplingDataPointsFilter: reserved fields must be 0";
  return nullptr;
}
int lsgpu_cov_sampling_config_check(const lsgpu_cov_sampling_config* c) { return lsgpu_cov_sampling_config_why(c) ? LSGPU_BAD_CONFIG : LSGPU_OK; }

int lsgpu_cov_sampling_eigen(const double C21[21], float X[36], double values[6]) {
  if (!C21 || !X) return LSGPU_BAD_ARG;
  for (int k = 0; k < 21; ++k)
    if (!std::isfinite(C21[k])) return LSGPU_BAD_ARG;
  lsgpu::covs::eigen(C21, X, values);
  return LSGPU_OK;
}

int lsgpu_filter_cov_sampling(const float* xyz1, const float* normals, int64_t n, int nb_sample, int torque_norm, const double* sums_in,
                              float* out_xyz1, float* out_normals, int32_t* out_ids, int64_t* n_out, double sums_out[32]) {
  namespace cs = lsgpu::covs;
  if (!n_out) return LSGPU_BAD_ARG;
  *n_out = 0;
  if (n < 0 || n > cs::kPointsMax || (n > 0 && (!xyz1 || !normals || !out_xyz1 || !out_normals)) || (n > 0 && (out_xyz1 == xyz1 || out_normals == normals)))
    return LSGPU_BAD_ARG;
  if (!cs::nb_sample_ok(nb_sample) || !cs::torque_norm_ok(torque_norm)) return LSGPU_BAD_CONFIG;
  if (n == 0) return LSGPU_NO_CONVERGENCE;
  if ((int64_t)nb_sample >= n) {   // the cloud passes unchanged, nothing is computed
    std::memcpy(out_xyz1, xyz1, (size_t)n * 16);
    std::memcpy(out_normals, normals, (size_t)n * 12);
    if (out_ids) std::iota(out_ids, out_ids + n, 0);
    if (sums_out) { std::fill(sums_out, sums_out + cs::kSums, 0.0); sums_out[cs::kSumN] = (double)n; }
    *n_out = n;
    return LSGPU_OK;
  }
  double sums[cs::kSums];
  std::fill(sums, sums + cs::kSums, 0.0);
  if (sums_in) std::memcpy(sums, sums_in, sizeof sums);
  sums[cs::kSumN] = (double)n;
  if (!sums_in) {
    for (int a = 0; a < 3; ++a) { sums[cs::kSumMin + a] = (double)INFINITY; sums[cs::kSumMax + a] = -(double)INFINITY; }
    for (int64_t i = 0; i < n; ++i)
      for (int a = 0; a < 3; ++a) {
        const double v = (double)xyz1[4 * i + a];
        sums[cs::kSumS + a] += v;
        if (v < sums[cs::kSumMin + a]) sums[cs::kSumMin + a] = v;
        if (v > sums[cs::kSumMax + a]) sums[cs::kSumMax + a] = v;
      }
  }
  if (!cs::finite_sums(sums)) return LSGPU_BAD_ARG;
  float c[3];
  cs::centre(sums, n, c);
  if (!sums_in && torque_norm == 1)
    for (int64_t i = 0; i < n; ++i)
      sums[cs::kSumLen] += (double)cs::length(xyz1[4 * i] - c[0], xyz1[4 * i + 1] - c[1], xyz1[4 * i + 2] - c[2]);
  const float L = cs::lnorm(torque_norm, sums, n);
  if (!(L != 0.f) || !std::isfinite(L)) return LSGPU_BAD_ARG;
  const float invL = 1.f / L;
  std::vector<float> v6(6 * (size_t)n);
  for (int64_t i = 0; i < n; ++i)
    cs::vec6(xyz1[4 * i], xyz1[4 * i + 1], xyz1[4 * i + 2], normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], c, invL, &v6[6 * (size_t)i]);
  if (!sums_in)
    for (int64_t i = 0; i < n; ++i) {
      const float* v = &v6[6 * (size_t)i];
      for (int a = 0, k = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++k) sums[cs::kSumC + k] += (double)v[a] * (double)v[b];
    }
  if (!cs::finite_sums(sums)) return LSGPU_BAD_ARG;
  cs::Eig e;
  cs::eigen(sums + cs::kSumC, e.X, nullptr);
  std::vector<float> mag(6 * (size_t)n);
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 6; ++k) mag[6 * (size_t)i + k] = cs::magnitude(&v6[6 * (size_t)i], e.X, k);
  const int64_t m = nb_sample;   // (< n)
  std::vector<cs::Head> heads(6 * (size_t)m);
  std::vector<uint32_t> order((size_t)n);
  for (int k = 0; k < 6; ++k) {
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
      return cs::sort_key(mag[6 * (size_t)x + k]) < cs::sort_key(mag[6 * (size_t)y + k]);
    });
    for (int64_t j = 0; j < m; ++j) {
      cs::Head& hd = heads[(size_t)k * (size_t)m + (size_t)j];
      hd.id = order[(size_t)j];
      std::memcpy(hd.mag, &mag[6 * (size_t)hd.id], 24);
    }
  }
  std::vector<uint32_t> ids((size_t)m);
  std::vector<uint64_t> chosen;
  if (cs::walk(heads.data(), m, n, m, ids.data(), chosen) != m) return LSGPU_BAD_ARG;
  for (int64_t j = 0; j < m; ++j) {
    std::memcpy(out_xyz1 + 4 * j, xyz1 + 4 * (size_t)ids[(size_t)j], 16);
    std::memcpy(out_normals + 3 * j, normals + 3 * (size_t)ids[(size_t)j], 12);
    if (out_ids) out_ids[j] = (int32_t)ids[(size_t)j];
  }
  if (sums_out) std::memcpy(sums_out, sums, sizeof sums);
  *n_out = m;
  return LSGPU_OK;
}

int lsgpu_check_rigid(const float T[16]) { return std::fabs(1.0f - det3(T)) <= 0.001f; }

void lsgpu_correct_rigid(const float T[16], float out[16]) {
  float c[3][3];
  for (int k = 0; k < 3; ++k) {
    const float x = T[k * 4], y = T[k * 4 + 1], z = T[k * 4 + 2];
    const float n = std::sqrt(x * x + y * y + z * z);
    c[k][0] = x / n; c[k][1] = y / n; c[k][2] = z / n;
  }
  const float c0[3] = {c[1][1] * c[2][2] - c[1][2] * c[2][1], c[1][2] * c[2][0] - c[1][0] * c[2][2],
                       c[1][0] * c[2][1] - c[1][1] * c[2][0]};
  const float c1[3] = {c[2][1] * c0[2] - c[2][2] * c0[1], c[2][2] * c0[0] - c[2][0] * c0[2],
                       c[2][0] * c0[1] - c[2][1] * c0[0]};
  std::memcpy(out, T, 16 * sizeof(float));
  for (int r = 0; r < 3; ++r) { out[r] = c0[r]; out[4 + r] = c1[r]; out[8 + r] = c[2][r]; }
}

int lsgpu_point_to_point_solve(const double sums[29], float T_out[16]) {
  if (!sums || !T_out) return LSGPU_BAD_ARG;
  double Mc[9], pq[6], x[6];
  if (!lsgpu::hostmath::point_to_point_delta(sums, T_out, Mc, pq, x)) {
    lsgpu::hostmath::identity4(T_out);
    return LSGPU_NO_CONVERGENCE;
  }
  return LSGPU_OK;
}

int lsgpu_point_to_plane_solve(const double sums[27], float dT[16]) {
  if (!sums || !dT) return LSGPU_BAD_ARG;
  double A[36], b[6];
  float x[6];
  lsgpu::hostmath::unpack_normal_eq(sums, A, b);
  if (!lsgpu::hostmath::llt_solve6(A, b, x)) {
    lsgpu::hostmath::identity4(dT);
    return LSGPU_NO_CONVERGENCE;
  }
  lsgpu::hostmath::delta_from_x(x, dT);
  return LSGPU_OK;
}

// ---- PointToPlaneErrorMinimizer force4DOF / force2D and BoundTransformationChecker (lsgpu_icp_set_motion)
void lsgpu_motion_config_default(lsgpu_motion_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->max_rotation_norm = 1.f; c->max_translation_norm = 1.f;
}
const char* lsgpu_motion_config_why(const lsgpu_motion_config* c) {
  if (!c) return "PointToPlaneErrorMinimizer / BoundTransformationChecker: no configuration";
  if (c->dof != LSGPU_MOTION_DOF_6 && c->dof != LSGPU_MOTION_DOF_3 && c->dof != LSGPU_MOTION_DOF_4)
    return "PointToPlaneErrorMinimizer: dof must be 0 (free), 3 (force2D) or 4 (force4DOF)";
  if (c->bound != 0 && c->bound != 1) return "BoundTransformationChecker: bound must be 0 or 1";
  if (c->bound_before_counter != 0 && c->bound_before_counter != 1) return "BoundTransformationChecker: bound_before_counter must be 0 or 1";
  if (c->bound) {
    if (!(c->max_rotation_norm >= 0.f) || std::isinf(c->max_rotation_norm)) return "BoundTransformationChecker: maxRotationNorm must be finite and >= 0";
    if (!(c->max_translation_norm >= 0.f) || std::isinf(c->max_translation_norm)) return "BoundTransformationChecker: maxTranslationNorm must be finite and >= 0";
  }
  if (c->reserved[0] || c->reserved[1] || c->reserved[2]) return "PointToPlaneErrorMinimizer / BoundTransformationChecker: reserved fields must be 0";
  return nullptr;
}
int lsgpu_motion_config_check(const lsgpu_motion_config* c) { return lsgpu_motion_config_why(c) ? LSGPU_BAD_CONFIG : LSGPU_OK; }

int lsgpu_point_to_plane_solve_dof(const double sums[27], int dof, float dT[16]) {
  if (dof == LSGPU_MOTION_DOF_6) return lsgpu_point_to_plane_solve(sums, dT);
  if (!sums || !dT || (dof != LSGPU_MOTION_DOF_3 && dof != LSGPU_MOTION_DOF_4)) return LSGPU_BAD_ARG;
  double A[36], b[6];
  float x[6];
  lsgpu::hostmath::unpack_normal_eq(sums, A, b);
  lsgpu::hostmath::identity4(dT);
  const bool ok = dof == LSGPU_MOTION_DOF_3 ? lsgpu::hostmath::point_to_plane_step_yaw<3>(A, b, x, dT)
                                            : lsgpu::hostmath::point_to_plane_step_yaw<4>(A, b, x, dT);
  return ok ? LSGPU_OK : LSGPU_NO_CONVERGENCE;
}

int lsgpu_bound_first_violation(const float* T_iters, int n, float max_rot, float max_trans) {
  if (!T_iters || n < 2) return -1;
  std::vector<float> hist((size_t)8 * n);
  lsgpu::hostmath::CheckerState cs{0, 0};
  for (int i = 0; i < n; ++i) lsgpu::hostmath::checker_push(&cs, hist.data(), T_iters + 16 * i);
  return lsgpu::hostmath::bound_first_violation(hist.data(), n, max_rot, max_trans, nullptr, nullptr);
}

// ---- PointToPlaneWithCovErrorMinimizer: the 6x6 work on the sums of k_cov (csrc/lsgpu_cov.h)
void lsgpu_covariance_config_default(lsgpu_covariance_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->sensor_std_dev = 0.01f;
}

int lsgpu_point_to_plane_cov_solve(const double sums[44], float sensor_std_dev, double cov[36]) {
  if (!sums || !cov) return LSGPU_BAD_ARG;
  if (!(sensor_std_dev >= 0.f) || std::isinf(sensor_std_dev)) return LSGPU_BAD_CONFIG;
  if (!(sums[42] > 0.0)) return LSGPU_NO_CONVERGENCE;   // "no point to minimize" (a NaN count included)
  return lsgpu::cov::solve(sums, (double)sensor_std_dev, cov) ? LSGPU_OK : LSGPU_NO_CONVERGENCE;
}

// ---- RobustOutlierFilter: the host twins of the device loop's scale and weights (csrc/lsgpu_robust.h)
void lsgpu_robust_config_default(lsgpu_robust_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->robust_fct = LSGPU_ROBUST_CAUCHY; c->tuning = 1.f; c->scale_estimator = LSGPU_ROBUST_SCALE_MAD;
  c->nb_iteration_for_scale = 0; c->distance_type = LSGPU_ROBUST_DIST_POINT2POINT; c->approximation = INFINITY;
}

int lsgpu_robust_config_check(const lsgpu_robust_config* c, int error_minimizer, int have_normals) {
  return lsgpu::robust::check(c, error_minimizer, have_normals, nullptr);
}
const char* lsgpu_robust_config_why(const lsgpu_robust_config* c, int error_minimizer, int have_normals) {
  const char* why = nullptr;
  lsgpu::robust::check(c, error_minimizer, have_normals, &why);
  return why;
}

int lsgpu_robust_scale(const float* d2, int64_t n, float* median, float* scale) {
  if (!d2 || n < 0 || !median || !scale) return LSGPU_BAD_ARG;
  std::vector<float> v;
  v.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i)
    if (std::isfinite(d2[i])) v.push_back(d2[i]);
  if (v.empty()) return LSGPU_NO_CONVERGENCE;
  const size_t mid = v.size() / 2;
  std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)mid, v.end());
  const float med = v[mid];
  for (float& x : v) x = std::fabs(x - med);
  std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)mid, v.end());
  *median = med;
  *scale = sqrtf(v[mid]);
  return LSGPU_OK;
}

int lsgpu_robust_weights(const lsgpu_robust_config* cfg, float scale, const float* e, int64_t n, float* w_out) {
  if (!cfg || n < 0 || (n > 0 && (!e || !w_out))) return LSGPU_BAD_ARG;
  if (lsgpu::robust::check(cfg, LSGPU_MINIMIZER_POINT_TO_PLANE, 1, nullptr) != LSGPU_OK) return LSGPU_BAD_CONFIG;
  const lsgpu::robust::Params p = lsgpu::robust::params(*cfg);
  for (int64_t i = 0; i < n; ++i) w_out[i] = lsgpu::robust::weight(p.fct, e[i], scale, p.k, p.approx2);
  return LSGPU_OK;
}

// ---- SurfaceNormalOutlierFilter and the orientation step: the host twins of the device code (csrc/lsgpu_normal_angle.h)
void lsgpu_normals_config_default(lsgpu_normals_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->max_angle = -1.f;
}

int lsgpu_normals_config_check(const lsgpu_normals_config* c, int error_minimizer, int have_reference_normals) {
  return lsgpu::normal_angle::check(c, error_minimizer, have_reference_normals, nullptr);
}
const char* lsgpu_normals_config_why(const lsgpu_normals_config* c, int error_minimizer, int have_reference_normals) {
  const char* why = nullptr;
  lsgpu::normal_angle::check(c, error_minimizer, have_reference_normals, &why);
  return why;
}

int lsgpu_orient_normals(const float* xyz1, int64_t n, const float sensor[3], int mode, float* normals) {
  if (n < 0 || (mode != 1 && mode != 2) || !sensor || (n > 0 && (!xyz1 || !normals))) return LSGPU_BAD_ARG;
  for (int64_t i = 0; i < n; ++i) {
    float* v = normals + 3 * i;
    const float* p = xyz1 + 4 * i;
    if (lsgpu::normal_angle::flips(p[0], p[1], p[2], sensor[0], sensor[1], sensor[2], v[0], v[1], v[2], mode)) {
      v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2];
    }
  }
  return LSGPU_OK;
}

int lsgpu_normal_angle_weights(const float T[16], const float* reading_normals, int64_t nq, const float* reference_normals,
                               const int32_t* ids, int k, float max_angle, float* w) {
  if (!T || nq < 0 || k < 1 || (nq > 0 && (!reading_normals || !reference_normals || !ids || !w))) return LSGPU_BAD_ARG;
  if (!(max_angle >= 0.f && max_angle <= 3.1416f)) return LSGPU_BAD_CONFIG;
  const float eps = lsgpu::normal_angle::eps_of(max_angle);
  float rows[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) rows[r * 4 + c] = T[c * 4 + r];
  for (int64_t i = 0; i < nq; ++i) {
    const float* rn = reading_normals + 3 * i;
    for (int j = 0; j < k; ++j) {
      const int32_t id = ids[i * k + j];
      if (id < 0) { w[i * k + j] = 0.f; continue; }
      const float* f = reference_normals + 3 * (int64_t)id;
      w[i * k + j] = lsgpu::normal_angle::keep(rows, rn[0], rn[1], rn[2], f[0], f[1], f[2], eps) ? 1.f : 0.f;
    }
  }
  return LSGPU_OK;
}

float lsgpu_rotation_distance(const float Ta[16], const float Tb[16]) {
  float qa[4], qb[4];
  lsgpu::hostmath::quat_from_rotation(Ta, qa);
  lsgpu::hostmath::quat_from_rotation(Tb, qb);
  return lsgpu::hostmath::angular_distance(qa, qb);
}

}  // extern "C"
