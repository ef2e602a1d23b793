// lsgpu_octree_filter.h -- OctreeGridDataPointsFilter of the input filter chain (libpointmatcher's module, 3-D case): the
// arithmetic shared by the device kernels (lsgpu_octree_filter.hip.h) and the host twin lsgpu_filter_octree_grid_points
// (DESIGN.md §3 "OctreeGridDataPointsFilter"; the restatement choices are §5 (49)-(54), the contract is in
// include/lsgpu_icp.h).
//
// All float, one IEEE operation per rounding (+ - * / sqrtf; the library is compiled with -ffp-contract=off and without
// fast-math), so that the recursion on the host and the per-point walk on the device agree bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include "lsgpu_host_math.h"
#include "../../include/lsgpu_icp.h"

namespace lsgpu {
namespace octreef {

constexpr int kMaxDepth = 21;   // 3 x 21 = 63 key bits (the one DEVIATION: upstream halves until the radius underflows)
enum { kFirstPts = 0, kRandomPts = 1, kCentroid = 2, kMedoid = 3 };

// the root box of ONE cloud and the depth below which no node is split
struct Root {
  float c[3];
  float radius;
  int depth;   // D = min(kMaxDepth, first depth whose nodes have 2 radius <= maxSizeByNode)
};

struct Pt { float x, y, z, w; };

// the module's parameters as lsgpu_point_filter carries them: nullptr, or what is wrong with them
inline const char* why_bad_params(float max_size, float max_point, int method, int build_parallel) {
  if (!(max_size >= 0.f) || !std::isfinite(max_size)) return "OctreeGridDataPointsFilter: maxSizeByNode must be finite and >= 0";
  if (!(max_point >= 1.f && max_point <= 16777216.f) || max_point != std::floor(max_point))
    return "OctreeGridDataPointsFilter: maxPointByNode must be an integer in [1, 2^24]";
  if (method < kFirstPts || method > kMedoid)
    return "OctreeGridDataPointsFilter: samplingMethod must be 0 (FirstPts), 1 (RandomPts), 2 (Centroid) or 3 (Medoid)";
  if (build_parallel != 0 && build_parallel != 1) return "OctreeGridDataPointsFilter: buildParallel must be 0 or 1";
  return nullptr;
}

// 2 radius <= maxSizeByNode: the node is not split whatever it holds
LSGPU_HD bool small_enough(float radius, float max_size) { return 2.0f * radius <= max_size; }

// the root from the cloud's finite minimum / maximum
inline void make_root(const float lo[3], const float hi[3], float max_size, Root* g) {
  float ext_max = 0.f;
  for (int a = 0; a < 3; ++a) {
    const float ext = hi[a] - lo[a];
    g->c[a] = lo[a] + ext * 0.5f;
    ext_max = ext > ext_max ? ext : ext_max;
  }
  g->radius = ext_max * 0.5f;
  float r = g->radius;
  int d = 0;
  while (d < kMaxDepth && !small_enough(r, max_size)) { r = r * 0.5f; ++d; }
  g->depth = d;
}

LSGPU_HD uint32_t octant(float x, float y, float z, const float c[3]) {
  return (x > c[0] ? 1u : 0u) | (y > c[1] ? 2u : 0u) | (z > c[2] ? 4u : 0u);
}

// child `o` of the node (c, radius): radius' = radius 0.5f, centre'_a = centre_a +- radius'
LSGPU_HD void descend(float c[3], float* radius, uint32_t o) {
  const float r = *radius * 0.5f;
  for (int a = 0; a < 3; ++a) c[a] = (o >> a) & 1u ? c[a] + r : c[a] - r;
  *radius = r;
}

// the octants of a point on its way from the root down to depth D, first level in the most significant used bits
LSGPU_HD uint64_t path_key(const Root& g, float x, float y, float z) {
  float c[3] = {g.c[0], g.c[1], g.c[2]};
  float r = g.radius;
  uint64_t key = 0;
  for (int l = 0; l < g.depth; ++l) {
    const uint32_t o = octant(x, y, z, c);
    key = (key << 3) | (uint64_t)o;
    descend(c, &r, o);
  }
  return key;
}

LSGPU_HD float dist(const Pt& v, const Pt& c) {
  const float dx = v.x - c.x, dy = v.y - c.y, dz = v.z - c.z;
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

// The output point of a leaf.  at(j): the leaf's j-th point in ascending input index, j in [0, count); one caller, one
// sequential float sum per leaf, however many points it holds.  draw: read for kRandomPts only.
template <class At>
LSGPU_HD Pt leaf_point(At at, uint32_t count, int method, float draw) {
  const Pt p0 = at(0u);
  if (method == kFirstPts) return p0;
  if (method == kRandomPts) return at((uint32_t)((float)(count - 1u) * draw));
  float sx = p0.x, sy = p0.y, sz = p0.z;
  for (uint32_t j = 1; j < count; ++j) {
    const Pt v = at(j);
    sx += v.x; sy += v.y; sz += v.z;
  }
  const float n = (float)count;
  const Pt cen = {sx / n, sy / n, sz / n, p0.w};
  if (method == kCentroid) return cen;
  uint32_t best = 0;
  float best_d = dist(p0, cen);
  for (uint32_t j = 1; j < count; ++j) {
    const float d = dist(at(j), cen);
    if (d < best_d) { best_d = d; best = j; }   // strict: the earliest point wins a tie
  }
  return at(best);
}

}  // namespace octreef
}  // namespace lsgpu
