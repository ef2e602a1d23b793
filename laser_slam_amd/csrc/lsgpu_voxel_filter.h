// lsgpu_voxel_filter.h -- VoxelGridDataPointsFilter of the input filter chain (libpointmatcher's module, NOT pcl::VoxelGrid
// of lsgpu_filter_voxel_grid): the arithmetic shared by the device kernels (lsgpu_voxel_filter.hip.h) and the host twin
// lsgpu_filter_voxel_grid_points (DESIGN.md §3 "VoxelGridDataPointsFilter"; the restatement choices are §5 (30)-(34), the
// contract is in include/lsgpu_icp.h).
//
// All float, one IEEE operation per rounding (+ - * / floorf; the library is compiled with -ffp-contract=off and without
// fast-math, so `/` is the correctly rounded division on the host and on the device), so that the two agree bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include "lsgpu_host_math.h"
#include "../../include/lsgpu_icp.h"

namespace lsgpu {
namespace voxelf {

// what the kernels are handed: the grid of ONE cloud (its anchor is the cloud's own minimum)
struct Geom {
  float vsize[3];
  float minb[3];     // min_a / vSize_a
  uint32_t ndiv[3];  // (uint)((1 + maxB) - minB), at least 1; ndiv[0] ndiv[1] ndiv[2] <= 2^31 - 1
};

// the module's parameters as lsgpu_point_filter carries them: nullptr, or what is wrong with them
inline const char* why_bad_params(const float v[3], int use_centroid, int average_descriptors) {
  for (int a = 0; a < 3; ++a)
    if (!(v[a] > 0.f) || !std::isfinite(v[a])) return "VoxelGridDataPointsFilter: vSizeX / vSizeY / vSizeZ must be finite and > 0";
  if (use_centroid != 0 && use_centroid != 1) return "VoxelGridDataPointsFilter: useCentroid must be 0 or 1";
  if (average_descriptors != 0 && average_descriptors != 1) return "VoxelGridDataPointsFilter: averageExistingDescriptors must be 0 or 1";
  return nullptr;
}

// The grid from the cloud's finite minimum / maximum (host side).  LSGPU_OK, or LSGPU_BAD_CONFIG "too many voxels".
inline int make_geom(const float lo[3], const float hi[3], const float v[3], Geom* g) {
  uint64_t nvox = 1;
  for (int a = 0; a < 3; ++a) {
    g->vsize[a] = v[a];
    g->minb[a] = lo[a] / v[a];
    const float maxb = hi[a] / v[a];
    const float t = (1.0f + maxb) - g->minb[a];
    if (!(t < 2147483648.f)) return LSGPU_BAD_CONFIG;
    const uint32_t nd = (uint32_t)t;
    g->ndiv[a] = nd ? nd : 1u;   // (1 + maxB rounds to maxB for |maxB| >= 2^24: a cloud of one cell still has that cell)
    nvox *= g->ndiv[a];          // < 2^31 * 2^31 before the check
    if (nvox > 2147483647ull) return LSGPU_BAD_CONFIG;
  }
  return LSGPU_OK;
}

// i = (uint)floorf(x / vSize - minB), clamped to numDiv - 1 (x >= min, so the floor is never negative)
LSGPU_HD uint32_t cell(float x, float vsize, float minb, uint32_t ndiv) {
  const float f = floorf(x / vsize - minb);
  const uint32_t i = f >= 2147483648.f ? 0x7FFFFFFFu : (uint32_t)f;
  return i < ndiv ? i : ndiv - 1u;
}

LSGPU_HD uint32_t voxel_index(const Geom& g, float x, float y, float z) {
  const uint32_t i = cell(x, g.vsize[0], g.minb[0], g.ndiv[0]);
  const uint32_t j = cell(y, g.vsize[1], g.minb[1], g.ndiv[1]);
  const uint32_t k = cell(z, g.vsize[2], g.minb[2], g.ndiv[2]);
  return i + j * g.ndiv[0] + k * g.ndiv[0] * g.ndiv[1];
}

// the centre of cell i on axis a: vSize (minB + (float)i + 0.5), in that order
LSGPU_HD float centre(const Geom& g, int a, uint32_t i) {
  return g.vsize[a] * ((g.minb[a] + (float)i) + 0.5f);
}

}  // namespace voxelf
}  // namespace lsgpu
