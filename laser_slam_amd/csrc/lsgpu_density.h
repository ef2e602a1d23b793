// lsgpu_density.h -- the density descriptor of SurfaceNormalDataPointsFilter (keepDensities 1) and the acceptance rule of
// MaxDensityDataPointsFilter, shared by the host filters (lsgpu_host_filters.cpp) and the device kernels (lsgpu_snf.hip.h,
// lsgpu_max_density.hip.h).  Compiled with -ffp-contract=off; only IEEE + - * / sqrt in a fixed order (no pow), so host
// and device agree bit for bit when they visit the neighbourhood in the same order (choices 36-40).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LSGPU_DN_HD __host__ __device__ inline
#else
#define LSGPU_DN_HD inline
#endif

namespace lsgpu {
namespace density {

constexpr float kFourThirdsPi = 4.18879020478639098f;   // (4 / 3) pi, rounded once to float

// Density of one neighbourhood.  point(i, d) -> coordinate d of its i-th point, in the order box_normal visits them:
// the mean is box_normal's (float sums in that order, / (float)cnt), r = the largest distance of a point from it,
// density = cnt / ((4/3) pi r r r).  r == 0 (cnt identical points) gives +inf.
template <class PointFn>
LSGPU_DN_HD float of_neighbourhood(int cnt, PointFn point) {
  float mean[3] = {0.f, 0.f, 0.f};
  for (int i = 0; i < cnt; ++i)
    for (int d = 0; d < 3; ++d) mean[d] += point(i, d);
  for (int d = 0; d < 3; ++d) mean[d] /= (float)cnt;
  float r2 = 0.f;
  for (int i = 0; i < cnt; ++i) {
    const float ex = point(i, 0) - mean[0], ey = point(i, 1) - mean[1], ez = point(i, 2) - mean[2];
    const float ee = (ex * ex + ey * ey) + ez * ez;
    r2 = ee > r2 ? ee : r2;
  }
  const float r = sqrtf(r2);
  const float volume = kFourThirdsPi * ((r * r) * r);
  return (float)cnt / volume;
}

// MaxDensityDataPointsFilter: does the point take a draw?  (A NaN density does not: it is kept.)
LSGPU_DN_HD bool is_dense(float dens, float max_density) { return dens > max_density; }

// ... and is it kept with this draw?  last = the largest non-NaN density of the cloud, sat = 0 iff every point's density
// equals it (upstream's integer division 1 - nbSaturated / n), else 1.
LSGPU_DN_HD bool keeps(float dens, float max_density, float last, int sat, float draw) {
  float accept = max_density / dens;
  if (dens == last) accept = accept * (float)sat;
  return draw < accept;
}

}  // namespace density
}  // namespace lsgpu
