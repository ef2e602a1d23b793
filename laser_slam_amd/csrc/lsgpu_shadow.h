// lsgpu_shadow.h -- the predicate of ShadowDataPointsFilter, shared by the host filter (lsgpu_host_filters.cpp) and the device
// pass (lsgpu_shadow.hip.h), and the check of the module's parameter.  Compiled with -ffp-contract=off; only IEEE * + / sqrt
// and fabs in a fixed order, so host and device agree bit for bit (choices 41-44).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LSGPU_SH_HD __host__ __device__ inline
#else
#define LSGPU_SH_HD inline
#endif

namespace lsgpu {
namespace shadow {

constexpr float kEpsMax = 3.1416f;   // upstream's upper bound of eps

// |cos| of the angle between the normal n and the ray from the sensor (the origin of the frame the point is given in) to the
// point p: both normalised with three divisions each, every sum of three terms left to right.  A zero normal, a point at the
// origin or a NaN anywhere gives 0 or NaN.
LSGPU_SH_HD float value(float px, float py, float pz, float nx, float ny, float nz) {
  const float ln = sqrtf((nx * nx + ny * ny) + nz * nz);
  const float lp = sqrtf((px * px + py * py) + pz * pz);
  const float ux = nx / ln, uy = ny / ln, uz = nz / ln;
  const float vx = px / lp, vy = py / lp, vz = pz / lp;
  return fabsf((ux * vx + uy * vy) + uz * vz);
}

// Is the point kept?  (A NaN value compares false: dropped.  0 / 0 of a zero normal or a point at the origin is NaN too.)
LSGPU_SH_HD bool keeps(float px, float py, float pz, float nx, float ny, float nz, float eps) {
  return value(px, py, pz, nx, ny, nz) > eps;
}

// eps of a side that has the module: finite, in [0, 3.1416]
LSGPU_SH_HD bool eps_ok(float eps) { return eps >= 0.f && eps <= kEpsMax; }

}  // namespace shadow
}  // namespace lsgpu
