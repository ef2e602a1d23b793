// lsgpu_normal_angle.h -- SurfaceNormalOutlierFilter (the angle test between a reading normal and its match's normal) and
// the orientation step of ObservationDirectionDataPointsFilter + OrientNormalsDataPointsFilter: the arithmetic shared by
// the chain instantiations of k_normal_eq_loop, k_orient_normals and the host twins lsgpu_normal_angle_weights /
// lsgpu_orient_normals ("SurfaceNormalOutlierFilter"; the restatement choices are §5 (24)-(29)).
//
// All float, one IEEE operation per rounding with explicit fmaf (the library is compiled with -ffp-contract=off), so that
// the host and the device agree bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include "lsgpu_host_math.h"
#include "../../include/lsgpu_icp.h"

namespace lsgpu {
namespace normal_angle {

// eps of the filter: the cosine is taken once, on the host, in double
inline float eps_of(float max_angle) { return (float)std::cos((double)max_angle); }

// a / |a|, |a| = sqrtf(fma(z,z,fma(y,y,x x))); a vector of length 0 stays as it is
LSGPU_HD void normalize(float& x, float& y, float& z) {
  const float n = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
  if (n != 0.f) { x = x / n; y = y / n; z = z / n; }
}

// Is the pair kept?  rows: the iteration's transform as Mat34 rows (m[r * 4 + c]), of which the rotation is applied to the
// reading normal r with the fma chain of lsgpu_rotate_descriptors; f the matched reference normal.  v < eps rejects; a
// NaN v keeps the pair (as the upstream comparison).
LSGPU_HD bool keep(const float* rows, float rx, float ry, float rz, float fx, float fy, float fz, float eps) {
  float ax = fmaf(rows[2], rz, fmaf(rows[1], ry, rows[0] * rx));
  float ay = fmaf(rows[6], rz, fmaf(rows[5], ry, rows[4] * rx));
  float az = fmaf(rows[10], rz, fmaf(rows[9], ry, rows[8] * rx));
  normalize(ax, ay, az);
  normalize(fx, fy, fz);
  const float v = fmaf(az, fz, fmaf(ay, fy, ax * fx));
  return !(v < eps);
}

// OrientNormalsDataPointsFilter on one point: is the normal n of the point p flipped?  s = (sensor - p) . n;
// mode 1 (towardCenter): s < 0 flips; mode 2 (away): s > 0 flips.
LSGPU_HD bool flips(float px, float py, float pz, float sx, float sy, float sz, float nx, float ny, float nz, int mode) {
  const float ox = sx - px, oy = sy - py, oz = sz - pz;
  const float s = fmaf(oz, nz, fmaf(oy, ny, ox * nx));
  return mode == 1 ? s < 0.f : mode == 2 ? s > 0.f : false;
}

// LSGPU_OK or LSGPU_BAD_CONFIG; `why` (nullable) receives the reason, the module's name in it
inline int check(const lsgpu_normals_config* c, int error_minimizer, int have_reference_normals, const char** why) {
  (void)error_minimizer;
  const char* w = nullptr;
  if (!c) w = "SurfaceNormalOutlierFilter: no configuration";
  else if (std::isnan(c->max_angle) || c->max_angle > 3.1416f) w = "SurfaceNormalOutlierFilter: maxAngle must be in [0, 3.1416]";
  else if (c->reading_sn_knn != 0 && (c->reading_sn_knn < 3 || c->reading_sn_knn > 32))
    w = "SurfaceNormalDataPointsFilter (reading): knn must be in [3, 32]";
  else if (c->reading_orient < 0 || c->reading_orient > 2 || c->reference_orient < 0 || c->reference_orient > 2)
    w = "OrientNormalsDataPointsFilter: orientation must be 0 (off), 1 (towardCenter) or 2 (away)";
  else if (c->reading_orient != 0 && c->reading_sn_knn == 0)
    w = "OrientNormalsDataPointsFilter (reading): needs the normals of a SurfaceNormalDataPointsFilter in front of it";
  else if (c->reference_orient != 0 && !have_reference_normals)
    w = "OrientNormalsDataPointsFilter (reference): needs the normals of a reference filter in front of it";
  else if (c->max_angle >= 0.f && c->reading_sn_knn == 0 && c->reading_normals_given == 0)
    w = "SurfaceNormalOutlierFilter: the reading section provides no normals (SurfaceNormalDataPointsFilter)";
  else if (c->max_angle >= 0.f && !have_reference_normals)
    w = "SurfaceNormalOutlierFilter: the reference section provides no normals";
  else if (c->reading_sn_knn != 0 && !(c->max_angle >= 0.f))
    w = "SurfaceNormalDataPointsFilter (reading): only SurfaceNormalOutlierFilter reads reading normals, and the chain holds none";
  else if (c->reading_normals_given < 0 || c->reading_normals_given > 1 || c->reserved[0] != 0) w = "SurfaceNormalOutlierFilter: reserved fields must be 0";
  else {
    for (int i = 0; i < 3 && !w; ++i)
      if (!std::isfinite(c->reading_sensor[i]) || !std::isfinite(c->reference_sensor[i]))
        w = "ObservationDirectionDataPointsFilter: x, y, z must be finite";
  }
  if (why) *why = w;
  return w ? LSGPU_BAD_CONFIG : LSGPU_OK;
}

}  // namespace normal_angle
}  // namespace lsgpu
