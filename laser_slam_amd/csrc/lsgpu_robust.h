// lsgpu_robust.h -- RobustOutlierFilter (libpointmatcher's M-estimator weights with a MAD scale), the arithmetic shared by
// the weighted instantiation of k_normal_eq_loop and the host twins lsgpu_robust_scale / lsgpu_robust_weights
// ("RobustOutlierFilter"; the restatement choices are §5 (18)-(23)).
//
// All float, one IEEE operation per rounding (+ - * / sqrt; the library is compiled with -ffp-contract=off), so that the
// host and the device agree bit for bit.  welsch and student are not here: exp / pow differ between the two.
#pragma once
#include <cmath>
#include <cstdint>
#include "lsgpu_host_math.h"
#include "../../include/lsgpu_icp.h"

namespace lsgpu {
namespace robust {

// what the kernels are handed (from a checked lsgpu_robust_config)
struct Params {
  int fct;          // LSGPU_ROBUST_CAUCHY .. LSGPU_ROBUST_L1
  int plane;        // distanceType point2plane: e = r r instead of d2
  int mad;          // scaleEstimator mad (0: none, scale = 1)
  float k;          // tuning
  float approx2;    // approximation^2 (+inf: none)
};

// w(e) with e2 = e / scale^2, k = tuning
LSGPU_HD float weight(int fct, float e, float scale, float k, float approx2) {
  const float s2 = scale * scale;
  const float e2 = e / s2;
  const float k2 = k * k;
  float w;
  switch (fct) {
    case LSGPU_ROBUST_CAUCHY: { const float t = e2 / k2; w = 1.f / (1.f + t); break; }
    case LSGPU_ROBUST_HUBER: { w = e2 < k2 ? 1.f : k / sqrtf(e2); break; }
    case LSGPU_ROBUST_TUKEY: { const float t = 1.f - e2 / k2; w = e2 < k2 ? t * t : 0.f; break; }
    case LSGPU_ROBUST_GM: { const float d = k + e2; w = k2 / (d * d); break; }
    case LSGPU_ROBUST_SC: { const float d = k + e2; const float n = 4.f * k2; w = e2 > k ? n / (d * d) : 1.f; break; }
    default: { w = 1.f / sqrtf(e2); break; }   // LSGPU_ROBUST_L1
  }
  if (approx2 < INFINITY && e2 >= approx2) w = 0.f;
  return w;
}

// is the scale recomputed in iteration `it` (1-based, restarted by every align)?
LSGPU_HD bool recomputes(int nb_iteration_for_scale, int it) {
  return nb_iteration_for_scale == 0 || it <= nb_iteration_for_scale;
}

// LSGPU_OK or LSGPU_BAD_CONFIG; `why` (nullable) receives the reason, the module's name in it
inline int check(const lsgpu_robust_config* c, int error_minimizer, int have_normals, const char** why) {
  const char* w = nullptr;
  if (!c) w = "RobustOutlierFilter: no configuration";
  else if (c->robust_fct == LSGPU_ROBUST_WELSCH || c->robust_fct == LSGPU_ROBUST_STUDENT)
    w = "RobustOutlierFilter: robustFct welsch / student are not implemented (exp / pow are not bit-identical between host and device)";
  else if (c->robust_fct < LSGPU_ROBUST_CAUCHY || c->robust_fct > LSGPU_ROBUST_STUDENT) w = "RobustOutlierFilter: unknown robustFct";
  else if (c->scale_estimator == LSGPU_ROBUST_SCALE_BERG || c->scale_estimator == LSGPU_ROBUST_SCALE_STD)
    w = "RobustOutlierFilter: scaleEstimator berg / std are not implemented (none and mad are)";
  else if (c->scale_estimator != LSGPU_ROBUST_SCALE_NONE && c->scale_estimator != LSGPU_ROBUST_SCALE_MAD) w = "RobustOutlierFilter: unknown scaleEstimator";
  else if (!(c->tuning >= 0.f)) w = "RobustOutlierFilter: tuning must be >= 0";
  else if (!(c->approximation >= 0.f)) w = "RobustOutlierFilter: approximation must be >= 0 (inf: none)";
  else if (c->nb_iteration_for_scale < 0) w = "RobustOutlierFilter: nbIterationForScale must be >= 0";
  else if (c->distance_type != LSGPU_ROBUST_DIST_POINT2POINT && c->distance_type != LSGPU_ROBUST_DIST_POINT2PLANE) w = "RobustOutlierFilter: unknown distanceType";
  else if (c->distance_type == LSGPU_ROBUST_DIST_POINT2PLANE && error_minimizer == LSGPU_MINIMIZER_POINT_TO_POINT && !have_normals)
    w = "RobustOutlierFilter: distanceType point2plane needs reference normals";
  else if (c->reserved[0] != 0 || c->reserved[1] != 0) w = "RobustOutlierFilter: reserved fields must be 0";
  if (why) *why = w;
  return w ? LSGPU_BAD_CONFIG : LSGPU_OK;
}

inline Params params(const lsgpu_robust_config& c) {
  Params p;
  p.fct = c.robust_fct;
  p.plane = c.distance_type == LSGPU_ROBUST_DIST_POINT2PLANE ? 1 : 0;
  p.mad = c.scale_estimator == LSGPU_ROBUST_SCALE_MAD ? 1 : 0;
  p.k = c.tuning;
  p.approx2 = std::isinf(c.approximation) ? INFINITY : c.approximation * c.approximation;
  return p;
}

}  // namespace robust
}  // namespace lsgpu
