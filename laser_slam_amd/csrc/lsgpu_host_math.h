// lsgpu_host_math.h -- the O(1) arithmetic of one ICP iteration, shared by host and device code
// (k_icp_update runs it on the GPU so that the loop needs no per-iteration host round trip; the host
// uses it for the final composition).
//
// libpointmatcher pieces restated here (selected by laser_slam/configurations/icp_default.yaml):
//   PointToPlaneErrorMinimizer solve + AngleAxis update ............ yaml:18-19
//   PointToPlaneErrorMinimizer force2D / force4DOF: the sub-system solve and the planar update (a ground vehicle's chain;
//     not in icp_default.yaml)
//   CounterTransformationChecker / DifferentialTransformationChecker  yaml:21-27
//   BoundTransformationChecker: its ConvergenceError is what laser_slam/src/laser_track.cpp:496-499 catches around
//     icp_.compute to fall back to the odometry (evaluated on the host after the loop, bound_first_violation)
//   final composition T_refIn_refMean * T_iter * T_refMean_dataIn
// All float, column-major 4x4 (PointMatcher<float>::TransformationParameters,
// laser_slam/include/laser_slam/common.hpp:14).  Compiled with -ffp-contract=off; only IEEE
// + - * / sqrt are used, except sin/cos/atan2 which are evaluated in double and rounded to float
// (within 1 ulp of libm's float versions, identical in all but ~1e-9 of the cases).
#pragma once
#include <cmath>
#include <cstring>

#if defined(__HIPCC__)
#define LSGPU_HD __host__ __device__ inline
#else
#define LSGPU_HD inline
#endif

namespace lsgpu {
namespace hostmath {

LSGPU_HD float at(const float* m, int r, int c) { return m[c * 4 + r]; }
LSGPU_HD void set(float* m, int r, int c, float v) { m[c * 4 + r] = v; }

LSGPU_HD void identity4(float* m) {
  for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f;
}

// out = a * b (out may alias an input)
LSGPU_HD void mul4(const float* a, const float* b, float* out) {
  float t[16];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      float s = at(a, r, 0) * at(b, 0, c);
      s = s + at(a, r, 1) * at(b, 1, c);
      s = s + at(a, r, 2) * at(b, 2, c);
      s = s + at(a, r, 3) * at(b, 3, c);
      t[c * 4 + r] = s;
    }
  for (int i = 0; i < 16; ++i) out[i] = t[i];
}

// device accumulator layout: 21 upper-tri (row major, a<=c), 6 rhs, count, sum r^2
LSGPU_HD void unpack_normal_eq(const double* ne, double A[36], double b[6]) {
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c, ++k) A[a * 6 + c] = A[c * 6 + a] = ne[k];
  for (int a = 0; a < 6; ++a) b[a] = ne[21 + a];
}

// x = A.llt().solve(b) in float (the minimiser works in PointMatcher<float>).
LSGPU_HD bool llt_solve6(const double A[36], const double b[6], float x[6]) {
  float L[6][6];
  float y[6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) L[i][j] = 0.f;
  for (int j = 0; j < 6; ++j) {
    float s = (float)A[j * 6 + j];
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.f)) return false;
    L[j][j] = sqrtf(s);
    for (int i = j + 1; i < 6; ++i) {
      float t = (float)A[i * 6 + j];
      for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    float t = (float)b[i];
    for (int k = 0; k < i; ++k) t = t - L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    float t = y[i];
    for (int k = i + 1; k < 6; ++k) t = t - L[k][i] * x[k];
    x[i] = t / L[i][i];
  }
  for (int i = 0; i < 6; ++i)
    if (x[i] != x[i]) return false;
  return true;
}

// ---- PointToPointErrorMinimizer.  Device accumulator layout (the same 29 slots as the normal equations):
// [0..2] sum p, [3..5] sum q, [6..14] sum q p^T (row major), [15..26] 0, [27] count, [28] sum |p - q|^2.
// M = sum (q - q_)(p - p_)^T;  R = argmax over SO(3) of tr(R^T M) -- what U V^T with the reflection fix
// (U diag(1,1,-1) V^T if det < 0) computes -- by Horn's quaternion: the eigenvector of the largest eigenvalue of
// a symmetric 4x4 built from M.  Cyclic Jacobi with an exact stopping rule: a rotation whose off-diagonal element is
// below 1e-18 of its two diagonal elements is skipped, the sweeps end with the first one that rotates nothing (at most
// kP2pSweeps; quadratic convergence: 4-5 reach double precision).  Same IEEE operations on both sides, so host and
// device give the same bits.  A rank-deficient M (collinear or coincident matches) still yields a unit quaternion,
// i.e. a proper rotation.  (The update lane runs this on ONE lane, a dependent chain of double divisions and square
// roots: every sweep saved is time off each iteration.)
constexpr int kP2pSweeps = 12;

LSGPU_HD void jacobi_eig4(double a[16], double v[16]) {
  for (int i = 0; i < 16; ++i) v[i] = (i % 5 == 0) ? 1.0 : 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int sweep = 0; sweep < kP2pSweeps; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p * 4 + q];
        if (!(fabs(apq) > 1e-18 * (fabs(a[p * 4 + p]) + fabs(a[q * 4 + q])))) continue;
        rotated = true;
        const double theta = (a[q * 4 + q] - a[p * 4 + p]) / (2.0 * apq);
        const double at = fabs(theta);
        double t = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {   // A <- A J (columns p, q)
          const double akp = a[k * 4 + p], akq = a[k * 4 + q];
          a[k * 4 + p] = c * akp - s * akq;
          a[k * 4 + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {   // A <- J^T A (rows p, q)
          const double apk = a[p * 4 + k], aqk = a[q * 4 + k];
          a[p * 4 + k] = c * apk - s * aqk;
          a[q * 4 + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {   // V <- V J
          const double vkp = v[k * 4 + p], vkq = v[k * 4 + q];
          v[k * 4 + p] = c * vkp - s * vkq;
          v[k * 4 + q] = s * vkp + c * vkq;
        }
      }
    if (!rotated) break;
  }
}

// dT (column major float) from the 29 sums; Mc = the centred M (row major), pq = {p_, q_}, x = {rotation vector, t}.
// false: no pair (count 0, "no point to minimize") or a non-finite result.
LSGPU_HD bool point_to_point_delta(const double* ne, float dT[16], double Mc[9], double pq[6], double x[6]) {
  const double W = ne[27];
  if (!(W > 0.0)) return false;
  for (int d = 0; d < 3; ++d) { pq[d] = ne[d] / W; pq[3 + d] = ne[3 + d] / W; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Mc[r * 3 + c] = ne[6 + r * 3 + c] - ne[3 + r] * pq[c];
  // Horn: S_ab = sum p'_a q'_b = M[b][a]
  const double Sxx = Mc[0], Syx = Mc[1], Szx = Mc[2], Sxy = Mc[3], Syy = Mc[4], Szy = Mc[5], Sxz = Mc[6], Syz = Mc[7], Szz = Mc[8];
  double N[16] = {Sxx + Syy + Szz, Syz - Szy,        Szx - Sxz,        Sxy - Syx,
                  Syz - Szy,       Sxx - Syy - Szz,  Sxy + Syx,        Szx + Sxz,
                  Szx - Sxz,       Sxy + Syx,        Syy - Sxx - Szz,  Syz + Szy,
                  Sxy - Syx,       Szx + Sxz,        Syz + Szy,        Szz - Sxx - Syy};
  double V[16];
  jacobi_eig4(N, V);
  // the column of the largest eigenvalue (the first of equal ones); selected without indexing by a variable
  double lam = N[0], w = V[0], qx = V[4], qy = V[8], qz = V[12];
  for (int i = 1; i < 4; ++i) {
    const bool better = N[i * 4 + i] > lam;
    lam = better ? N[i * 4 + i] : lam;
    w = better ? V[i] : w; qx = better ? V[4 + i] : qx; qy = better ? V[8 + i] : qy; qz = better ? V[12 + i] : qz;
  }
  const double nn = sqrt(w * w + qx * qx + qy * qy + qz * qz);
  if (!(nn > 0.0)) return false;
  if (w < 0.0) { w = -w; qx = -qx; qy = -qy; qz = -qz; }
  w = w / nn; qx = qx / nn; qy = qy / nn; qz = qz / nn;
  const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - w * qz),         2.0 * (qx * qz + w * qy),
                       2.0 * (qx * qy + w * qz),         1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - w * qx),
                       2.0 * (qx * qz - w * qy),         2.0 * (qy * qz + w * qx),         1.0 - 2.0 * (qx * qx + qy * qy)};
  identity4(dT);
  bool finite = true;
  for (int r = 0; r < 3; ++r) {
    const double t = pq[3 + r] - ((R[r * 3] * pq[0] + R[r * 3 + 1] * pq[1]) + R[r * 3 + 2] * pq[2]);
    x[3 + r] = t;
    set(dT, r, 3, (float)t);
    for (int c = 0; c < 3; ++c) set(dT, r, c, (float)R[r * 3 + c]);
    finite = finite && t - t == 0.0;
  }
  const double s = sqrt(qx * qx + qy * qy + qz * qz);
  const double ang = s > 0.0 ? 2.0 * atan2(s, w) / s : 0.0;
  x[0] = qx * ang; x[1] = qy * ang; x[2] = qz * ang;
  return finite;
}

LSGPU_HD float sin_f32(float a) { return (float)sin((double)a); }
LSGPU_HD float cos_f32(float a) { return (float)cos((double)a); }
LSGPU_HD float atan2_f32(float y, float x) { return (float)atan2((double)y, (double)x); }

// dT = [AngleAxis(|w|, w/|w|), t] with x = [w; t]; a zero rotation vector gives identity.
LSGPU_HD void delta_from_x(const float x[6], float* dT) {
  identity4(dT);
  const float ang = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (ang > 0.f && ang <= 3.4e38f) {
    const float ax = x[0] / ang, ay = x[1] / ang, az = x[2] / ang;
#if defined(__HIP_DEVICE_COMPILE__)
    double sd, cd;   // one range reduction for both (the device library's sin / cos are this same routine)
    sincos((double)ang, &sd, &cd);
    const float s = (float)sd, c = (float)cd;
#else
    const float s = sin_f32(ang), c = cos_f32(ang);
#endif
    const float sx = s * ax, sy = s * ay, sz = s * az;
    const float kx = (1.f - c) * ax, ky = (1.f - c) * ay, kz = (1.f - c) * az;
    float t = kx * ay; set(dT, 0, 1, t - sz); set(dT, 1, 0, t + sz);
    t = kx * az;       set(dT, 0, 2, t + sy); set(dT, 2, 0, t - sy);
    t = ky * az;       set(dT, 1, 2, t - sx); set(dT, 2, 1, t + sx);
    set(dT, 0, 0, kx * ax + c);
    set(dT, 1, 1, ky * ay + c);
    set(dT, 2, 2, kz * az + c);
  }
  set(dT, 0, 3, x[3]); set(dT, 1, 3, x[4]); set(dT, 2, 3, x[5]);
}

// ---- PointToPlaneErrorMinimizer force4DOF / force2D: the step with roll and pitch (and, force2D, z) held fixed.
// The unknowns are rows and columns 2 .. 2 + N - 1 of the 6x6 system: N = 4 {yaw, tx, ty, tz}, N = 3 {yaw, tx, ty}.
// The float LLT of llt_solve6 on that sub-system; x = {0, 0, yaw, tx, ty, tz}, the fixed unknowns exactly 0.
template <int N>
LSGPU_HD bool llt_solve_yaw(const double A[36], const double b[6], float x[6]) {
  static_assert(N == 3 || N == 4, "force2D: 3 unknowns, force4DOF: 4");
  constexpr int F = 2;
  float L[N][N];
  float y[N], z[N];
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) L[i][j] = 0.f;
  for (int j = 0; j < N; ++j) {
    float s = (float)A[(F + j) * 6 + F + j];
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.f)) return false;
    L[j][j] = sqrtf(s);
    for (int i = j + 1; i < N; ++i) {
      float t = (float)A[(F + i) * 6 + F + j];
      for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  for (int i = 0; i < N; ++i) {
    float t = (float)b[F + i];
    for (int k = 0; k < i; ++k) t = t - L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = N - 1; i >= 0; --i) {
    float t = y[i];
    for (int k = i + 1; k < N; ++k) t = t - L[k][i] * z[k];
    z[i] = t / L[i][i];
  }
  for (int i = 0; i < N; ++i)
    if (z[i] != z[i]) return false;
  for (int i = 0; i < 6; ++i) x[i] = 0.f;
  for (int i = 0; i < N; ++i) x[F + i] = z[i];
  return true;
}

// dT = [rotation by x[2] about z, t = x[3..5]]: the sine and cosine of |yaw| as delta_from_x takes them (its axis is
// (0, 0, +-1), so s * az is +-s exactly), the third row and column of the rotation written as 0, 0, 1 -- Rodrigues'
// (1 - c) + c is not 1 in float for every c.  A yaw of 0 (or a non-finite one) gives the identity rotation.
LSGPU_HD void delta_from_yaw(const float x[6], float* dT) {
  identity4(dT);
  const float ang = fabsf(x[2]);
  if (ang > 0.f && ang <= 3.4e38f) {
#if defined(__HIP_DEVICE_COMPILE__)
    double sd, cd;
    sincos((double)ang, &sd, &cd);
    const float s = (float)sd, c = (float)cd;
#else
    const float s = sin_f32(ang), c = cos_f32(ang);
#endif
    const float sz = x[2] < 0.f ? -s : s;
    set(dT, 0, 0, c); set(dT, 0, 1, -sz);
    set(dT, 1, 0, sz); set(dT, 1, 1, c);
  }
  set(dT, 0, 3, x[3]); set(dT, 1, 3, x[4]); set(dT, 2, 3, x[5]);
}

// the constrained step from the unpacked sums: N as above.  false: a failed pivot or a NaN (dT untouched)
template <int N>
LSGPU_HD bool point_to_plane_step_yaw(const double A[36], const double b[6], float x[6], float dT[16]) {
  if (!llt_solve_yaw<N>(A, b, x)) return false;
  delta_from_yaw(x, dT);
  return true;
}

// Eigen Quaternion(Matrix3): q = {w, x, y, z}
LSGPU_HD void quat_from_rotation(const float* T, float q[4]) {
  float t = at(T, 0, 0) + at(T, 1, 1) + at(T, 2, 2);
  if (t > 0.f) {
    t = sqrtf(t + 1.0f);
    q[0] = 0.5f * t;
    t = 0.5f / t;
    q[1] = (at(T, 2, 1) - at(T, 1, 2)) * t;
    q[2] = (at(T, 0, 2) - at(T, 2, 0)) * t;
    q[3] = (at(T, 1, 0) - at(T, 0, 1)) * t;
  } else {
    int i = 0;
    if (at(T, 1, 1) > at(T, 0, 0)) i = 1;
    if (at(T, 2, 2) > at(T, i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrtf(at(T, i, i) - at(T, j, j) - at(T, k, k) + 1.0f);
    q[1 + i] = 0.5f * t;
    t = 0.5f / t;
    q[0] = (at(T, k, j) - at(T, j, k)) * t;
    q[1 + j] = (at(T, j, i) + at(T, i, j)) * t;
    q[1 + k] = (at(T, k, i) + at(T, i, k)) * t;
  }
}

// angle of a * conj(b): 2 atan2(|vec|, |w|)   (Eigen >= 3.3 angularDistance)
LSGPU_HD float angular_distance(const float a[4], const float b[4]) {
  const float bw = b[0], bx = -b[1], by = -b[2], bz = -b[3];
  const float w = a[0] * bw - a[1] * bx - a[2] * by - a[3] * bz;
  const float x = a[0] * bx + a[1] * bw + a[2] * bz - a[3] * by;
  const float y = a[0] * by + a[2] * bw + a[3] * bx - a[1] * bz;
  const float z = a[0] * bz + a[3] * bw + a[1] * by - a[2] * bx;
  return 2.0f * atan2_f32(sqrtf(x * x + y * y + z * z), fabsf(w));
}

// Counter (first) then Differential, in the order icp_default.yaml:21-27 lists them.  The history
// lives in caller-provided arrays of (max_iter + 2) entries: hist[i] = {qw,qx,qy,qz, tx,ty,tz, |rotation to entry i-1|}.
struct CheckerState {
  int counter;
  int n_hist;
};

LSGPU_HD void checker_push(CheckerState* s, float* hist, const float* T) {
  float* e = hist + 8 * s->n_hist;
  quat_from_rotation(T, e);
  e[4] = at(T, 0, 3); e[5] = at(T, 1, 3); e[6] = at(T, 2, 3);
  // slot 7: the rotation between this entry and its predecessor -- the differential checker looks at every pair
  // `smooth` times over consecutive iterations; computed once, here (an atan2 evaluated in double each)
  e[7] = s->n_hist > 0 ? fabsf(angular_distance(e, e - 8)) : 0.f;
  s->n_hist++;
}

// false => NaN (ConvergenceError).  *iterate is cleared when a checker says stop.
// (out2: the two smoothed changes the differential checker compared with its limits, 0 while its history is short --
// the device's loop state carries them to the host, which sizes its next group of launches from them)
LSGPU_HD bool checker_check(CheckerState* s, float* hist, int max_iter, int smooth, float lim_rot,
                            float lim_trans, const float* T, bool* iterate, bool* by_diff, float* out2 = nullptr) {
  if (out2) { out2[0] = 0.f; out2[1] = 0.f; }
  if (++s->counter >= max_iter) { *iterate = false; return true; }  // MaxNumIterationsReached
  checker_push(s, hist, T);
  float rot = 0.f, trans = 0.f;
  const int n = s->n_hist;
  if (n > smooth) {
    for (int i = n - 1; i >= n - smooth; --i) {
      const float* a = hist + 8 * i;
      const float* b = hist + 8 * (i - 1);
      rot += a[7];   // = fabsf(angular_distance(a, b)), see checker_push
      const float dx = a[4] - b[4], dy = a[5] - b[5], dz = a[6] - b[6];
      trans += fabsf(sqrtf(dx * dx + dy * dy + dz * dz));
    }
    rot /= (float)smooth;
    trans /= (float)smooth;
    if (out2) { out2[0] = rot; out2[1] = trans; }
    if (rot < lim_rot && trans < lim_trans) { *iterate = false; *by_diff = true; }
  }
  return !(rot != rot || trans != trans);
}

// BoundTransformationChecker over a checker history (entries as checker_push writes them, entry 0 the state the checkers
// were initialised with): the first index >= 1 whose rotation or translation differs from entry 0 by MORE than its limit,
// -1 if there is none.  rot / trans (nullable): the two values of that entry.  Host side only: the loop's kernels do not
// evaluate the bound, the library does after the loop.
inline int bound_first_violation(const float* hist, int n, float max_rot, float max_trans, float* rot, float* trans) {
  for (int i = 1; i < n; ++i) {
    const float* e = hist + 8 * i;
    const float r = angular_distance(e, hist);
    const float dx = e[4] - hist[4], dy = e[5] - hist[5], dz = e[6] - hist[6];
    const float t = sqrtf(dx * dx + dy * dy + dz * dz);
    if (r > max_rot || t > max_trans) {
      if (rot) *rot = r;
      if (trans) *trans = t;
      return i;
    }
  }
  return -1;
}

}  // namespace hostmath
}  // namespace lsgpu
