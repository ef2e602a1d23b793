// lsgpu_cov_sampling.h -- the arithmetic of CovarianceSamplingDataPointsFilter shared by the device path
// (lsgpu_cov_sampling.hip.h, lsgpu_icp_filter_cov_sampling) and the host twin (lsgpu_host_filters.cpp): the per-point 6-vector,
// the projections and their sort key for host and device, and -- host only -- Lnorm, the Jacobi of step 5 and the walk of
// step 8.  include/lsgpu_icp.h, "CovarianceSamplingDataPointsFilter", states the module; DESIGN.md §5 choices 55-62.  Compiled
// with -ffp-contract=off; only IEEE * + - / sqrt and fabs in a fixed order, so host and device agree bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define LSGPU_CS_HD __host__ __device__ inline
#else
#define LSGPU_CS_HD inline
#endif

namespace lsgpu {
namespace covs {

constexpr int kNbSampleMax = 0x7FFFFFF0;   // 2^31 - 16
constexpr long long kPointsMax = 0x7FFFFFF0ll / 6;   // points of a cloud (the kernels hold a point's index in an int, as the Shadow pass does)
// sums_out[32]: S (3), min (3), max (3), sum of |p - c| (1), C upper triangle row major (21), n (1)
constexpr int kSumS = 0, kSumMin = 3, kSumMax = 6, kSumLen = 9, kSumC = 10, kSumN = 31, kSums = 32;

struct Eig { float X[36]; };                 // X[6 a + k]: component a of the k-th eigenvector, rounded to float
struct Head { uint32_t id; float mag[6]; };  // an entry of a sorted list: the point and its six magnitudes (28 bytes)

LSGPU_CS_HD bool nb_sample_ok(long long nb) { return nb >= 1 && nb <= (long long)kNbSampleMax; }
LSGPU_CS_HD bool torque_norm_ok(int t) { return t >= 0 && t <= 2; }

// |d|, sum of three terms left to right
LSGPU_CS_HD float length(float dx, float dy, float dz) { return sqrtf((dx * dx + dy * dy) + dz * dz); }

// v = (invL (d x n), n) with d = p - c
LSGPU_CS_HD void vec6(float px, float py, float pz, float nx, float ny, float nz, const float c[3], float invL, float v[6]) {
  const float dx = px - c[0], dy = py - c[1], dz = pz - c[2];
  const float mx = dy * nz - dz * ny, my = dz * nx - dx * nz, mz = dx * ny - dy * nx;
  v[0] = invL * mx; v[1] = invL * my; v[2] = invL * mz;
  v[3] = nx; v[4] = ny; v[5] = nz;
}

// mag_k = |v . X_k|, the six products added left to right
LSGPU_CS_HD float magnitude(const float v[6], const float* X, int k) {
  const float s = ((((v[0] * X[k] + v[1] * X[6 + k]) + v[2] * X[12 + k]) + v[3] * X[18 + k]) + v[4] * X[24 + k]) + v[5] * X[30 + k];
  return fabsf(s);
}

// The bits of a non-negative float order as unsigned integers; complemented, ascending keys are descending magnitudes, and a
// stable sort leaves equal magnitudes in ascending index order.  (A NaN magnitude -- inf - inf of an overflowed projection --
// has the largest bits: it sorts in front of everything, on host and device alike.)
LSGPU_CS_HD uint32_t sort_key(float mag) {
  return ~__builtin_bit_cast(uint32_t, mag);
}

// ---- host only from here

inline bool finite_sums(const double* s) {
  for (int k = 0; k < kSumN; ++k)
    if (!std::isfinite(s[k])) return false;
  return true;
}

inline void centre(const double* sums, int64_t n, float c[3]) {
  for (int a = 0; a < 3; ++a) c[a] = (float)(sums[kSumS + a] / (double)n);
}

// Lnorm of step 2 from the sums (sum of lengths: read at torqueNorm 1 only)
inline float lnorm(int torque_norm, const double* sums, int64_t n) {
  if (torque_norm == 0) return 1.f;
  if (torque_norm == 1) return (float)(sums[kSumLen] / (double)n);
  float e = (float)sums[kSumMax] - (float)sums[kSumMin];
  for (int a = 1; a < 3; ++a) {
    const float d = (float)sums[kSumMax + a] - (float)sums[kSumMin + a];
    if (d > e) e = d;
  }
  return e * 0.5f;
}

// Step 5: cyclic Jacobi on the symmetric 6 x 6 matrix whose upper triangle, row major, is C21.  X (nullable): the eigenvectors
// rounded to float, X[6 a + k]; values (nullable): the eigenvalues, ascending, ties by the original column.  Returns the
// sweeps done.
inline int eigen(const double C21[21], float X[36], double values[6]) {
  double A[6][6], V[6][6];
  for (int a = 0, k = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b, ++k) { A[a][b] = C21[k]; A[b][a] = C21[k]; }
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) V[a][b] = a == b ? 1.0 : 0.0;
  int sweeps = 0;
  for (; sweeps < 30; ++sweeps) {
    double off = 0.0;
    for (int p = 0; p < 6; ++p)
      for (int q = p + 1; q < 6; ++q) off += A[p][q] * A[p][q];
    if (off == 0.0) break;
    for (int p = 0; p < 6; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double at = std::fabs(theta) + std::sqrt(theta * theta + 1.0);
        const double t = theta < 0.0 ? -1.0 / at : 1.0 / at;
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < 6; ++k) {   // columns p and q of every row ...
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = cs * akp - sn * akq;
          A[k][q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < 6; ++k) {   // ... then rows p and q of every column
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = cs * apk - sn * aqk;
          A[q][k] = sn * apk + cs * aqk;
        }
        A[p][q] = 0.0; A[q][p] = 0.0;
        for (int k = 0; k < 6; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = cs * vkp - sn * vkq;
          V[k][q] = sn * vkp + cs * vkq;
        }
      }
  }
  int order[6] = {0, 1, 2, 3, 4, 5};
  for (int i = 1; i < 6; ++i)   // insertion sort: stable, ascending
    for (int j = i; j > 0 && A[order[j]][order[j]] < A[order[j - 1]][order[j - 1]]; --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
  for (int k = 0; k < 6; ++k) {
    if (values) values[k] = A[order[k]][order[k]];
    if (X)
      for (int a = 0; a < 6; ++a) X[6 * a + k] = (float)V[a][order[k]];
  }
  return sweeps;
}

// Step 8 over the heads of the six sorted lists: heads[k m + j], j < m, is the j-th entry of list k, m = min(nbSample, n)
// entries each.  Every entry popped is a chosen point and chosen points are distinct, so no list is read past m - 1.
// out_ids: room for nb; chosen: scratch, resized to n bits.  Returns the points chosen (nb), or -1 if a list ran out (it cannot).
inline int64_t walk(const Head* heads, int64_t m, int64_t n, int64_t nb, uint32_t* out_ids, std::vector<uint64_t>& chosen) {
  chosen.assign((size_t)((n + 63) / 64), 0ull);
  float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int64_t pos[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t s = 0; s < nb; ++s) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
      if (t[k] > t[i]) k = i;
    const Head* list = heads + (size_t)k * (size_t)m;
    while (pos[k] < m && (int64_t)list[pos[k]].id < n && ((chosen[list[pos[k]].id >> 6] >> (list[pos[k]].id & 63u)) & 1ull)) ++pos[k];
    if (pos[k] >= m || (int64_t)list[pos[k]].id >= n) return -1;
    const Head& e = list[pos[k]++];
    chosen[e.id >> 6] |= 1ull << (e.id & 63u);
    out_ids[s] = e.id;
    for (int j = 0; j < 6; ++j) t[j] += e.mag[j] * e.mag[j];
  }
  return nb;
}

}  // namespace covs
}  // namespace lsgpu
