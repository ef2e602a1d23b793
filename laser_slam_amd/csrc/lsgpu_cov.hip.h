// lsgpu_cov.hip.h -- PointToPlaneWithCovErrorMinimizer on the device: the sums of Censi's closed-form covariance over the
// pairs of one iteration (include/lsgpu_icp.h "PointToPlaneWithCovErrorMinimizer" states the arithmetic).
//   k_cov        one grid-stride pass in the mould of k_normal_eq: per kept pair the three 6-vectors h, a, b in float, then
//                21 + 21 upper-triangle products and sums in double, the pair count and the squared plane residual;
//                wave_sum, LDS, one row of partials per block
//   k_cov_final  the rows added in a fixed order by one block
//   k_cov_unpermute_points  the loop's sorted, moved reading back in the caller's order (the pass after the loop sums in the
//                order lsgpu_point_to_plane_cov sums in, so the two agree bit for bit)
// No atomics and no dependence on the order blocks arrive in: the result is reproducible run to run.  The kernel runs once
// per alignment: 44 double accumulators per lane are kept in registers (no scratch), occupancy is not what it is after.
#pragma once
#include "lsgpu_common.hip.h"

namespace lsgpu {

constexpr int kCov = 44;         // 21 of H, 21 of M, count, sum (n . (p - q))^2
constexpr int kCovStride = 48;   // doubles per row of partials

struct CovStep { float w[3]; float t[3]; };   // {alpha, beta, gamma}, {tx, ty, tz} of the iteration's step (lsgpu_cov.h)

// IDS_ORIG: ids index the reference as given to set_reference (inv maps them to the sorted reference)
template <bool IDS_ORIG>
__global__ __launch_bounds__(256) void k_cov(const float4* __restrict__ rdq, int nq, Mat34 T,
                                             const int* __restrict__ ids, const float* __restrict__ d2,
                                             const float4* __restrict__ pts, const float4* __restrict__ nrm,
                                             const uint32_t* __restrict__ inv, uint32_t nr, float limit, float lo2,
                                             CovStep s, double* __restrict__ partials) {
  __shared__ double red[4][kCov];
  double accH[21], accM[21];
  double cnt = 0.0, rss = 0.0;
#pragma unroll
  for (int k = 0; k < 21; ++k) { accH[k] = 0.0; accM[k] = 0.0; }
  for (int j = blockIdx.x * 256 + threadIdx.x; j < nq; j += gridDim.x * 256) {
    const float d = d2[j];
    int id = ids[j];
    if (!(d <= limit) || !(lo2 <= d) || (uint32_t)id >= nr) continue;   // (a negative id is an invalid match)
    if (IDS_ORIG) id = (int)inv[id];
    const float4 r = rdq[j];
    const float3 p = xform(T, r.x, r.y, r.z);
    const float4 q = pts[id];
    const float4 n = nrm[id];
    const float rp = sqrtf((p.x * p.x + p.y * p.y) + p.z * p.z);
    const float rq = sqrtf((q.x * q.x + q.y * q.y) + q.z * q.z);
    const float ux = p.x / rp, uy = p.y / rp, uz = p.z / rp;
    const float vx = q.x / rq, vy = q.y / rq, vz = q.z / rq;
    const float mx = uy * n.z - uz * n.y, my = uz * n.x - ux * n.z, mz = ux * n.y - uy * n.x;
    const float cx = s.w[1] * p.z - s.w[2] * p.y, cy = s.w[2] * p.x - s.w[0] * p.z, cz = s.w[0] * p.y - s.w[1] * p.x;
    const float gx = s.w[1] * uz - s.w[2] * uy, gy = s.w[2] * ux - s.w[0] * uz, gz = s.w[0] * uy - s.w[1] * ux;
    const float ex = ((p.x + cx) + s.t[0]) - q.x, ey = ((p.y + cy) + s.t[1]) - q.y, ez = ((p.z + cz) + s.t[2]) - q.z;
    const float E = (n.x * ex + n.y * ey) + n.z * ez;
    const float Nrd = (n.x * (ux + gx) + n.y * (uy + gy)) + n.z * (uz + gz);
    const float Nrf = -((n.x * vx + n.y * vy) + n.z * vz);
    const float ar = E + rp * Nrd;
    const float hv[6] = {n.x, n.y, n.z, rp * mx, rp * my, rp * mz};
    const float av[6] = {n.x * Nrd, n.y * Nrd, n.z * Nrd, mx * ar, my * ar, mz * ar};
    const float bv[6] = {n.x * Nrf, n.y * Nrf, n.z * Nrf, (rq * mx) * Nrf, (rq * my) * Nrf, (rq * mz) * Nrf};
    const float res = (p.x - q.x) * n.x + (p.y - q.y) * n.y + (p.z - q.z) * n.z;   // as k_normal_eq
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c = a; c < 6; ++c, ++k) {
        accH[k] += (double)hv[a] * (double)hv[c];
        accM[k] += (double)av[a] * (double)av[c] + (double)bv[a] * (double)bv[c];
      }
    }
    cnt += 1.0;
    rss += (double)res * (double)res;
  }
#pragma unroll
  for (int k = 0; k < 21; ++k) { accH[k] = wave_sum(accH[k]); accM[k] = wave_sum(accM[k]); }
  cnt = wave_sum(cnt); rss = wave_sum(rss);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 21; ++k) { red[w][k] = accH[k]; red[w][21 + k] = accM[k]; }
    red[w][42] = cnt; red[w][43] = rss;
  }
  __syncthreads();
  if (threadIdx.x < kCov)
    partials[(size_t)blockIdx.x * kCovStride + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// 1024 threads = 16 groups of 64: group g adds rows g, g + 16, ... of its column, then the 16 group sums are added in a
// fixed order
__global__ __launch_bounds__(1024) void k_cov_final(const double* __restrict__ partials, int nblocks,
                                                    double* __restrict__ out) {
  __shared__ double sh[16][65];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  double s = 0.0;
  if (col < kCov)
    for (int b = grp; b < nblocks; b += 16) s += partials[(size_t)b * kCovStride + col];
  sh[grp][col] = s;
  __syncthreads();
  if (threadIdx.x < kCov) {
    double t = 0.0;
    for (int r = 0; r < 16; ++r) t += sh[r][threadIdx.x];
    out[threadIdx.x] = t;
  }
}

// the sorted reading (w = caller index) -> the caller's order; the caller index is < nq by construction (k_query_gather)
__global__ __launch_bounds__(256) void k_cov_unpermute_points(const float4* __restrict__ rdq, int nq,
                                                              float4* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nq) return;
  const float4 r = rdq[j];
  const uint32_t o = __float_as_uint(r.w);
  if (o < (uint32_t)nq) out[o] = make_float4(r.x, r.y, r.z, 1.f);
}

}  // namespace lsgpu
