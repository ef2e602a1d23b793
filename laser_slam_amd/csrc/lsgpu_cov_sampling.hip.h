// lsgpu_cov_sampling.hip.h -- CovarianceSamplingDataPointsFilter on the device (include/lsgpu_icp.h,
// "CovarianceSamplingDataPointsFilter"; DESIGN.md §3 of the same name; lsgpu_cov_sampling.h has the arithmetic host and device
// share).  The passes, in the order lsgpu_icp_filter_cov_sampling enqueues them:
//   k_cs_pass<0>  sum of the points in double, minimum and maximum per axis               -> 9 columns per block
//   k_cs_pass<1>  sum of |p - c| in double (torqueNorm 1 only)                             -> 1 column
//   k_cs_pass<2>  the 6-vector of every point, the 21 sums of its products in double      -> 21 columns
//   k_cs_final    the rows of a pass combined in a fixed order by one block (k_cov_final's shape)
//   k_cs_project  the 6-vector again, its six magnitudes -> mag[6 i ..]
//   k_cs_keys     list k: key = complemented bits of mag_k, value = the index; the stable radix sort (lsgpu_sort.hip.h) follows
//   k_cs_heads    the first m entries of the sorted list: index + the six magnitudes of that point, 28 bytes each
//   k_cs_gather   the chosen points and normals in pick order
// The passes follow k_cov (lsgpu_cov.hip.h): grid stride, registers, a wave reduction, four wave results through LDS, one row
// of double partials per block.  No atomics and no dependence on the order blocks arrive in: reproducible run to run.
#pragma once
#include "lsgpu_common.hip.h"
#include "lsgpu_cov_sampling.h"

namespace lsgpu {

constexpr int kCsStride = 32;        // doubles per row of partials
constexpr int kCsBlocksMax = 1024;   // rows

struct CsParams { float c[3]; float invL; };

__device__ __forceinline__ double cs_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = w < v ? w : v; }
  return v;
}
__device__ __forceinline__ double cs_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  return v;
}
// how column `col` of pass `pass` combines: 0 sum, 1 minimum, 2 maximum
__host__ __device__ inline int cs_op(int pass, int col) { return pass != 0 || col < 3 ? 0 : col < 6 ? 1 : 2; }
__host__ __device__ inline int cs_cols(int pass) { return pass == 0 ? 9 : pass == 1 ? 1 : 21; }
__device__ __forceinline__ double cs_combine(int op, double a, double b) { return op == 0 ? a + b : op == 1 ? (b < a ? b : a) : (b > a ? b : a); }

// pts: n points as given; nrm3: 3 floats per point (PASS 2 only); partials: gridDim.x rows of kCsStride doubles
template <int PASS>
__global__ __launch_bounds__(256) void k_cs_pass(const float4* __restrict__ pts, const float* __restrict__ nrm3, int n, CsParams q,
                                                 double* __restrict__ partials) {
  constexpr int NC = PASS == 0 ? 9 : PASS == 1 ? 1 : 21;
  __shared__ double red[4][NC];
  double acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.0;
  if (PASS == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { acc[3 + a] = (double)INFINITY; acc[6 + a] = -(double)INFINITY; }
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 p = pts[i];
    if (PASS == 0) {
      const double v[3] = {(double)p.x, (double)p.y, (double)p.z};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        acc[a] += v[a];
        acc[3 + a] = v[a] < acc[3 + a] ? v[a] : acc[3 + a];
        acc[6 + a] = v[a] > acc[6 + a] ? v[a] : acc[6 + a];
      }
    } else if (PASS == 1) {
      acc[0] += (double)covs::length(p.x - q.c[0], p.y - q.c[1], p.z - q.c[2]);
    } else {
      float v[6];
      covs::vec6(p.x, p.y, p.z, nrm3[3 * (size_t)i + 0], nrm3[3 * (size_t)i + 1], nrm3[3 * (size_t)i + 2], q.c, q.invL, v);
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = a; b < 6; ++b, ++k) acc[k] += (double)v[a] * (double)v[b];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int op = cs_op(PASS, k);
    acc[k] = op == 0 ? wave_sum(acc[k]) : op == 1 ? cs_wave_min(acc[k]) : cs_wave_max(acc[k]);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NC; ++k) red[w][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    const int op = cs_op(PASS, (int)threadIdx.x);
    double r = red[0][threadIdx.x];
    for (int ww = 1; ww < 4; ++ww) r = cs_combine(op, r, red[ww][threadIdx.x]);
    partials[(size_t)blockIdx.x * kCsStride + threadIdx.x] = r;
  }
}

// 1024 threads = 16 groups of 64: group g combines rows g, g + 16, ... of its column, then the 16 group results are combined
// in a fixed order.  out: cs_cols(pass) doubles.
__global__ __launch_bounds__(1024) void k_cs_final(const double* __restrict__ partials, int nblocks, int pass, double* __restrict__ out) {
  __shared__ double sh[16][65];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int ncol = cs_cols(pass), op = cs_op(pass, col);
  const double unit = op == 0 ? 0.0 : op == 1 ? (double)INFINITY : -(double)INFINITY;
  double s = unit;
  if (col < ncol)
    for (int b = grp; b < nblocks; b += 16) s = cs_combine(op, s, partials[(size_t)b * kCsStride + col]);
  sh[grp][col] = s;
  __syncthreads();
  if ((int)threadIdx.x < ncol) {
    double t = unit;
    for (int r = 0; r < 16; ++r) t = cs_combine(op, t, sh[r][threadIdx.x]);
    out[threadIdx.x] = t;
  }
}

// mag: 6 floats per point
__global__ __launch_bounds__(256) void k_cs_project(const float4* __restrict__ pts, const float* __restrict__ nrm3, int n, CsParams q,
                                                    covs::Eig e, float* __restrict__ mag) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  const float4 p = pts[i];
  float v[6];
  covs::vec6(p.x, p.y, p.z, nrm3[3 * (size_t)i + 0], nrm3[3 * (size_t)i + 1], nrm3[3 * (size_t)i + 2], q.c, q.invL, v);
#pragma unroll
  for (int k = 0; k < 6; ++k) mag[6 * (size_t)i + k] = covs::magnitude(v, e.X, k);
}

// the pairs of list k in index order (the sort reads the low 32 key bits)
__global__ __launch_bounds__(256) void k_cs_keys(const float* __restrict__ mag, int n, int k, uint64_t* __restrict__ keys,
                                                 uint32_t* __restrict__ vals) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n) return;
  keys[i] = (uint64_t)covs::sort_key(mag[6 * (size_t)i + k]);
  vals[i] = (uint32_t)i;
}

// sorted: the point indices of a list by decreasing magnitude; heads: room for m entries (m <= n)
__global__ __launch_bounds__(256) void k_cs_heads(const uint32_t* __restrict__ sorted, int m, int n, const float* __restrict__ mag,
                                                  covs::Head* __restrict__ heads) {
  const int j = (int)(blockIdx.x * 256u + threadIdx.x);
  if (j >= m) return;
  const uint32_t id = sorted[j];
  covs::Head hd;
  hd.id = id;
#pragma unroll
  for (int k = 0; k < 6; ++k) hd.mag[k] = id < (uint32_t)n ? mag[6 * (size_t)id + k] : 0.f;   // (a sorted value is an index < n)
  heads[j] = hd;
}

// ids: m chosen indices in pick order, each < n; out_pts / out_nrm / out_ids: room for m points
__global__ __launch_bounds__(256) void k_cs_gather(const float4* __restrict__ pts, const float* __restrict__ nrm3,
                                                   const uint32_t* __restrict__ ids, int m, int n, float4* __restrict__ out_pts,
                                                   float* __restrict__ out_nrm, int32_t* __restrict__ out_ids) {
  const int j = (int)(blockIdx.x * 256u + threadIdx.x);
  if (j >= m) return;
  const uint32_t id = ids[j];
  if (id >= (uint32_t)n) return;
  out_pts[j] = pts[id];
#pragma unroll
  for (int a = 0; a < 3; ++a) out_nrm[3 * (size_t)j + a] = nrm3[3 * (size_t)id + a];
  out_ids[j] = (int32_t)id;
}

}  // namespace lsgpu
