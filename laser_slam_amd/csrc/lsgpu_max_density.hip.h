// lsgpu_max_density.hip.h -- MaxDensityDataPointsFilter behind SurfaceNormalDataPointsFilter (keepDensities 1) in the
// reference section of an ICP chain (include/lsgpu_icp.h, "MaxDensityDataPointsFilter"; DESIGN.md §3 "Thinning the dense
// near range").  A point whose density exceeds maxDensity takes one draw and is kept with probability maxDensity / density;
// every other point is kept.  The pass follows k_cut_pass (lsgpu_chain_cut.hip.h): 256-thread blocks, the rank inside a block
// from cut_block_rank, block counts and their scans, no flag array:
//   k_md_pass<0>  the block's count of dense points -> cnt[block]; the minimum and the maximum of the non-NaN densities and the
//                 number of NaN ones -> stat[0..2] (densities are >= 0: their bits order as unsigned integers)
//   scan          exclusive, over the block counts
//   k_md_pass<1>  rank among the dense points -> the point's draw; keep; the block's count of kept points -> cnt[block]
//   scan
//   k_md_pass<2>  the same again; the kept point AS GIVEN to out_pts[rank], its normal -- gathered through inv from the
//                 Morton-sorted normals the snf kernels have just written -- to out_nrm[3 rank ..]: only kept points pay the
//                 scattered 16-byte read
// plus the k_to_host launch that sends the two totals (dense, kept).  The draw of a dense point is indexed by its rank among
// the dense points: the sequential filter draws once per dense point, in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lsgpu_chain_cut.hip.h"
#include "lsgpu_density.h"

namespace lsgpu {

// stat: {min bits, max bits, NaN count, unused}; before stage 0: {0xFFFFFFFF, 0, 0, 0}
struct MdStat { uint32_t lo, hi, nan, pad; };

// last = the largest non-NaN density; sat = 0 iff every point's density equals it
__device__ __forceinline__ void md_last_sat(const MdStat& s, float* last, int* sat) {
  *last = __uint_as_float(s.hi);
  *sat = (s.lo == s.hi && s.nan == 0u) ? 0 : 1;
}

// One point per thread, block b = points [256 b, 256 b + 256).  dens: the density of point i (the cloud's own order).
// draws: at least as many as there can be dense points (n).  inv: index in the cloud -> position in the sorted normals nrm
// (nrm nullable: a handle that reads no normals; out_nrm is then not written).  out_pts: room for n points; not src.
template <int STAGE>
__global__ __launch_bounds__(256) void k_md_pass(const float4* __restrict__ src, const float* __restrict__ dens, int n,
                                                 float max_density, const float* __restrict__ draws, MdStat* __restrict__ stat,
                                                 const uint32_t* __restrict__ off_dense, const uint32_t* __restrict__ off_keep,
                                                 uint32_t* __restrict__ cnt, const uint32_t* __restrict__ inv,
                                                 const float4* __restrict__ nrm, float4* __restrict__ out_pts,
                                                 float* __restrict__ out_nrm) {
  __shared__ uint32_t ws_dense[4], ws_keep[4], ws_lo[4], ws_hi[4], ws_nan[4];
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  const bool valid = i < n;
  const float d = valid ? dens[i] : 0.f;
  const bool dense = valid && density::is_dense(d, max_density);
  uint32_t total = 0;
  if (STAGE == 0) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool num = valid && d == d;
    uint32_t lo = num ? __float_as_uint(d) : 0xFFFFFFFFu, hi = num ? __float_as_uint(d) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
      hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
    }
    const uint32_t nn = (uint32_t)__popcll(__ballot(valid && !num));
    if (lane == 0) { ws_lo[w] = lo; ws_hi[w] = hi; ws_nan[w] = nn; }
    cut_block_rank(dense, ws_dense, &total);   // (synchronises: the words above are visible behind it)
    if (threadIdx.x == 0) {
      cnt[blockIdx.x] = total;
      atomicMin(&stat->lo, min(min(ws_lo[0], ws_lo[1]), min(ws_lo[2], ws_lo[3])));
      atomicMax(&stat->hi, max(max(ws_hi[0], ws_hi[1]), max(ws_hi[2], ws_hi[3])));
      const uint32_t nans = ws_nan[0] + ws_nan[1] + ws_nan[2] + ws_nan[3];
      if (nans) atomicAdd(&stat->nan, nans);
    }
    return;
  }
  const uint32_t r = cut_block_rank(dense, ws_dense, &total);
  float last; int sat;
  md_last_sat(*stat, &last, &sat);
  // (&&: only a dense point reads a draw)
  const bool keep = valid && (!dense || density::keeps(d, max_density, last, sat, draws[off_dense[blockIdx.x] + r]));
  const uint32_t rk = cut_block_rank(keep, ws_keep, &total);
  if (STAGE == 1) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    return;
  }
  if (keep) {
    const size_t o = (size_t)off_keep[blockIdx.x] + rk;
    out_pts[o] = src[i];
    if (nrm) {
      const float4 v = nrm[inv[i]];
      out_nrm[3 * o + 0] = v.x; out_nrm[3 * o + 1] = v.y; out_nrm[3 * o + 2] = v.z;
    }
  }
}

}  // namespace lsgpu
