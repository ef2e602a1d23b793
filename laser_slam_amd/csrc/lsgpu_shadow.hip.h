// lsgpu_shadow.hip.h -- ShadowDataPointsFilter behind the module that produces the normals, in either filter section of an
// ICP chain (include/lsgpu_icp.h, "ShadowDataPointsFilter"; DESIGN.md §3 "ShadowDataPointsFilter").  A point whose normal is
// nearly perpendicular to the ray that observed it is dropped (lsgpu_shadow.h has the predicate); the survivors and their
// normals are compacted together, order preserved.  The pass follows k_cut_pass (lsgpu_chain_cut.hip.h) and k_md_pass
// (lsgpu_max_density.hip.h): 256-thread blocks, the rank inside a block from cut_block_rank, block counts and their scan, no
// flag array:
//   k_shadow_pass<0>  the block's count of kept points -> cnt[block]
//   scan              exclusive, over the block counts
//   k_shadow_pass<2>  the predicate again; the kept point to out_pts[rank], its normal to out_nrm[3 rank ..]
// plus the k_to_host launch that sends the total.  Every point reads its normal in both stages (the predicate needs it):
// GATHER false -- 3 packed floats per point in the cloud's own order (the sampling filter's or the thinning pass's output, the
// reading's unpermuted normals); GATHER true -- the Morton-sorted float4 normals the snf kernels have just written, through
// inv as k_md_pass<2> reads them.  28 B read per point and pass without the gather, 36 B (one scattered 16 B read) with it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lsgpu_chain_cut.hip.h"
#include "lsgpu_shadow.h"

namespace lsgpu {

// One point per thread, block b = points [256 b, 256 b + 256).  src: the points as given to the section (not centred).
// GATHER false: nrm3 = 3 floats per point, the cloud's order; inv and nrm4 are not read.  GATHER true: nrm4[inv[i]] is the normal
// of point i; nrm3 is not read.  STAGE 0: cnt[b] = the block's kept points.  STAGE 2: off = exclusive scan of the counts;
// out_pts / out_nrm: room for n points / 3 n floats; neither is an input.
template <int STAGE, bool GATHER>
__global__ __launch_bounds__(256) void k_shadow_pass(const float4* __restrict__ src, const float* __restrict__ nrm3,
                                                     const uint32_t* __restrict__ inv, const float4* __restrict__ nrm4, int n,
                                                     float eps, const uint32_t* __restrict__ off, uint32_t* __restrict__ cnt,
                                                     float4* __restrict__ out_pts, float* __restrict__ out_nrm) {
  __shared__ uint32_t ws_keep[4];
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  float nx = 0.f, ny = 0.f, nz = 0.f;
  bool keep = false;
  if (i < n) {
    p = src[i];
    if (GATHER) {
      const float4 v = nrm4[inv[i]];
      nx = v.x; ny = v.y; nz = v.z;
    } else {
      nx = nrm3[3 * (size_t)i + 0]; ny = nrm3[3 * (size_t)i + 1]; nz = nrm3[3 * (size_t)i + 2];
    }
    keep = shadow::keeps(p.x, p.y, p.z, nx, ny, nz, eps);
  }
  uint32_t total = 0;
  const uint32_t rk = cut_block_rank(keep, ws_keep, &total);
  if (STAGE == 0) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    return;
  }
  if (keep) {
    const size_t o = (size_t)off[blockIdx.x] + rk;   // (< n: the rank among the kept points in front of this one)
    out_pts[o] = p;
    out_nrm[3 * o + 0] = nx; out_nrm[3 * o + 1] = ny; out_nrm[3 * o + 2] = nz;
  }
}

}  // namespace lsgpu
