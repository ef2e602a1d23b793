// lsgpu_chain_cut.hip.h -- the cut modules of an ICP chain's filter sections (include/lsgpu_icp.h, "cut modules in the ICP
// chain"): MaxDist-, MinDist-, BoundingBox- and RemoveNaNDataPointsFilter in front of the sampling / normals modules of
// readingDataPointsFilters and referenceDataPointsFilters, evaluated inside lsgpu_icp_compute.
//
// One set of predicates (cut_keep_dist / _box / _nan) serves the input filter chain's k_point_filter_select (lsgpu_ssn.hip.h),
// which runs one module per launch, and k_cut_pass below, which runs a whole section -- up to kCutMax modules, by value in the kernel's
// arguments -- on a point in one go.  A section costs the same launches whatever it holds:
//   without RandomSampling   k_cut_pass<0>  the block's count of survivors            -> cnt_a[block]
//                            scan           exclusive, over the nb = ceil(n / 256) block counts (one launch up to 1 M points)
//                            k_cut_pass<2>  the predicate again, rank = off_a[block] + rank in the block, out[rank] = p
//   with RandomSampling      k_cut_pass<0>  counts `pre`: the survivors of the modules IN FRONT of the sampling module
//                            scan
//                            k_cut_pass<1>  rank of `pre` -> the point's draw; keep = pre && draw < prob && post; counts keep
//                            scan
//                            k_cut_pass<2>  the same again, rank of keep, out[rank] = p
//   a cloud with normals     k_cut_pass<2, RS, true> in place of k_cut_pass<2, RS>: the normal of a kept point goes with it
// plus the one k_to_host launch that sends the totals.  There is no flag array and no per-point scan: the rank inside a block
// is a wave64 ballot + popcount and four wave totals in LDS, the only arrays are the nb block counts and their offsets.  The
// predicate is evaluated two or three times per point instead -- it is a handful of compares on a float4 the compaction
// reads anyway (16 B per point and pass, 4 B more for a draw).
// The draw of a point is indexed by its rank among `pre`: RandomSampling draws once per point that reaches it, in order,
// so draws[rank] is the draw the sequential chain would have made for it, and the `pre` total is the number consumed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsgpu {

constexpr int kCutMax = 8;   // == LSGPU_CHAIN_CUT_MAX

struct CutModuleDev { int type, dim, flag; float v[6]; };
// modules [0, n_pre) stand in front of RandomSampling, [n_pre, n) behind it (no RandomSampling: n_pre == n)
struct CutSectionDev { int n, n_pre; CutModuleDev m[kCutMax]; };

// The predicates of the stateless per-point modules, one function each, F: anything with type, dim, flag and v[6].
// Max- / MinDist (f.type 1 / 2).  Upstream asymmetry (libpointmatcher MaxDist.cpp / MinDist.cpp, from knowledge): the radial
// branch of both compares the norm with |limit|; on ONE axis MaxDist compares the SIGNED coordinate (x < maxDist keeps every
// negative x), MinDist the absolute one
template <class F>
__device__ __forceinline__ bool cut_keep_dist(const float4& p, const F& f) {
  const float c = f.dim == 0 ? p.x : f.dim == 1 ? p.y : p.z;
  if (f.dim < 0) {
    const float val = sqrtf(__fmaf_rn(p.z, p.z, __fmaf_rn(p.y, p.y, p.x * p.x)));
    return f.type == 1 ? val < fabsf(f.v[0]) : val > fabsf(f.v[0]);
  }
  return f.type == 1 ? c < f.v[0] : fabsf(c) > f.v[0];
}
template <class F>
__device__ __forceinline__ bool cut_keep_box(const float4& p, const F& f) {   // BoundingBox
  const bool in = p.x > f.v[0] && p.x < f.v[1] && p.y > f.v[2] && p.y < f.v[3] && p.z > f.v[4] && p.z < f.v[5];
  return f.flag ? !in : in;
}
// RemoveNaN: a column with a NaN in any feature row goes (colArray == colArray).all()
__device__ __forceinline__ bool cut_keep_nan(const float4& p) { return p.x == p.x && p.y == p.y && p.z == p.z && p.w == p.w; }

// Does point p survive module f (LSGPU_FILTER_MAX_DIST / _MIN_DIST / _BOUNDING_BOX / _REMOVE_NAN; any other type keeps it)?
template <class F>
__device__ __forceinline__ bool point_cut_keep(const float4& p, const F& f) {
  if (f.type == 1 || f.type == 2) return cut_keep_dist(p, f);
  if (f.type == 3) return cut_keep_box(p, f);
  if (f.type == 6) return cut_keep_nan(p);
  return true;
}

// Rank of this thread among the block's threads with `flag` (threads in front of it only), and the block's total.  Every
// thread of the 256-thread block calls it (it synchronises); ws: four words of LDS of this call's own.
__device__ __forceinline__ uint32_t cut_block_rank(bool flag, uint32_t* ws, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  const uint32_t in_wave = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) ws[w] = (uint32_t)__popcll(b);
  __syncthreads();
  const uint32_t s0 = ws[0], s1 = ws[1], s2 = ws[2], s3 = ws[3];
  *total = s0 + s1 + s2 + s3;
  return in_wave + (w > 0 ? s0 : 0u) + (w > 1 ? s1 : 0u) + (w > 2 ? s2 : 0u);
}

// One point per thread, block b = points [256 b, 256 b + 256).  STAGE 0: cnt[b] = the block's `pre`.  STAGE 1 (RS): cnt[b] =
// the block's kept points.  STAGE 2: the kept points to out, order preserved.  RS: the section has RandomSampling -- off_pre
// = exclusive scan of stage 0's counts, off_keep = of stage 1's; without it the kept points are `pre` and off_keep is the
// scan of stage 0's counts.  draws: at least as many as `pre` can count (n).  out: room for n points; not src.
// NRM (stage 2 of a cloud that carries normals somebody reads; include/lsgpu_icp.h, "carried normals"): the point's normal goes
// with it, out_nrm[3 rank ..] = nrm[3 i ..] -- nrm: 3 floats per point of src, out_nrm: room for 3 n floats, not nrm.  No other
// stage reads a normal.
template <int STAGE, bool RS, bool NRM = false>
__global__ __launch_bounds__(256) void k_cut_pass(const float4* __restrict__ src, int n, CutSectionDev cs,
                                                  const float* __restrict__ draws, float prob,
                                                  const uint32_t* __restrict__ off_pre, const uint32_t* __restrict__ off_keep,
                                                  uint32_t* __restrict__ cnt, float4* __restrict__ out,
                                                  const float* __restrict__ nrm, float* __restrict__ out_nrm) {
  __shared__ uint32_t ws_pre[4], ws_keep[4];
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  bool pre = false, post = false;
  if (i < n) {
    p = src[i];
    pre = true; post = true;
#pragma unroll
    for (int k = 0; k < kCutMax; ++k) {   // (unrolled: every module is read from the kernel's arguments at a constant offset)
      if (k < cs.n) {
        const bool ok = point_cut_keep(p, cs.m[k]);
        if (k < cs.n_pre) pre = pre && ok; else post = post && ok;
      }
    }
  }
  bool keep = pre;
  uint32_t total = 0;
  if (STAGE == 0 || RS) {
    const uint32_t r = cut_block_rank(pre, ws_pre, &total);
    if (STAGE == 0) {
      if (threadIdx.x == 0) cnt[blockIdx.x] = total;
      return;
    }
    keep = pre && draws[off_pre[blockIdx.x] + r] < prob && post;   // (&&: only a point that reaches the module reads a draw)
  }
  const uint32_t rk = cut_block_rank(keep, ws_keep, &total);
  if (STAGE == 1) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    return;
  }
  if (!keep) return;
  const uint32_t at = off_keep[blockIdx.x] + rk;
  out[at] = p;
  if (NRM) {
    const float* a = nrm + 3 * (size_t)i;
    float* o = out_nrm + 3 * (size_t)at;
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
  }
}

}  // namespace lsgpu
