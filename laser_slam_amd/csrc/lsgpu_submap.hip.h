// lsgpu_submap.hip.h -- sub-map assembly for clouds that carry normals (include/lsgpu_icp.h, "carried normals"):
// submap = concat_i ( T_i * cloud_i ), the points AND the normals of every member, in one launch.
//
// Composed from k_transform and k_rotate3 the assembly would cost two short launches per member in front of a compute that
// is a chain of short launches already.  Here the members stand in a table in the kernel's arguments -- first output
// index, source pointers, the transform's rows, identity flag -- and a thread finds its member by search over the first
// indices: a block may span any number of members, empty ones included.  A sub-map of more members than the table holds
// goes out as one launch per member (the table then holds one).
//
// The arithmetic is that of k_transform (points: xform, w kept) and k_rotate3 (normals: the rotation's rows, the same fma
// chain).  A member flagged identity is copied bit for bit -- Inf, NaN and w included -- as the plain path's
// device-to-device copy does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lsgpu_common.hip.h"

namespace lsgpu {

constexpr int kSubmapMembers = 16;

struct SubmapTable {
  int n;                                // members in the table, 1 .. kSubmapMembers
  uint32_t first[kSubmapMembers + 1];   // member m writes out[first[m] .. first[m + 1]); first[n] closes the last one
  const float4* pts[kSubmapMembers];
  const float* nrm[kSubmapMembers];     // 3 floats per point
  Mat34 T[kSubmapMembers];
  int identity[kSubmapMembers];
};

// One output point per thread: thread j writes out[first[0] + j].  out_pts / out_nrm: room for first[n] points.
__global__ __launch_bounds__(256) void k_assemble_submap(SubmapTable tab, float4* __restrict__ out_pts, float* __restrict__ out_nrm) {
  const uint32_t i = tab.first[0] + blockIdx.x * 256u + threadIdx.x;
  if (i >= tab.first[tab.n]) return;
  // the last member whose first index is not behind i: an empty member shares its first index with the one behind it,
  // which the count steps over
  int m = 0;
#pragma unroll
  for (int k = 1; k < kSubmapMembers; ++k)
    if (k < tab.n && tab.first[k] <= i) m = k;
  const uint32_t s = i - tab.first[m];
  const float4 p = tab.pts[m][s];
  const float* nsrc = tab.nrm[m] + 3 * (size_t)s;
  const float x = nsrc[0], y = nsrc[1], z = nsrc[2];
  float* o = out_nrm + 3 * (size_t)i;
  if (tab.identity[m]) {
    out_pts[i] = p;
    o[0] = x; o[1] = y; o[2] = z;
    return;
  }
  const Mat34 T = tab.T[m];
  const float3 q = xform(T, p.x, p.y, p.z);
  out_pts[i] = make_float4(q.x, q.y, q.z, p.w);
  o[0] = __fmaf_rn(T.m[2], z, __fmaf_rn(T.m[1], y, T.m[0] * x));
  o[1] = __fmaf_rn(T.m[6], z, __fmaf_rn(T.m[5], y, T.m[4] * x));
  o[2] = __fmaf_rn(T.m[10], z, __fmaf_rn(T.m[9], y, T.m[8] * x));
}

}  // namespace lsgpu
