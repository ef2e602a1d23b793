// lsgpu_voxel_filter.hip.h -- VoxelGridDataPointsFilter of the input filter chain on the device (include/lsgpu_icp.h has
// the contract, lsgpu_voxel_filter.h the arithmetic it shares with the host twin).
//
// The module is the one in the chain that WRITES points instead of keeping a subset: keys -> the library's stable radix
// sort (a run of equal keys is a voxel, its points in input order, its head the voxel's first point) -> k_vgf_reduce forms
// the voxel's point and puts it where the FIRST point stood -> the chain's scan + k_compact_points over input positions,
// which leaves the voxels in the order of their first points without a second sort.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsgpu_voxel_filter.h"

namespace lsgpu {

// voxel index of every point (key), input index (value)
__global__ __launch_bounds__(256) void k_vgf_keys(const float4* __restrict__ p, int n, voxelf::Geom g,
                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 v = p[i];
  keys[i] = (uint64_t)voxelf::voxel_index(g, v.x, v.y, v.z);
  vals[i] = (uint32_t)i;
}

// One thread per SORTED position.  idx[i] is an input index and every input index appears once, so every keep[] word is
// written: 1 at a voxel's first point, 0 at every other point.  The head of a run walks it: s starts as the first point's
// coordinate, every further point is added in input order (the stable sort's order), s / (float)count -- one lane, one float
// sum per voxel, however long the run (upstream's summation order; a parallel sum would round differently).
// use_centroid 0: the voxel's centre instead, from the key.  out[first].w = the first point's fourth component.
// `out` has n entries and is none of p and the chain's two buffers.
__global__ __launch_bounds__(256) void k_vgf_reduce(const float4* __restrict__ p, const uint64_t* __restrict__ keys,
                                                    const uint32_t* __restrict__ idx, int n, voxelf::Geom g, int use_centroid,
                                                    float4* __restrict__ out, uint32_t* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  const uint32_t first = idx[i];
  if (i > 0 && keys[i - 1] == key) { keep[first] = 0u; return; }
  const float4 v0 = p[first];
  float4 r;
  if (use_centroid) {
    float sx = v0.x, sy = v0.y, sz = v0.z;
    int j = i + 1;
    for (; j < n && keys[j] == key; ++j) {
      const float4 v = p[idx[j]];
      sx += v.x; sy += v.y; sz += v.z;
    }
    const float c = (float)(j - i);
    r = make_float4(sx / c, sy / c, sz / c, v0.w);
  } else {
    const uint32_t k32 = (uint32_t)key, nxy = g.ndiv[0] * g.ndiv[1];
    const uint32_t ck = k32 / nxy, rem = k32 - ck * nxy, cj = rem / g.ndiv[0], ci = rem - cj * g.ndiv[0];
    r = make_float4(voxelf::centre(g, 0, ci), voxelf::centre(g, 1, cj), voxelf::centre(g, 2, ck), v0.w);
  }
  out[first] = r;
  keep[first] = 1u;
}

}  // namespace lsgpu
