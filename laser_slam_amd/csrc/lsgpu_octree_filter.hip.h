// lsgpu_octree_filter.hip.h -- OctreeGridDataPointsFilter of the input filter chain on the device (include/lsgpu_icp.h has
// the contract, lsgpu_octree_filter.h the arithmetic it shares with the host twin).
//
// The recursion becomes a sort: every point walks down from the root box to depth D with the recursion's own float
// operations and writes its octants into a key (k_ogf_keys) -> the library's stable radix sort over 3 D bits: the sorted
// order is the depth-first order of the nodes at EVERY depth -> k_ogf_leaves finds per sorted position the depth at which
// its node stops being split and marks the leaves' heads -> the chain's scan over the heads ranks the leaves ->
// k_ogf_regroup + a second stable sort, by leaf rank from input order, put every leaf's points in ascending input index ->
// k_ogf_sample forms one point per head and writes it at the leaf's rank.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lsgpu_octree_filter.h"

namespace lsgpu {

// path of every point (key), input index (value)
__global__ __launch_bounds__(256) void k_ogf_keys(const float4* __restrict__ p, int n, octreef::Root g,
                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 v = p[i];
  keys[i] = octreef::path_key(g, v.x, v.y, v.z);
  vals[i] = (uint32_t)i;
}

// The node of sorted position i at depth d is the run of keys that share its first 3 d bits (shift = 3 (D - d)).  Does it
// hold at most max_point points?  Such a run lies inside [i - max_point, i + max_point], so the two ends are looked for in
// that window only (binary search: the keys are sorted, "same prefix as keys[i]" is monotone on either side of i); a run
// that leaves the window has more than max_point points in it.
__device__ __forceinline__ bool ogf_few_points(const uint64_t* __restrict__ keys, uint32_t n, uint32_t i, int shift, uint32_t max_point) {
  const uint64_t prefix = keys[i] >> shift;
  uint32_t a = i > max_point ? i - max_point : 0u, b = i;
  while (a < b) {   // the first position of the window with the prefix
    const uint32_t m = a + ((b - a) >> 1);
    if ((keys[m] >> shift) == prefix) b = m; else a = m + 1u;
  }
  const uint32_t first = a;
  if (i - first >= max_point) return false;
  a = i; b = (n - 1u - i > max_point) ? i + max_point : n - 1u;
  while (a < b) {   // the last one
    const uint32_t m = b - ((b - a) >> 1);
    if ((keys[m] >> shift) == prefix) a = m; else b = m - 1u;
  }
  return a - first + 1u <= max_point;
}

// One thread per SORTED position: the depth of its leaf = the smallest d <= D whose node holds at most max_point points,
// else D (the size rule and the depth cap are in D).  A node's count cannot grow with depth: binary search over d.  Every
// point of a leaf finds the same depth (they share all the prefixes that were looked at).  code[i] = 1 + the leaf's key
// shift at the leaf's first point (its predecessor's prefix differs), 0 elsewhere; all n words are written.
__global__ __launch_bounds__(256) void k_ogf_leaves(const uint64_t* __restrict__ keys, int n, int depth, uint32_t max_point,
                                                    uint32_t* __restrict__ code) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = depth;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ogf_few_points(keys, (uint32_t)n, (uint32_t)i, 3 * (depth - mid), max_point)) hi = mid; else lo = mid + 1;
  }
  const int shift = 3 * (depth - lo);   // <= 63
  const bool head = i == 0 || (keys[i - 1] >> shift) != (keys[i] >> shift);
  code[i] = head ? (uint32_t)shift + 1u : 0u;
}

// The path sort leaves a leaf above depth D ordered by its points' deeper octants, not by input index (the stable sort keeps
// input order among EQUAL keys only).  The second, shorter sort puts that right: every point's key becomes the rank of its
// leaf, written at the point's INPUT position (value = that position), and a stable sort of that sequence by leaf rank has
// the leaves in visiting order and every leaf in ascending input index.  A leaf keeps its range of sorted positions -- the
// leaves are in the same order, with the same sizes, in both sorts -- so code[] and rank[] stay valid.
// One thread per position of the path sort; idx is a permutation of [0, n): every word of leaf_of / self is written.
// rank[i]: the exclusive count of leaf heads in front of i.
__global__ __launch_bounds__(256) void k_ogf_regroup(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ code,
                                                     const uint32_t* __restrict__ rank, int n, uint64_t* __restrict__ leaf_of,
                                                     uint32_t* __restrict__ self) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = idx[i];
  leaf_of[j] = (uint64_t)(rank[i] - (code[i] ? 0u : 1u));   // (position 0 is a head: no underflow)
  self[j] = j;
}

// One thread per sorted position (leaf rank, input index), at work where a leaf begins: the leaf's end by binary search
// (FirstPts reads none of it), then octreef::leaf_point over the leaf's points in ascending input index -- one lane, one
// float sum per leaf, however long the leaf (the rule of k_vgf_reduce: a parallel sum would round differently).  The leaf's
// rank is < the number of leaves <= n = the room of `out`; draws: one per leaf, read for RandomPts only.
__global__ __launch_bounds__(256) void k_ogf_sample(const float4* __restrict__ p, const uint64_t* __restrict__ leaf_of,
                                                    const uint32_t* __restrict__ idx, int n, const uint32_t* __restrict__ code,
                                                    int method, const float* __restrict__ draws, float4* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!code[i]) return;
  const uint64_t leaf64 = leaf_of[i];
  const uint32_t leaf = (uint32_t)leaf64;
  uint32_t count = 1;
  if (method != octreef::kFirstPts) {
    uint32_t a = (uint32_t)i, b = (uint32_t)n - 1u;
    while (a < b) {   // the last position of the leaf
      const uint32_t m = b - ((b - a) >> 1);
      if (leaf_of[m] == leaf64) a = m; else b = m - 1u;
    }
    count = a - (uint32_t)i + 1u;
  }
  const float draw = method == octreef::kRandomPts ? draws[leaf] : 0.f;
  const octreef::Pt r = octreef::leaf_point(
      [&](uint32_t j) { const float4 v = p[idx[(uint32_t)i + j]]; return octreef::Pt{v.x, v.y, v.z, v.w}; }, count, method, draw);
  out[leaf] = make_float4(r.x, r.y, r.z, r.w);
}

}  // namespace lsgpu
