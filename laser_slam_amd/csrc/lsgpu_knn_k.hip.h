// lsgpu_knn_k.hip.h -- exact k-nearest correspondence search: KDTreeMatcher::findClosests with knn = k (2..8 in the ICP
// loop, 1..8 on the chain plan and through lsgpu_knn_k), epsilon 0.  Matches then holds k x N dists / ids (one column per reading point) and
// every pair goes on to the outlier filter and the error minimizer ("k nearest matches").
//
// Restatement choices (choice 13):
//   * Order within a column.  libnabo does not sort under the flags KDTreeMatcher passes; the order only changes the
//     order in which the double sums are added.  This library returns the k matches in ascending d2, ties going to the
//     smaller index of the Morton-sorted reference -- the k = 1 rule of lsgpu_knn.hip.h, extended.  The same rule decides
//     which point is kept when the k-th and the (k+1)-th candidates are at exactly the same distance.
//   * Distances are computed as everywhere else: fma(dz,dz, fma(dy,dy, dx*dx)) of the moved query minus the point
//     (choice 5).
//   * A reference with fewer than k points is refused (LSGPU_BAD_ARG); epsilon > 0 (libnabo's approximate search) is
//     refused: an exact search meets libnabo's guarantee but would not reproduce its results.
//
// Scheme (exact, no approximation):
//   * every query carries an upper bound on its k-th distance: the largest distance, under the new T, to the k distinct
//     points it matched in the previous iteration (warm start), or to k points of the first cell around it that holds
//     at least k points (k_knnk_seed, first search of an alignment / the kernel-level API).
//   * k_knnk_tile: one wave = 64 Morton-neighbouring queries.  Each lane keeps its k best {d2, index} in registers, a list
//     of compile-time length K kept sorted by unrolled compare-and-swap steps (no runtime-indexed private array: it
//     would live in scratch).  The wave takes the bounding box of its lanes' balls, picks the pyramid level at which
//     that box spans <= 4x4x4 cells (one hash lookup per lane), culls the cells' chunk boxes 64 at a time against that
//     box, and tests a surviving chunk per lane against the lane's CURRENT k-th distance; a chunk some lane needs is
//     staged through LDS and broadcast to all lanes.
//   * lanes whose ball is wider than r_cap go to k_knnk_fallback: one wave per query, chunks culled lane-parallel against
//     the single ball, nearest box first, the surviving chunks evaluated one point per lane into per-lane lists that
//     are merged at the end (k rounds of a wave minimum).
//   * MAXD instantiations (KDTreeMatcher maxDist, DESIGN.md §5 choice 14): every bound above -- the seed's, the warm
//     start's, the fallback's -- is cut to maxDist^2 before anything is searched, so no launch looks further than maxDist
//     from its first one on.  An empty list entry IS the bound (the sentinel ranks behind a real point at exactly that
//     distance: d2 == maxDist^2 is valid), entries left empty are stored invalid (index -1, d2 +inf) behind the valid
//     ones, and a query with an invalid entry searches the whole maxDist ball again in the next iteration.
// Output: pair p = j * K + s (j = sorted query, s = rank) -> kmatch[p] = {x, y, z, sorted index bits} of the matched
// reference point, kd2[p] = its squared distance.  kmatch is also the next search's warm start.
#pragma once
#include "lsgpu_common.hip.h"
#include "lsgpu_knn.hip.h"

namespace lsgpu {

constexpr int kKnnKMax = LSGPU_MATCHER_KNN_MAX;
constexpr float kKnnKRCap = 1.0f;          // [m] a lane whose ball is wider searches alone (k_knnk_fallback), as r_cap of k = 1
constexpr int kKnnNoIndex = 0x7FFFFFFF;   // sentinel of an empty list entry: ranks behind every real point at the same d2

struct KnnKArgs {
  const float4* rdq;        // sorted reading (already moved by T_refMean_dataIn), w = caller index
  int nq;
  Mat34 T;                  // applied on load; from the loop state if st is set
  const IcpState* st;       // loop state (nullable): T, and `done` turns the launch into an exit
  GridDev g;
  const float4* pts;        // Morton-sorted centred reference
  const ChunkDesc* chunks;
  float4* kmatch;           // in: warm start, out: the k matches of every query (see the header comment)
  float* kd2;               // out: their squared distances
  uint32_t* strag;          // queries handed to k_knnk_fallback ...
  uint32_t* strag_count;    // ... and their number (re-armed by the normal-equation kernel of the loop)
  float r_cap;              // lanes with a wider ball go to the fallback
  float max_d2;             // MAXD instantiations: KDTreeMatcher maxDist squared -- a match is valid iff d2 <= max_d2
};

// (d, i) before (e, j) in the order of a column: ascending distance, then the smaller sorted index
__device__ __forceinline__ bool kbest_before(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

// one candidate into a sorted list of compile-time length K: replace the last entry, bubble it to its place
template <int K>
__device__ __forceinline__ void kbest_insert(float (&D)[K], int (&I)[K], float d, int i) {
  if (!kbest_before(d, i, D[K - 1], I[K - 1])) return;
  D[K - 1] = d; I[K - 1] = i;
#pragma unroll
  for (int s = K - 1; s > 0; --s) {
    const bool sw = kbest_before(D[s], I[s], D[s - 1], I[s - 1]);
    const float td = D[s - 1]; const int ti = I[s - 1];
    D[s - 1] = sw ? D[s] : td; I[s - 1] = sw ? I[s] : ti;
    D[s] = sw ? td : D[s]; I[s] = sw ? ti : I[s];
  }
}

template <int K>
__device__ __forceinline__ void kbest_init(float (&D)[K], int (&I)[K], float ub) {
#pragma unroll
  for (int s = 0; s < K; ++s) { D[s] = ub; I[s] = kKnnNoIndex; }
}

// upper bound on the k-th distance: the largest distance to the k distinct points of the warm start
template <int K>
__device__ __forceinline__ float kbest_warm_bound(const KnnKArgs& a, int j, float qx, float qy, float qz) {
  float ub = 0.f;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const float4 m = a.kmatch[(size_t)j * K + s];
    ub = fmaxf(ub, __float_as_int(m.w) >= 0 ? dist2(qx - m.x, qy - m.y, qz - m.z) : INFINITY);
  }
  return ub;
}

template <int K>
__device__ __forceinline__ void kbest_store(const KnnKArgs& a, int j, const float (&D)[K], const int (&I)[K]) {
#pragma unroll
  for (int s = 0; s < K; ++s) {
    const bool ok = I[s] != kKnnNoIndex;
    const float4 p = ok ? a.pts[I[s]] : make_float4(0.f, 0.f, 0.f, 0.f);
    a.kmatch[(size_t)j * K + s] = make_float4(p.x, p.y, p.z, __int_as_float(ok ? I[s] : -1));
    a.kd2[(size_t)j * K + s] = ok ? D[s] : INFINITY;
  }
}

// ---------------------------------------------------------------- seed
// k points near the query: climb the pyramid from level 0 until the cell holding the query (clamped into the grid) has
// at least K points, keep the K best of its first 256.  (The top level is one cell with every point, and the handle
// refuses a reference with fewer than K points.)
template <int K, bool MAXD = false>
__global__ __launch_bounds__(256) void k_knnk_seed(KnnKArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nq) return;
  Mat34 T; float cap2;
  if (!iter_params(a.st, a.T, INFINITY, 0, T, cap2)) return;
  const float4 r = a.rdq[j];
  const float3 q = xform(T, r.x, r.y, r.z);
  const GridDev& g = a.g;
  const int lim = (1 << (g.bits + g.fine)) - 1;
  const int fx = fine_coord(q.x, g.ox, g.inv_hf, lim);
  const int fy = fine_coord(q.y, g.oy, g.inv_hf, lim);
  const int fz = fine_coord(q.z, g.oz, g.inv_hf, lim);
  float D[K]; int I[K];
  kbest_init<K>(D, I, MAXD ? a.max_d2 : INFINITY);
  for (int l = 0; l <= g.bits; ++l) {
    const int sh = g.fine + l;
    uint32_t cs, ce;
    if (!grid_lookup(g, l, (uint32_t)(fx >> sh), (uint32_t)(fy >> sh), (uint32_t)(fz >> sh), cs, ce)) continue;
    const uint32_t p0 = a.chunks[cs].start;
    const ChunkDesc dl = a.chunks[ce - 1];
    uint32_t p1 = dl.start + dl.count;
    if (p1 - p0 < (uint32_t)K && l < g.bits) continue;
    if (p1 - p0 > 256u) p1 = p0 + 256u;
    for (uint32_t t = p0; t < p1; ++t) {
      const float4 c = a.pts[t];
      kbest_insert<K>(D, I, dist2(q.x - c.x, q.y - c.y, q.z - c.z), (int)t);
    }
    break;
  }
  kbest_store<K>(a, j, D, I);
}

// ---------------------------------------------------------------- tile search, 64 queries per wave
template <int K, bool MAXD = false>
__global__ __launch_bounds__(64) void k_knnk_tile(KnnKArgs a) {
  __shared__ float4 stage[kChunkMax];
  Mat34 T; float cap2;
  if (!iter_params(a.st, a.T, INFINITY, 0, T, cap2)) return;
  const int lane = (int)threadIdx.x;
  const int j = blockIdx.x * 64 + lane;
  const bool valid = j < a.nq;
  const GridDev& g = a.g;
  float qx = 0.f, qy = 0.f, qz = 0.f, ub = INFINITY;
  if (valid) {
    const float4 r = a.rdq[j];
    const float3 q = xform(T, r.x, r.y, r.z);
    qx = q.x; qy = q.y; qz = q.z;
    ub = kbest_warm_bound<K>(a, j, qx, qy, qz);
    if (MAXD) ub = fminf(ub, a.max_d2);
  }
  const float R = sqrtf(ub) * (1.0f + 1e-5f) + 1e-7f + kFineSlack * g.hf;
  const bool wide = valid && !(R <= a.r_cap);   // (an infinite bound included)
  if (wide) a.strag[atomicAdd(a.strag_count, 1u)] = (uint32_t)j;
  const bool search = valid && !wide;
  if (__ballot(search) == 0ull) return;
  float D[K]; int I[K];
  kbest_init<K>(D, I, ub);
  // the box of the searching lanes' balls, and the level at which it spans at most four cells per axis
  const float lox = wave_min(search ? qx - R : INFINITY), hix = wave_max(search ? qx + R : -INFINITY);
  const float loy = wave_min(search ? qy - R : INFINITY), hiy = wave_max(search ? qy + R : -INFINITY);
  const float loz = wave_min(search ? qz - R : INFINITY), hiz = wave_max(search ? qz + R : -INFINITY);
  const int lim = (1 << (g.bits + g.fine)) - 1;
  const int flx = fine_coord(lox, g.ox, g.inv_hf, lim), fhx = fine_coord(hix, g.ox, g.inv_hf, lim);
  const int fly = fine_coord(loy, g.oy, g.inv_hf, lim), fhy = fine_coord(hiy, g.oy, g.inv_hf, lim);
  const int flz = fine_coord(loz, g.oz, g.inv_hf, lim), fhz = fine_coord(hiz, g.oz, g.inv_hf, lim);
  int l = 0, sh = g.fine;
  for (; l < g.bits; ++l, ++sh)
    if ((fhx >> sh) - (flx >> sh) < 4 && (fhy >> sh) - (fly >> sh) < 4 && (fhz >> sh) - (flz >> sh) < 4) break;
  sh = g.fine + l;
  const int x0 = flx >> sh, y0 = fly >> sh, z0 = flz >> sh;
  const int nx = (fhx >> sh) - x0 + 1, ny = (fhy >> sh) - y0 + 1, nz = (fhz >> sh) - z0 + 1;
  uint32_t cs = 0, ce = 0;
  {
    const int cx = lane & 3, cy = (lane >> 2) & 3, cz = lane >> 4;
    if (cx < nx && cy < ny && cz < nz &&
        !grid_lookup(g, l, (uint32_t)(x0 + cx), (uint32_t)(y0 + cy), (uint32_t)(z0 + cz), cs, ce)) {
      cs = 0; ce = 0;
    }
  }
  unsigned long long cells = __ballot(ce > cs);
  while (cells) {
    const int c = __ffsll((long long)cells) - 1;
    cells &= cells - 1;
    const uint32_t ccs = rl_u(cs, c), cce = rl_u(ce, c);
    for (uint32_t base = ccs; base < cce; base += 64) {
      const uint32_t ch = base + (uint32_t)lane;
      float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
      bool keep = false;
      if (ch < cce) {   // lane-parallel cull against the wave's box
        const float4* cd = reinterpret_cast<const float4*>(a.chunks + ch);
        b0 = cd[0]; b1 = cd[1];
        keep = b0.x <= hix && b1.x >= lox && b0.y <= hiy && b1.y >= loy && b0.z <= hiz && b1.z >= loz;
      }
      unsigned long long m = __ballot(keep);
      while (m) {
        const int k = __ffsll((long long)m) - 1;
        m &= m - 1;
        // per lane against its current k-th distance (boxes at exactly that distance stay in: a point there may carry a
        // smaller index)
        const float bd = box_dist2(rl_f(b0.x, k), rl_f(b0.y, k), rl_f(b0.z, k), rl_f(b1.x, k), rl_f(b1.y, k),
                                   rl_f(b1.z, k), qx, qy, qz);
        const bool need = search && bd * kPruneShrink <= D[K - 1];
        if (__ballot(need) == 0ull) continue;
        const uint32_t st = rl_u(__float_as_uint(b0.w), k), cnt = rl_u(__float_as_uint(b1.w), k);
        __syncthreads();   // (the previous chunk's points have been read)
        if ((uint32_t)lane < cnt) stage[lane] = a.pts[st + lane];
        __syncthreads();
        if (need) {
          for (uint32_t t = 0; t < cnt; ++t) {
            const float4 p = stage[t];
            kbest_insert<K>(D, I, dist2(qx - p.x, qy - p.y, qz - p.z), (int)(st + t));
          }
        }
      }
    }
  }
  if (search) kbest_store<K>(a, j, D, I);
}

// ---------------------------------------------------------------- exact fallback, one wave per query
template <int K, bool MAXD = false>
__global__ __launch_bounds__(256) void k_knnk_fallback(KnnKArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t nw = gridDim.x * 4u;
  Mat34 T; float cap2;
  if (!iter_params(a.st, a.T, INFINITY, 0, T, cap2)) return;
  const uint32_t count = *a.strag_count;
  const GridDev& g = a.g;
  const int lim = (1 << (g.bits + g.fine)) - 1;
  for (uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6); s < count; s += nw) {
    const int j = (int)a.strag[s];
    const float4 r = a.rdq[j];
    const float3 q = xform(T, r.x, r.y, r.z);
    float ub = kbest_warm_bound<K>(a, j, q.x, q.y, q.z);
    if (MAXD) ub = fminf(ub, a.max_d2);
    float D[K]; int I[K];
    kbest_init<K>(D, I, ub);
    float bound = ub;
    const float B = sqrtf(bound) * (1.0f + 1e-5f) + 1e-7f + kFineSlack * g.hf;
    const int flx = fine_coord(q.x - B, g.ox, g.inv_hf, lim), fhx = fine_coord(q.x + B, g.ox, g.inv_hf, lim);
    const int fly = fine_coord(q.y - B, g.oy, g.inv_hf, lim), fhy = fine_coord(q.y + B, g.oy, g.inv_hf, lim);
    const int flz = fine_coord(q.z - B, g.oz, g.inv_hf, lim), fhz = fine_coord(q.z + B, g.oz, g.inv_hf, lim);
    int l = 0, sh = g.fine;
    for (; l < g.bits; ++l, ++sh)
      if ((fhx >> sh) - (flx >> sh) < 4 && (fhy >> sh) - (fly >> sh) < 4 && (fhz >> sh) - (flz >> sh) < 4) break;
    sh = g.fine + l;
    const int x0 = flx >> sh, y0 = fly >> sh, z0 = flz >> sh;
    const int nx = (fhx >> sh) - x0 + 1, ny = (fhy >> sh) - y0 + 1, nz = (fhz >> sh) - z0 + 1;
    uint32_t cs = 0, ce = 0;
    {
      const int cx = lane & 3, cy = (lane >> 2) & 3, cz = lane >> 4;
      if (cx < nx && cy < ny && cz < nz &&
          !grid_lookup(g, l, (uint32_t)(x0 + cx), (uint32_t)(y0 + cy), (uint32_t)(z0 + cz), cs, ce)) {
        cs = 0; ce = 0;
      }
    }
    unsigned long long cells = __ballot(ce > cs);
    while (cells) {
      const int c = __ffsll((long long)cells) - 1;
      cells &= cells - 1;
      const uint32_t ccs = rl_u(cs, c), cce = rl_u(ce, c);
      for (uint32_t base = ccs; base < cce; base += 64) {
        const uint32_t ch = base + (uint32_t)lane;
        float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
        float bd = INFINITY;
        bool live = ch < cce;
        if (live) {
          const float4* cd = reinterpret_cast<const float4*>(a.chunks + ch);
          b0 = cd[0]; b1 = cd[1];
          bd = box_dist2(b0.x, b0.y, b0.z, b1.x, b1.y, b1.z, q.x, q.y, q.z) * kPruneShrink;
        }
        // nearest box first: the bound shrinks as soon as close points turn up
        unsigned long long m = __ballot(live && bd <= bound);
        while (m) {
          const unsigned long long key =
              (live && bd <= bound) ? (((unsigned long long)__float_as_uint(bd) << 32) | (unsigned long long)lane) : ~0ull;
          const int k = __builtin_amdgcn_readfirstlane((int)(wave_min_u64(key) & 63ull));
          const uint32_t st = rl_u(__float_as_uint(b0.w), k), cnt = rl_u(__float_as_uint(b1.w), k);
          if ((uint32_t)lane < cnt) {
            const float4 p = a.pts[st + lane];
            kbest_insert<K>(D, I, dist2(q.x - p.x, q.y - p.y, q.z - p.z), (int)(st + lane));
          }
          // a lane whose list holds K points bounds the k-th distance of the query (a list still holding sentinels
          // shows the warm-start bound)
          bound = fminf(bound, wave_min(D[K - 1]));
          if (lane == k) live = false;
          m = __ballot(live && bd <= bound);
        }
      }
    }
    // merge the 64 lists: K rounds of the wave minimum of the lanes' heads (the lowest lane holding it pops)
    float RD[K]; int RI[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(D[0]) << 32) | (unsigned long long)(uint32_t)I[0];
      const unsigned long long mk = wave_min_u64(key);
      RD[t] = __uint_as_float((uint32_t)(mk >> 32)); RI[t] = (int)(uint32_t)(mk & 0xFFFFFFFFull);
      const unsigned long long who = __ballot(key == mk);
      if (lane == __ffsll((long long)who) - 1) {
#pragma unroll
        for (int u = 0; u < K - 1; ++u) { D[u] = D[u + 1]; I[u] = I[u + 1]; }
        D[K - 1] = INFINITY; I[K - 1] = kKnnNoIndex;
      }
    }
    if (lane == 0) kbest_store<K>(a, j, RD, RI);
  }
}

// pairs (sorted-query order, sorted-reference ids) -> caller order, original reference ids (k x N column major)
__global__ __launch_bounds__(256) void k_knnk_unpermute(const float4* __restrict__ rdq, int npairs, int k,
                                                        const float4* __restrict__ kmatch,
                                                        const float* __restrict__ kd2,
                                                        const float4* __restrict__ pts,
                                                        int* __restrict__ ids_out, float* __restrict__ d2_out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= npairs) return;
  const int j = p / k, s = p - j * k;
  const size_t o = (size_t)__float_as_uint(rdq[j].w) * (size_t)k + (size_t)s;
  const int id = __float_as_int(kmatch[p].w);
  ids_out[o] = id < 0 ? -1 : (int)__float_as_uint(pts[id].w);
  d2_out[o] = kd2[p];
}

}  // namespace lsgpu
