// lsgpu_snf.hip.h -- SurfaceNormalDataPointsFilter on the device: every point of the reference keeps its place and gets
// the PCA normal of its own knn nearest neighbours (itself included), DESIGN.md §3 "Surface normals of every point".
//
// Restatement choices (choices 15-17; the contract is in include/lsgpu_icp.h):
//   * Coordinates.  Distances, means and covariances are taken on the cloud centred on its mean exactly as set_reference
//     centres it (k_ref_gather: one float subtraction per coordinate), so the Morton-sorted cloud, the chunks and the
//     cell tables set_reference builds ARE the search structure of the filter, and the reference the loop then matches
//     against: nothing is built twice.
//   * Order of a neighbourhood: ascending d2 = fma(dz,dz, fma(dy,dy, dx*dx)), ties to the smaller ORIGINAL index (the
//     lists below carry the original index, pts[].w, not the sorted one).  The same rule decides between the knn-th and
//     the (knn+1)-th point at the same distance.  The order is the order of the float sums of box_normal.
//   * A neighbourhood that fails box_normal's rank test keeps its point with the normal (0, 1, 0).
//
// Scheme (exact): the queries are the sorted reference itself.
//   * k_snf_tile<K>: one wave = 64 consecutive sorted points.  The wave's own window of 64 sorted points is evaluated
//     first: it fills every lane's list with real points and gives the lane its first bound, the knn-th distance inside
//     the window, for free.  From there on the kernel is k_knnk_tile: box of the lanes' balls, one level of the pyramid,
//     chunk boxes culled 64 at a time, a surviving chunk staged through LDS and broadcast (the window's points are
//     skipped: they are in the lists already).  Lists have a compile-time length K >= knn and live in registers; the
//     pruning bound is the knn-th entry, so the first knn entries are exact whatever K.
//   * Epilogue, same lane: the neighbours' sorted positions go to a private LDS column (no runtime-indexed private
//     array, no scratch), box_normal gathers the knn points from there -- the wave has just streamed them, this is L2
//     traffic -- and the normal is stored.  The neighbour list leaves the kernel only if the caller asked for ids.
//   * Lanes whose ball is wider than r_cap (isolated far-field points), and windows with fewer than knn points, go to
//     k_snf_fallback<K>: one wave per point, as k_knnk_fallback, then the same epilogue on lane 0.
#pragma once
#include "lsgpu_common.hip.h"
#include "lsgpu_box_normal.h"
#include "lsgpu_density.h"
#include "lsgpu_normal_angle.h"
#include "lsgpu_knn_k.hip.h"

namespace lsgpu {

constexpr int kSnfMinKnn = 3, kSnfMaxKnn = 32;
constexpr float kSnfRCap = 1.0f;   // [m] a lane whose ball is wider searches alone (k_snf_fallback)

struct SnfArgs {
  int n, knn;
  GridDev g;
  const float4* pts;          // Morton-sorted centred reference, w = original index
  const uint32_t* inv;        // original index -> sorted position
  const ChunkDesc* chunks;
  float4* nrm;                // out: normal of sorted point j
  int* ids;                   // out, nullable: knn original indices per point, point major, in ORIGINAL point order
  float* d2;                  // out, nullable (with ids): their squared distances
  uint2* strag;               // points handed to k_snf_fallback {sorted position, bound bits} ...
  uint32_t* strag_count;      // ... and their number
  float r_cap;
  float* dens;                // out (the DENS instantiations only): density of the point, at its ORIGINAL index
};

// the knn-th entry of a list of compile-time length, picked with masks: a runtime index -- and a chain of selects, which
// the compiler folds back into one -- would put the list in scratch
template <int K>
__device__ __forceinline__ float snf_kth(const float (&D)[K], int knn) {
  uint32_t v = 0u;
#pragma unroll
  for (int s = 0; s < K; ++s) v |= __float_as_uint(D[s]) & (uint32_t)-(int)(s == knn - 1);
  return __uint_as_float(v);
}

// the finished list of sorted point j -> optional ids / d2, normal.  col = this lane's LDS column (stride 64).
// DENS (keepDensities 1): the density of the same neighbourhood (lsgpu_density.h), read from the same column, stored at the
// point's original index as the ids are.
template <int K, bool DENS = false>
__device__ __forceinline__ void snf_finish(const SnfArgs& a, int j, uint32_t orig, const float (&D)[K],
                                           const int (&I)[K], int* col) {
#pragma unroll
  for (int s = 0; s < K; ++s)
    if (s < a.knn) {
      // (n >= knn, so the first knn entries are points; an empty entry would index past the cloud: the point itself)
      col[s * 64] = I[s] == kKnnNoIndex ? j : (int)a.inv[I[s]];
      if (a.ids) {
        a.ids[(size_t)orig * (size_t)a.knn + s] = I[s];
        a.d2[(size_t)orig * (size_t)a.knn + s] = D[s];
      }
    }
  const float* xyz = reinterpret_cast<const float*>(a.pts);
  float nv[3];
  const bool ok = boxnormal::box_normal(a.knn, [&](int i, int d) { return xyz[4 * (size_t)col[i * 64] + d]; }, nv);
  a.nrm[j] = ok ? make_float4(nv[0], nv[1], nv[2], 0.f) : make_float4(0.f, 1.f, 0.f, 0.f);
  if (DENS) a.dens[orig] = density::of_neighbourhood(a.knn, [&](int i, int d) { return xyz[4 * (size_t)col[i * 64] + d]; });
}

// amdgpu_waves_per_eu on both kernels: with the default occupancy target the compiler keeps rank3's 3 x 3 work matrix
// (rows and columns swapped by runtime index) in 48 B of scratch per lane; with it the matrix is promoted to LDS.  That is
// a compiler heuristic: devtools/check_snf_resources.sh recompiles the kernels and fails if any of them uses scratch.
// ---------------------------------------------------------------- tile search + normal, 64 points per wave
template <int K, bool DENS = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, K > 16 ? 2 : 4))) void k_snf_tile(SnfArgs a) {
  __shared__ float4 stage[kChunkMax];
  __shared__ int nb[K * 64];
  const int lane = (int)threadIdx.x;
  const int j = blockIdx.x * 64 + lane;
  const bool valid = j < a.n;
  const GridDev& g = a.g;
  // the wave's window: its own 64 sorted points (the last wave's reaches back)
  const int w0 = max(0, min((int)blockIdx.x * 64, a.n - 64));
  const int wc = min(64, a.n - w0);
  const float4 self = a.pts[valid ? j : w0];
  const float qx = self.x, qy = self.y, qz = self.z;
  if (lane < wc) stage[lane] = a.pts[w0 + lane];
  __syncthreads();
  float D[K]; int I[K];
  kbest_init<K>(D, I, INFINITY);
  for (int t = 0; t < wc; ++t) {
    const float4 p = stage[t];
    kbest_insert<K>(D, I, dist2(qx - p.x, qy - p.y, qz - p.z), (int)__float_as_uint(p.w));
  }
  const float ub = snf_kth<K>(D, a.knn);
  const float R = sqrtf(ub) * (1.0f + 1e-5f) + 1e-7f + kFineSlack * g.hf;
  const bool wide = valid && !(R <= a.r_cap);   // (an infinite bound -- a window of fewer than knn points -- included)
  if (wide) a.strag[atomicAdd(a.strag_count, 1u)] = make_uint2((uint32_t)j, __float_as_uint(ub));
  const bool search = valid && !wide;
  if (__ballot(search) == 0ull) return;
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
        // per lane against its current knn-th distance (boxes at exactly that distance stay in: a point there may carry
        // a smaller index)
        const float bd = box_dist2(rl_f(b0.x, k), rl_f(b0.y, k), rl_f(b0.z, k), rl_f(b1.x, k), rl_f(b1.y, k),
                                   rl_f(b1.z, k), qx, qy, qz);
        const bool need = search && bd * kPruneShrink <= snf_kth<K>(D, a.knn);
        if (__ballot(need) == 0ull) continue;
        const uint32_t st = rl_u(__float_as_uint(b0.w), k), cnt = rl_u(__float_as_uint(b1.w), k);
        __syncthreads();   // (the previous chunk's points have been read)
        if ((uint32_t)lane < cnt) stage[lane] = a.pts[st + lane];
        __syncthreads();
        if (need) {
          for (uint32_t t = 0; t < cnt; ++t) {
            if (st + t - (uint32_t)w0 < (uint32_t)wc) continue;   // a point of the window: in the list already
            const float4 p = stage[t];
            kbest_insert<K>(D, I, dist2(qx - p.x, qy - p.y, qz - p.z), (int)__float_as_uint(p.w));
          }
        }
      }
    }
  }
  if (search) snf_finish<K, DENS>(a, j, __float_as_uint(self.w), D, I, nb + lane);
}

// ---------------------------------------------------------------- exact fallback, one wave per point
template <int K, bool DENS = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, K > 16 ? 2 : 4))) void k_snf_fallback(SnfArgs a) {
  __shared__ int nb[K * 64];
  const int lane = (int)threadIdx.x;
  const uint32_t count = *a.strag_count;
  const GridDev& g = a.g;
  const int lim = (1 << (g.bits + g.fine)) - 1;
  for (uint32_t s = blockIdx.x; s < count; s += gridDim.x) {
    const uint2 sg = a.strag[s];
    const int j = (int)sg.x;
    const float4 q = a.pts[j];
    const float ub = __uint_as_float(sg.y);
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
            kbest_insert<K>(D, I, dist2(q.x - p.x, q.y - p.y, q.z - p.z), (int)__float_as_uint(p.w));
          }
          // a lane whose list holds knn points bounds the knn-th distance of the point (a list still holding sentinels
          // shows the bound it started from)
          bound = fminf(bound, wave_min(snf_kth<K>(D, a.knn)));
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
    if (lane == 0) snf_finish<K, DENS>(a, j, __float_as_uint(q.w), RD, RI, nb);
  }
}

// normals of the sorted reference -> 3 floats per point in the order the cloud was given
__global__ __launch_bounds__(256) void k_snf_unpermute(const float4* __restrict__ pts, int n,
                                                       const float4* __restrict__ nrm, float* __restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const size_t o = (size_t)__float_as_uint(pts[j].w);
  const float4 v = nrm[j];
  out[3 * o + 0] = v.x; out[3 * o + 1] = v.y; out[3 * o + 2] = v.z;
}

// OrientNormalsDataPointsFilter behind ObservationDirectionDataPointsFilter (lsgpu_normal_angle.h, flips): one thread per
// point, the normal negated where the rule says so.  Two layouts: normals of a cloud in its own order (nrm3, 3 floats per
// point, beside pos) -- the filtered reference before set_reference, the reading -- or the Morton-sorted float4 normals of
// the handle's reference (nrm4; sorted[j].w = the point's index in the cloud as given, whose staged copy `pos` supplies the
// uncentred position: the very bits the caller gave, no reconstruction from the centred point).
__global__ __launch_bounds__(256) void k_orient_normals(const float4* __restrict__ pos, const float4* __restrict__ sorted, int n,
                                                        float sx, float sy, float sz, int mode, float* __restrict__ nrm3,
                                                        float4* __restrict__ nrm4) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  if (sorted) {
    const float4 p = pos[(size_t)__float_as_uint(sorted[j].w)];
    float4 v = nrm4[j];
    if (normal_angle::flips(p.x, p.y, p.z, sx, sy, sz, v.x, v.y, v.z, mode)) { v.x = -v.x; v.y = -v.y; v.z = -v.z; nrm4[j] = v; }
  } else {
    const float4 p = pos[j];
    const float x = nrm3[3 * (size_t)j], y = nrm3[3 * (size_t)j + 1], z = nrm3[3 * (size_t)j + 2];
    if (normal_angle::flips(p.x, p.y, p.z, sx, sy, sz, x, y, z, mode)) { nrm3[3 * (size_t)j] = -x; nrm3[3 * (size_t)j + 1] = -y; nrm3[3 * (size_t)j + 2] = -z; }
  }
}

// lsgpu_cloud_ingest's last step: the kept cloud and its normals into a cloud slot, one thread per point of the cloud AS
// STAGED (thread i = point i, so the 16-byte point load, the 16-byte point store and the 12-byte normal store of a wave are
// contiguous; the one gather is the normal, through inv as k_md_pass reads it).  It stands for k_snf_unpermute,
// k_orient_normals (its nrm3 layout) and the two copies into the slot: the point's bits are the staged ones, the normal's
// are nrm[inv[i]]'s, negated where normal_angle::flips says so (mode 0: never) -- the very values those kernels leave.
// No LDS, no atomics; out_pts / out_nrm are the slot's own buffers and never alias the inputs.
__global__ __launch_bounds__(256) void k_ingest_store(const float4* __restrict__ staged, int n, const uint32_t* __restrict__ inv,
                                                      const float4* __restrict__ nrm, float sx, float sy, float sz, int mode,
                                                      float4* __restrict__ out_pts, float* __restrict__ out_nrm) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = staged[i];
  float4 v = nrm[inv[i]];
  if (normal_angle::flips(p.x, p.y, p.z, sx, sy, sz, v.x, v.y, v.z, mode)) { v.x = -v.x; v.y = -v.y; v.z = -v.z; }
  out_pts[i] = p;
  out_nrm[3 * (size_t)i + 0] = v.x; out_nrm[3 * (size_t)i + 1] = v.y; out_nrm[3 * (size_t)i + 2] = v.z;
}

}  // namespace lsgpu
