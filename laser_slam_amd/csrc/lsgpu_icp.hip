// lsgpu_icp.hip -- C-ABI shim (include/lsgpu_icp.h) over the gfx950 kernels.
//
// Host-side control flow restates PointMatcher::ICP::compute as called from
// laser_slam/src/laser_track.cpp:496 and laser_slam/src/incremental_estimator.cpp:108:
//   set_reference : steps 2-3 (centre on mean, matcher init)
//   align         : steps 5-7 (move reading by T_refMean_dataIn, iterate, compose)
// Kernels: lsgpu_grid.hip.h, lsgpu_knn.hip.h, lsgpu_solve.hip.h.  No CPU fallback exists: every failure is returned to the caller.
#include <atomic>
#include <cstring>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <chrono>
#include <system_error>
#include <thread>
#include <type_traits>
#include <utility>

#include <dlfcn.h>

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is opened lazily (dlopen) by lsgpu_icp_comm_init

#include "../../include/lsgpu_icp.h"
#include "lsgpu_grid.hip.h"
#include "lsgpu_tuning.h"
#include "lsgpu_policy.h"
#include "lsgpu_section_plan.h"
#include "lsgpu_modules.h"
#include "lsgpu_submap.hip.h"
#include "lsgpu_knn.hip.h"
#include "lsgpu_knn_k.hip.h"
#include "lsgpu_snf.hip.h"
#include "lsgpu_max_density.hip.h"
#include "lsgpu_shadow.hip.h"
#include "lsgpu_cov_sampling.hip.h"
#include "lsgpu_cone.hip.h"
#include "lsgpu_solve.hip.h"
#include "lsgpu_cov.hip.h"
#include "lsgpu_cov.h"
#include "lsgpu_host_math.h"
#include "lsgpu_ssn.hip.h"
#include "lsgpu_voxel_filter.hip.h"
#include "lsgpu_octree_filter.hip.h"
#include "lsgpu_ssn_tree.hip.h"
#include "lsgpu_ssn_select.hip.h"
#include "lsgpu_sort.hip.h"
#include "lsgpu_scan.hip.h"
#include "lsgpu_rand.h"

using namespace lsgpu;

#define HIPC(expr)                                                                      \
  do {                                                                                  \
    hipError_t e__ = (expr);                                                            \
    if (e__ != hipSuccess) {                                                            \
      char buf__[256];                                                                  \
      snprintf(buf__, sizeof buf__, "%s:%d %s -> %s", __FILE__, __LINE__, #expr,        \
               hipGetErrorString(e__));                                                 \
      h->err = buf__;                                                                   \
      (void)hipGetLastError();                                                          \
      return LSGPU_HIP_ERROR;                                                           \
    }                                                                                   \
  } while (0)

namespace {

// RCCL entry points, resolved at run time so that liblsgpu_icp.so itself has no RCCL dependency.
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;  // optional
  ncclResult_t (*GroupStart)() = nullptr;           // optional (fused exchange of the committed select)
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi* rccl_api() {
  static RcclApi api;
  static bool tried = false;
  if (!tried) {
    tried = true;
    for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
    }
    if (api.lib) {
      api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.lib, "ncclGetUniqueId"));
      api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.lib, "ncclCommInitRank"));
      api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(api.lib, "ncclAllReduce"));
      api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.lib, "ncclCommDestroy"));
      api.CommAbort = reinterpret_cast<decltype(api.CommAbort)>(dlsym(api.lib, "ncclCommAbort"));
      api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.lib, "ncclGetErrorString"));
      api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(api.lib, "ncclGroupStart"));
      api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(api.lib, "ncclGroupEnd"));
      if (!api.GroupStart || !api.GroupEnd) { api.GroupStart = nullptr; api.GroupEnd = nullptr; }
      if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) api.lib = nullptr;
    }
  }
  return api.lib ? &api : nullptr;
}

// The four owners of what a handle takes from the runtime: device memory, pinned host memory, events, streams.  Each
// frees what it holds when it goes, none can be copied, and g_live counts what they hold between them
// (lsgpu_dev_live_resources: a create / destroy cycle must give back everything it took).
std::atomic<long> g_live{0};
inline hipError_t counted(hipError_t made) { if (made == hipSuccess) ++g_live; return made; }

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const size_t want = n + n / 8 + 256;
    hipError_t e = counted(hipMalloc((void**)&p, want * sizeof(T)));
    if (e == hipSuccess) cap = want; else p = nullptr;
    return e;
  }
  void release() { if (p) { (void)hipFree(p); --g_live; } p = nullptr; cap = 0; }
};

// pinned (host-coherent, device-mapped) host memory: reserve() grows by freeing and allocating anew -- the contents go
template <class T>
struct PinBuf {
  T* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = counted(hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault));
    if (e == hipSuccess) cap = n; else p = nullptr;
    return e;
  }
  void release() { if (p) { (void)hipHostFree(p); --g_live; } p = nullptr; cap = 0; }
  T* operator->() const { return p; }
};

// created on first use: ensure(hipEventDefault) for an event that times, ensure(hipEventDisableTiming) for one that orders
struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }   // (the pools are vectors; no copy, no assignment)
  ~Event() { if (ev) { (void)hipEventDestroy(ev); --g_live; } }
  hipError_t ensure(unsigned flags) { return ev ? hipSuccess : counted(hipEventCreateWithFlags(&ev, flags)); }
  operator hipEvent_t() const { return ev; }
};

// non-blocking, created on first use, waited for before it goes
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); --g_live; } }
  hipError_t ensure() { return s ? hipSuccess : counted(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  operator hipStream_t() const { return s; }
};

static_assert(!std::is_copy_constructible<DevBuf<float>>::value && !std::is_copy_constructible<PinBuf<float>>::value &&
              !std::is_copy_constructible<Event>::value && !std::is_copy_constructible<Stream>::value,
              "an owner that could be copied would free twice");

bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// A few words for the host, in ONE launch: the kernel stores into the pinned (host-coherent, device-mapped) staging words
// themselves.  (Each hipMemcpyAsync of four bytes is a 4 - 5 us slot of its own on the stream: four of them behind the
// reference filter, three behind the cell counts -- on chains of 0.8 and 0.25 ms.)
struct ToHost { const uint32_t* src[6]; uint32_t* dst[6]; uint32_t n[6]; };
__global__ __launch_bounds__(64) void k_to_host(ToHost c) {
#pragma unroll
  for (int e = 0; e < 6; ++e)
    for (uint32_t i = threadIdx.x; i < c.n[e]; i += 64u) c.dst[e][i] = c.src[e][i];
}
static void to_host_add(ToHost* c, int* used, const void* src, void* dst, size_t bytes) {
  c->src[*used] = static_cast<const uint32_t*>(src); c->dst[*used] = static_cast<uint32_t*>(dst); c->n[*used] = (uint32_t)(bytes / 4);
  ++*used;
}

// (Uploading a PINNED cloud with a copy kernel over its device mapping instead of hipMemcpyAsync was measured slower:
// 5.93 vs 5.48 ms per 1 M-point compute from host buffers; what had made the pinned path the slower one was two copies
// sharing the link -- lsgpu_icp_compute now queues the reading's copy behind the reference's.)

Mat34 to_mat34(const float* Tcm) {  // column-major 4x4 -> rows
  Mat34 m;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) m.m[r * 4 + c] = Tcm[c * 4 + r];
  return m;
}

double wall_ms() {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline int nblk(int64_t n) { return (int)((n + 255) / 256); }

}  // namespace

// The handle's pinned (host-coherent, device-mapped) staging block: the few words and small records that cross between
// host and device outside the clouds.  One member per use and no member shared, so a record that grows moves its
// neighbours instead of running into them.  k_to_host stores 4-byte words into it from the device, hipMemcpyAsync reads
// and writes the rest.  Every use starts a 64-byte line of its own (as the loop state and the bounds did at their old
// offsets): a copy never shares a line with words another use writes, and the copies keep their aligned path.
struct Staging {
  alignas(64) uint32_t cells[kMaxLevels];   // set_reference: occupied cells per level ...
  uint32_t nchunks;                         // ... and the number of chunks
  alignas(64) GeomDev geom;                 // ... and the grid geometry derived on the device
  alignas(64) double ne[32];                // stand-alone normal equations: the 29 sums (ne_out's layout: 29 + limit slot)
  alignas(64) float limit;                  // lsgpu_trim_limit
  alignas(64) SelState sel0;                // run_select: sel[0] = {0, rank} on its way to the device
  alignas(64) long long handshake[2];       // split-scan entry handshake of an align: {shard size, cannot-start flag}
  alignas(64) IcpState state;               // the loop state of the running align, as of the host's last look
  alignas(64) uint32_t totals[2][4];        // scan_totals, [lane.totals_row]: {last input, last scanned} of two scans
  alignas(64) uint32_t bounds[6];           // cloud_bounds: ordered keys of the minimum and the maximum
  alignas(64) double cov[kCovStride];       // PointToPlaneWithCovErrorMinimizer: the 44 sums of k_cov ...
  alignas(64) lsgpu_iter_trace cov_trace;   // ... and the last iteration's trace record (its normal equations give the step)
  alignas(64) uint32_t price[kPriceSlots * kPriceStride];   // run_knn: the price check's counters (price_cnt) behind the priced search
  alignas(64) uint32_t cone_occ;            // build_cone: occupied bins of the direction index, behind the build
  alignas(64) uint32_t gs_err[8];           // ssn_device: the error record of the sort-free levels (gs_err), with the totals
  alignas(64) double cs[kCsStride];         // CovarianceSamplingDataPointsFilter: the columns of one sums pass (k_cs_final)
};

struct lsgpu_icp {
  lsgpu_icp_config cfg;
  int device = 0;
  Stream stream;
  Stream copy_stream;      // lsgpu_icp_compute: the reading's H2D, overlapped with the reference filter
  Event copy_done;
  Event ref_up_done;       // the reference's H2D on `stream`: the reading's copy queues behind it
  std::string err;

  // reference (steps 2-3)
  int64_t nr = 0;
  float mean[3] = {0, 0, 0};
  GridDev grid;
  int ls = 0;  // start level of the main kNN pass
  lsgpu_icp_info info;
  DevBuf<float4> ref_in;   DevBuf<float> nrm_in;
  // Scratch of the sorts and scans.  Two sets: lsgpu_icp_compute orders the queries on a second stream while the
  // reference grid is built on the first.  A lane is what the helpers below enqueue on (stream, set, row of pin->totals):
  // `lane` is the main one except inside a LaneScope.
  struct SortScratch {
    DevBuf<uint64_t> keys, keys_alt;
    DevBuf<uint32_t> vals, vals_alt;
    DevBuf<char> sort_tmp;
    DevBuf<uint32_t> sort_hist;  // radix sort: 256 x blocks digit histograms + 256 digit totals
  };
  SortScratch scr_main, scr_side;
  struct Lane { hipStream_t stream; SortScratch* scratch; int totals_row; } lane{nullptr, &scr_main, 0};
  Lane main_lane() { return Lane{stream, &scr_main, 0}; }
  Lane side_lane() { return Lane{side_stream, &scr_side, 1}; }   // (lsgpu_icp_compute's side work, its align's deferred index build)
  Stream draw_stream;      // H2D of the filters' draws, issued by the helper thread that produces them
  Event draws_done, draws_first_done;
  Stream side_stream;      // lsgpu_icp_compute: reading filter + query order, beside the grid build
  Event side_done;
  DevBuf<float4> pts, nrm;
  DevBuf<uint32_t> ref_inv;
  DevBuf<HashEntry> tables;
  DevBuf<uint32_t> flags, cidx, bounds;
  DevBuf<ChunkDesc> chunks, chunk_groups;
  DevBuf<float> soa;            // chunk-blocked SoA copy of pts (k_soa_fill)
  DevBuf<uint32_t> soa_base, soa_cnt4, soa_first;
  uint32_t nchunks = 0;
  // direction index of the reference (lsgpu_cone.hip.h): the settled launches of an align search it instead of the voxel grid
  DevBuf<float> cone_soa;
  DevBuf<uint32_t> cone_tab, cone_map;
  DevBuf<float4> cone_rowz;
  ConeDev cone;
  bool cone_ok = false;       // built (or being built on the side stream: cone_pending) for the current reference
  bool cone_pending = false;  // the loop's stream has not yet waited for cone_done
  Event cone_done;
  DevBuf<uint32_t> cone_occ;          // occupied (row, column) bins of the index
  Event cone_occ_ready;               // ... are on the host (pin->cone_occ)
  bool cone_decided = false;          // ... looked at (per reference): cone_dense says whether the reference is too dense in direction
  bool cone_dense = false;
  float cone_occupancy = 0.f;         // points per occupied bin
  float cone_zeta_lo = 0.f, cone_zeta_hi = 0.f;
  bool cone_origin_inside = false;
  Event price_ready;                  // the price check's two counters are on the host (pin->price)
  DevBuf<uint32_t> price_cnt;         // kPriceSlots x kPriceStride words (lsgpu_knn.hip.h: ConePrice::count)
  // launch policy of the running align (lsgpu_policy.h): every decision about what is enqueued next lives there
  policy::Config pol_cfg;
  policy::State pol;
  // is the index paying on this handle's clouds?  (policy::index_not_paying; two event pairs per alignment)
  Event ev_pay[4];
  bool pay_voxel_timed = false, pay_index_timed = false;
  int index_rest = 0;         // alignments that still leave the index alone
  int64_t index_rest_nr = 0;  // ... decided on a reference of this size (another size: the judgement starts over)
  float pay_voxel_us = 0.f, pay_index_us = 0.f;   // the two timings behind it (lsgpu_icp_get_policy_info)
  int ssn_sort_fallbacks = 0, ssn_calls = 0;
  DevBuf<uint4> knn_dbg_wave;
  DevBuf<unsigned long long> knn_dbg;  // LSGPU_KNN_STATS builds: 8 counters
  DevBuf<uint2> cell_cache;  // ntiles x 64
  DevBuf<ulonglong2> cell_tags;
  uint32_t cache_gen = 1;
  ncclComm_t comm = nullptr;  // split-scan mode (lsgpu_icp_comm_init)
  int comm_rank = 0, comm_size = 1;
  DevBuf<long long> comm_tmp;
  int dbg_launch_no = 0;     // kNN launches since the last prepare_queries (stats build ablations)
  DevBuf<float> lb;          // per-query lower bound on the NN distance
  DevBuf<IcpState> state;    // loop state of the running align (device)
  DevBuf<float> chk_hist;    // checker history: 8 floats x (max_iterations + 2)
  DevBuf<lsgpu_iter_trace> trace_dev;
  DevBuf<float4> prev;       // warm start of every query: its current match {xyz, sorted index}
  DevBuf<RefStats> stat_partials;
  DevBuf<GeomDev> geom;      // grid geometry derived on the device (k_ref_stats_final)
  DevBuf<uint32_t> counters;  // [0..16] cell counts, [32] straggler count
  DevBuf<uint32_t> ang_cells; // angular occupancy of the reading (query order decision)
  uint32_t n_spread_host = 0;   // length of the spread list as of the last state fetch
  bool n_spread_known = false;
  DevBuf<uint32_t> spread_flag, spread_list, spread_cnt;  // front rows of the tile kernel (tiles whose queries share no candidates)
  DevBuf<uint32_t> sel_aux;   // predicted select: kSelBelowSlots counters + failure flag
  DevBuf<uint32_t> sel_win;   // committed select (split-scan mode): kSelWinRows x 512 window histogram
  DevBuf<uint2> amb_key;      // fused select: the distances of the limit's slice the normal equations set aside ...
  DevBuf<double> amb_val;     // ... and their contributions (kSelAmbCap x 32)

  // device filters (lsgpu_ssn.hip.h)
  DevBuf<SsnSeg> ssn_seg_a, ssn_seg_b;
  DevBuf<int> ssn_axis_a, ssn_axis_b;       // per segment: the axis its current order follows (segmented level sorts)
  DevBuf<uint32_t> ssn_seg_fb;
  DevBuf<SegBlock> ssn_blocktab;
  DevBuf<uint32_t> ssn_seg_of, ssn_box_pts, ssn_box_base, ssn_keep, ssn_out_pos, ssn_bb, ssn_bounds_ws;
  DevBuf<float> ssn_box_normal, ssn_draws;
  // sort-free upper levels of the reference filter (lsgpu_ssn_select.hip.h)
  DevBuf<uint32_t> gs_e[2], gs_k[6];          // two buffer sets: points + their three ordered keys
  DevBuf<GsBlock> gs_tab;                     // block tables of all levels (host-computed: segment sizes are static)
  DevBuf<GsSegBlocks> gs_sblk;
  DevBuf<uint32_t> gs_hist;                   // per segment 2 x 256 counters, two levels (ping-pong)
  DevBuf<GsMedian> gs_cand, gs_median;
  DevBuf<uint32_t> gs_cand_blk, gs_cand_n, gs_cl, gs_err;
  DevBuf<uint2> gs_rng;                       // per segment: the key range of its points on its cut axis (two levels)
  int64_t gs_plan_n = -1;                     // the cloud size / level count the tables on the device were made for
  int gs_plan_levels = -1;
  std::vector<uint32_t> gs_lvl_first, gs_lvl_blocks;
  DevBuf<float4> flt_in, flt_in2, flt_ref, flt_rd;
  DevBuf<float4> vgf_out;   // VoxelGridDataPointsFilter (lsgpu_voxel_filter.hip.h): the voxels' points at their first points' positions
  DevBuf<float> flt_nrm;
  modules::State mods;   // which of the eight optional modules run, and their configs (lsgpu_modules.h; lsgpu_icp_set_*, lsgpu_icp_set_modules)
  // cut modules of the ICP chain's filter sections (lsgpu_icp_set_chain_cuts; lsgpu_chain_cut.hip.h)
  DevBuf<uint32_t> cut_blk;   // the pass's block counts and their scans: 4 rows of ceil(n / 256) words
  DevBuf<float4> cut_ref;     // the reference behind its cut modules
  DevBuf<float> cut_ref_nrm;  // ... and its carried normals, when somebody reads them
  // MaxDensityDataPointsFilter behind SurfaceNormalDataPointsFilter keepDensities 1 (lsgpu_icp_set_max_density; lsgpu_max_density.hip.h)
  DevBuf<float> dens, dens_io;   // the density of every point of the cloud as given; its staging for a host caller
  DevBuf<MdStat> md_stat;        // minimum / maximum of the densities, NaN count
  DevBuf<uint32_t> md_blk;       // the pass's block counts and their scans: 4 rows of ceil(n / 256) words
  // ShadowDataPointsFilter behind the normals of either section (lsgpu_icp_set_shadow; lsgpu_shadow.hip.h)
  DevBuf<uint32_t> sh_blk;           // the pass's block counts and their scan: 2 rows of ceil(n / 256) words
  DevBuf<float4> sh_ref, sh_rd;      // the kept points of the reference (behind the sampling filter or the thinning) / the reading
  DevBuf<float> sh_nrm, sh_rd_nrm;   // the kept reference normals; the reading's normals in front of the pass
  DevBuf<float> sh_nrm_in;           // staging of a host caller's normals (lsgpu_icp_filter_shadow)
  // CovarianceSamplingDataPointsFilter (lsgpu_icp_filter_cov_sampling; lsgpu_cov_sampling.hip.h)
  DevBuf<float4> cs_ref, cs_rd;         // the chosen points of the reference / the reading ...
  DevBuf<float> cs_ref_nrm, cs_rd_nrm;  // ... and their normals
  DevBuf<float> cs_whole_nrm;           // behind SurfaceNormalDataPointsFilter alone: the whole reference's normals in its order
  DevBuf<int32_t> cs_pick;              // the picks of a section (not read behind the gather)
  DevBuf<double> cs_partials, cs_out;   // kCsBlocksMax x kCsStride, kCsStride
  DevBuf<float> cs_mag;                 // the six magnitudes of every point
  DevBuf<covs::Head> cs_heads;          // the first min(nbSample, n) entries of the six sorted lists ...
  PinBuf<covs::Head> cs_heads_pin;      // ... on the host, for the walk
  PinBuf<uint32_t> cs_ids_pin;          // the walk's picks on their way back ...
  DevBuf<uint32_t> cs_ids;              // ... and on the device
  std::vector<uint64_t> cs_chosen;      // the walk's bitmap, one bit per point
  double cs_ms[4] = {0, 0, 0, 0};       // wall time of the last call's phases (lsgpu_icp_cov_sampling_phase_ms)
  DevBuf<float> cs_nrm_in;              // staging of a host caller's normals ...
  DevBuf<float4> cs_pts_out; DevBuf<float> cs_nrm_out; DevBuf<int32_t> cs_ids_out;   // ... and of its results
  // PointToPlaneErrorMinimizer force4DOF / force2D and BoundTransformationChecker (lsgpu_icp_set_motion)
  PinBuf<float> h_chk;               // the bound's copy of the checker history (travels with the loop state's read-back)
  PinBuf<float> draws_pinned;     // host staging of the filter draws (pinned: async H2D)
  std::vector<DevBuf<float4>> clouds;  // lsgpu_cloud_upload slots
  std::vector<int64_t> cloud_n;        // -1: empty
  std::vector<DevBuf<float>> cloud_nrm;   // the normals a slot carries (lsgpu_cloud_upload_normals), 3 floats per point
  std::vector<char> cloud_has_nrm;        // the slot carries normals
  DevBuf<float4> submap;               // assembled reference of lsgpu_icp_compute_clouds
  DevBuf<float> submap_nrm;            // ... and its normals: every member carries some and somebody reads them
  DevBuf<float> car_ref_nrm, car_rd_nrm;   // a compute's carried normals where the caller's cannot be used in place (host memory; the orientation writes)

  // reading
  int64_t nq = 0;
  DevBuf<float4> q_in, rdq;
  DevBuf<int> ids;   DevBuf<float> d2;
  DevBuf<int> ids_io; DevBuf<float> d2_io;
  DevBuf<uint32_t> strag;
  // k-match loop (lsgpu_icp_config.matcher_knn >= 2) and lsgpu_knn_k: k entries per sorted query (lsgpu_knn_k.hip.h)
  DevBuf<float4> kmatch; DevBuf<float> kd2;
  // SurfaceNormalDataPointsFilter (lsgpu_snf.hip.h): the points its tile kernel hands to the wave-per-point pass
  DevBuf<uint2> snf_strag; DevBuf<uint32_t> snf_count;
  DevBuf<uint32_t> hist;      // 3 * kHistBins
  DevBuf<SelState> sel;       // [0] input rank, [1] after pass 2, [2] after pass 3
  DevBuf<uint32_t> hist_med;  // MedianDistOutlierFilter: the second run of the select's refining passes (3 * kHistBins, [0] unused) ...
  DevBuf<SelState> sel_med;   // ... and its three states
  // RobustOutlierFilter (lsgpu_icp_set_robust_filter): the MAD's select over |d2 - median|, the loop's robust state, its trace
  bool have_normals = false;  // the last set_reference was given normals (or a reference filter computed them)
  DevBuf<uint32_t> rb_hist; DevBuf<SelState> rb_sel; DevBuf<RobustState> rb_state; DevBuf<lsgpu_robust_trace> rb_trace_dev;
  size_t rb_trace_n = 0;      // records of the last alignment in rb_trace_dev
  // SurfaceNormalOutlierFilter / reading normals / orientation (lsgpu_icp_set_normals)
  DevBuf<float> rd_nrm;       // the reading's normals, 3 floats per point in the reading's order (lsgpu_icp_compute's step, or the caller's) ...
  DevBuf<float> rd_nrm0;      // ... moved by R_init (step 5): what the loop's angle test reads
  DevBuf<float> nrm_io;       // staging of lsgpu_icp_get_reference_normals
  DevBuf<lsgpu_normal_angle_trace> na_trace_dev;
  size_t na_trace_n = 0;      // records of the last alignment in na_trace_dev
  // PointToPlaneWithCovErrorMinimizer (lsgpu_icp_set_covariance): the pass after the loop and the record it leaves
  int quality_state = 0;      // of the last alignment: 0 none / it did not return LSGPU_OK, 1 `quality` holds it, 2 singular H
  lsgpu_icp_quality quality{};
  DevBuf<float4> cov_pts;     // the moved reading in the caller's order
  DevBuf<double> cov_partials, cov_out;   // kNeBlocksMax x kCovStride, kCovStride
  DevBuf<double> ne_partials; // kNeBlocks * 32
  DevBuf<double> ne_gpartials;  // (kNeBlocksMax / kNeGroup) * 32: first-level sums of k_normal_eq_loop
  DevBuf<uint32_t> ne_tickets;  // 1 + kNeBlocksMax / kNeGroup
  DevBuf<double> ne_out;      // 32 (29 + limit slot)
  DevBuf<float> limit_dev;
  PinBuf<Staging> pin;        // pinned host staging, one member per use
  Event ev0, ev1;
  Event ev_state;   // lsgpu_icp_align: completion of a loop-state copy (the stream goes on behind it)
  // lsgpu_icp_align may return with ONE more iteration queued on `stream` behind its last look at the loop state (it
  // exits at once: the state says `done`).  Work the next call starts on the handle's OTHER streams is ordered behind
  // it through this event, so that nothing ever depends on what that launch does not touch.
  Event ev_tail;
  bool tail_pending = false;
  struct KnnEv { Event a, b, c, d, e; bool second = false; };  // before kNN, after the main pass, after the wave-per-query pass (recorded only if one was launched: `second`), after the select, after the normal equations
  std::vector<KnnEv> knn_events;   // pool, reused across aligns
  // split-scan mode with profile_kernels: an event pair around every RCCL call of the loop (stats.t_comm_ms)
  std::vector<std::pair<Event, Event>> comm_events;
  size_t comm_events_used = 0;
  bool time_comm = false;
  size_t knn_events_used = 0;
  std::vector<lsgpu_iter_trace> trace;
  size_t trace_on_device = 0;   // records of the last alignment still in trace_dev (fetched by lsgpu_icp_get_trace)
  std::vector<std::pair<float, float>> trace_knn_us;   // their search timings (profiled runs), merged in on the fetch
};

struct LaneScope {   // the one way to leave the main lane: the helpers enqueue on `to` while the scope lives, on the main lane after it
  lsgpu_icp* const h;
  LaneScope(lsgpu_icp* hh, const lsgpu_icp::Lane& to) : h(hh) { h->lane = to; }
  ~LaneScope() { h->lane = h->main_lane(); }
};

// Wait for the handle's stream.  Plain handles block; a handle with a communicator polls with a deadline
// (LSGPU_COMM_TIMEOUT_MS, default 30 s): if a peer rank died inside the loop the collectives never complete, the
// communicator is aborted and the caller gets LSGPU_HIP_ERROR instead of a hang.
static int wait_stream(lsgpu_icp* h) {
  if (!h->comm) { HIPC(hipStreamSynchronize(h->stream)); return LSGPU_OK; }
  const double limit_ms = tuning().comm_timeout_ms;
  const double t0 = wall_ms();
  for (int spin = 0;; ++spin) {
    const hipError_t e = hipStreamQuery(h->stream);
    if (e == hipSuccess) return LSGPU_OK;
    if (e != hipErrorNotReady) { (void)hipGetLastError(); h->err = std::string("stream: ") + hipGetErrorString(e); return LSGPU_HIP_ERROR; }
    (void)hipGetLastError();
    if (wall_ms() - t0 > limit_ms) {
      h->err = "split-scan: a collective did not complete in time (peer rank lost?); communicator aborted";
      RcclApi* api = rccl_api();
      if (api && api->CommAbort) (void)api->CommAbort(h->comm); else if (api) (void)api->CommDestroy(h->comm);
      h->comm = nullptr; h->comm_size = 1; h->comm_rank = 0;
      return LSGPU_HIP_ERROR;
    }
    if (spin > 200) std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

// event pair around a collective (only when the align is profiled)
static void comm_mark(lsgpu_icp* h, bool begin) {
  if (!h->time_comm) return;
  if (begin) {
    if (h->comm_events_used == h->comm_events.size()) {
      std::pair<Event, Event> p;
      if (p.first.ensure(hipEventDefault) != hipSuccess || p.second.ensure(hipEventDefault) != hipSuccess) { (void)hipGetLastError(); h->time_comm = false; return; }
      h->comm_events.push_back(std::move(p));
    }
    (void)hipEventRecord(h->comm_events[h->comm_events_used].first, h->stream);
  } else {
    (void)hipEventRecord(h->comm_events[h->comm_events_used++].second, h->stream);
  }
}

static void order_after_tail(lsgpu_icp* h, hipStream_t s) {
  if (h->tail_pending && s && h->ev_tail && hipStreamWaitEvent(s, h->ev_tail, 0) != hipSuccess) (void)hipGetLastError();
}

// what lsgpu_icp_set_chain_cuts / lsgpu_icp_filter_section refuse in a lsgpu_chain_cuts, the module named; empty: nothing
static std::string chain_cuts_why(const lsgpu_chain_cuts* c) {
  const char* const names[7] = {nullptr, "MaxDistDataPointsFilter", "MinDistDataPointsFilter", "BoundingBoxDataPointsFilter", nullptr, nullptr,
                                "RemoveNaNDataPointsFilter"};
  const char* const all = "MaxDist- / MinDist- / BoundingBox- / RemoveNaNDataPointsFilter";
  for (int s = 0; s < 2; ++s) {
    const int n = s == 0 ? c->n_reading : c->n_reference;
    const std::string sec = s == 0 ? "readingDataPointsFilters: " : "referenceDataPointsFilters: ";
    if (n < 0 || n > LSGPU_CHAIN_CUT_MAX) return sec + "0 to " + std::to_string(LSGPU_CHAIN_CUT_MAX) + " cut modules (" + all + "), not " + std::to_string(n);
    for (int k = 0; k < n; ++k) {
      const lsgpu_point_filter& f = (s == 0 ? c->reading : c->reference)[k];
      const char* name = f.type >= 1 && f.type <= 6 ? names[f.type] : nullptr;
      if (!name) return sec + "module " + std::to_string(k) + " has type " + std::to_string(f.type) + ", which is no cut module (" + all + ": 1, 2, 3, 6)";
      if ((f.type == LSGPU_FILTER_MAX_DIST || f.type == LSGPU_FILTER_MIN_DIST) && (f.dim < -1 || f.dim > 2))
        return sec + name + ": dim must be in [-1, 2]";
    }
  }
  return std::string();   // (reading_sampling_at is clamped to 0 .. n_reading where it is read: without RandomSampling it means nothing)
}

static constexpr int kNeBlocksMax = 2048;
static const int kNeBlocks = tuning().ne_blocks;   // 64 .. kNeBlocksMax (lsgpu_tuning.h)
static constexpr int kStatBlocks = 512;
static constexpr int kHistBlocks = 256;
static constexpr int kFallbackBlocks = 8192;  // x 4 waves: one query per wave for up to 32 k stragglers, round robin beyond

// up to `cap` of the `have` records the last alignment left in `dev` -> out; the number copied
template <class T>
static int fetch_trace(lsgpu_icp* h, const T* dev, size_t have, T* out, int cap) {
  if (!out || cap <= 0 || !have) return 0;
  const int n = std::min<int>(cap, (int)have);
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
      hipMemcpy(out, dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

// ---- the module set of a handle.  Which modules run together is lsgpu_modules.h's business; a step below validates one module's
// values, puts it into the set in the making and asks.  lsgpu_icp_set_* is one step, lsgpu_icp_set_modules all eight: both work on
// a copy of the handle's state and commit it only if every step passed.
struct ModuleSet {
  modules::State s;
  modules::Facts f;
  std::string err;   // of the step that returned LSGPU_BAD_CONFIG
  int say(const std::string& why) { err = why; return LSGPU_BAD_CONFIG; }
  int ask(modules::Asker who) { err = modules::refusal(s, f, who); return err.empty() ? LSGPU_OK : LSGPU_BAD_CONFIG; }

  int robust(const lsgpu_robust_config* cfg) {
    const char* why = nullptr;
    // (whether the reference has normals is known to align / the stand-alone sums, which check point2plane again)
    if (cfg && robust::check(cfg, f.error_minimizer, 1, &why) != LSGPU_OK) return say(why);
    if ((s.robust_on = cfg != nullptr)) s.robust = *cfg;
    return ask(modules::kSetRobust);
  }
  int normals(const lsgpu_normals_config* cfg) {
    if ((s.normals_on = cfg != nullptr)) s.normals = *cfg;
    if (ask(modules::kSetNormalsFirst) != LSGPU_OK) return LSGPU_BAD_CONFIG;   // (a module on the reading that needs its normals)
    const char* why = nullptr;
    // (whether the reference has normals is known to align, for which a filter without them is inert)
    if (cfg && normal_angle::check(cfg, f.error_minimizer, 1, &why) != LSGPU_OK) return say(why);
    return ask(modules::kSetNormals);
  }
  int covariance(const lsgpu_covariance_config* cfg) {
    if (cfg && (!(cfg->sensor_std_dev >= 0.f) || std::isinf(cfg->sensor_std_dev))) return say("PointToPlaneWithCovErrorMinimizer: sensorStdDev must be finite and >= 0");
    if ((s.cov_on = cfg != nullptr)) s.cov_cfg = *cfg;
    return ask(modules::kSetCovariance);
  }
  int cuts(const lsgpu_chain_cuts* c) {
    s.cuts_on = c && (c->n_reading != 0 || c->n_reference != 0);
    const std::string why = s.cuts_on ? chain_cuts_why(c) : std::string();
    if (!why.empty()) return say(why);
    if (s.cuts_on) s.cuts = *c;
    return ask(modules::kSetCuts);
  }
  int max_density(const lsgpu_max_density_config* cfg) {
    // (SurfaceNormalDataPointsFilter's knn comes with the chain: lsgpu_icp_compute checks that it is there)
    if (const char* why = cfg ? lsgpu_max_density_config_why(cfg, kSnfMinKnn) : nullptr) return say(why);
    if ((s.md_on = cfg != nullptr)) s.md_cfg = *cfg;
    return ask(modules::kSetMaxDensity);
  }
  int shadow(const lsgpu_shadow_config* cfg) {
    if (const char* why = cfg ? lsgpu_shadow_config_why(cfg) : nullptr) return say(why);
    if ((s.sh_on = cfg && (cfg->reading_eps >= 0.f || cfg->reference_eps >= 0.f))) s.sh_cfg = *cfg;
    return ask(modules::kSetShadow);
  }
  int cov_sampling(const lsgpu_cov_sampling_config* cfg) {
    if (const char* why = cfg ? lsgpu_cov_sampling_config_why(cfg) : nullptr) return say(why);
    if ((s.cs_on = cfg && (cfg->reading_nb_sample != 0 || cfg->reference_nb_sample != 0))) s.cs_cfg = *cfg;
    return ask(modules::kSetCovSampling);
  }
  int motion(const lsgpu_motion_config* cfg) {
    if (const char* why = cfg ? lsgpu_motion_config_why(cfg) : nullptr) return say(why);
    if ((s.mo_on = cfg && (cfg->dof != LSGPU_MOTION_DOF_6 || cfg->bound))) s.mo_cfg = *cfg;
    return ask(modules::kSetMotion);
  }
};

static ModuleSet module_set(const lsgpu_icp* h) {
  ModuleSet m;
  m.s = h->mods;
  m.f.error_minimizer = h->cfg.error_minimizer; m.f.matcher_knn = h->cfg.matcher_knn;
  m.f.chain = policy::chain_fields(h->cfg.matcher_max_dist, h->cfg.outlier_max_dist, h->cfg.outlier_min_dist, h->cfg.outlier_median_factor);
  m.f.comm = h->comm != nullptr;
  return m;
}

// the end of a setter: the set's text, and its state if every step passed (else the handle stays as it was)
static int commit_modules(lsgpu_icp* h, const ModuleSet& m, int rc) {
  h->err = m.err;
  if (rc != LSGPU_OK) return rc;
  if (!(h->mods.cov_on && m.s.cov_on)) h->quality_state = 0;   // (the covariance removed, or switched on for the first time)
  h->mods = m.s;
  return LSGPU_OK;
}

template <class Cfg>
static int set_module(lsgpu_icp* h, int (ModuleSet::*step)(const Cfg*), const Cfg* cfg) {
  if (!h) return LSGPU_BAD_ARG;
  ModuleSet m = module_set(h);
  return commit_modules(h, m, (m.*step)(cfg));
}

extern "C" {

void lsgpu_icp_config_yaml(lsgpu_icp_config* c) {  // icp_default.yaml:14-27
  std::memset(c, 0, sizeof(*c));
  c->trim_ratio = 0.75f;
  c->max_iterations = 40;
  c->min_diff_rot = 0.001f;
  c->min_diff_trans = 0.01f;
  c->smooth_length = 4;
  c->cell_size = 0.f;
}

void lsgpu_icp_config_default(lsgpu_icp_config* c) {  // ICP::setDefault(), laser_track.cpp:20
  std::memset(c, 0, sizeof(*c));
  c->trim_ratio = 0.85f;
  c->max_iterations = 40;
  c->min_diff_rot = 0.001f;
  c->min_diff_trans = 0.001f;
  c->smooth_length = 3;
  c->cell_size = 0.f;
}

void lsgpu_chain_config_yaml(lsgpu_chain_config* c) {  // icp_default.yaml:1-7
  std::memset(c, 0, sizeof(*c));
  c->reading_prob = 0.5f; c->ssn_knn = 10; c->ssn_ratio = 0.5f; c->seed = -1;
}

void lsgpu_chain_config_default(lsgpu_chain_config* c) {  // ICP::setDefault(), laser_track.cpp:20
  std::memset(c, 0, sizeof(*c));
  c->reading_prob = 0.75f; c->ssn_knn = 7; c->ssn_ratio = 0.5f; c->seed = -1;
}

int lsgpu_chain_config_check(const lsgpu_chain_config* c, int error_minimizer) {
  if (!c) return LSGPU_BAD_CONFIG;
  auto knn_ok = [](int k) { return k == 0 || (k >= 3 && k <= kSsnMaxKnn); };
  static_assert(kSnfMinKnn == 3 && kSnfMaxKnn == kSsnMaxKnn, "both reference filters take knn 3..32");
  if (!knn_ok(c->ssn_knn) || !knn_ok(c->sn_knn) || (c->ssn_knn > 0 && c->sn_knn > 0)) return LSGPU_BAD_CONFIG;
  if (c->ssn_knn == 0 && c->sn_knn == 0 && error_minimizer != LSGPU_MINIMIZER_POINT_TO_POINT) return LSGPU_BAD_CONFIG;
  return LSGPU_OK;
}

int lsgpu_icp_set_robust_filter(lsgpu_icp* h, const lsgpu_robust_config* cfg) { return set_module(h, &ModuleSet::robust, cfg); }
int lsgpu_icp_set_normals(lsgpu_icp* h, const lsgpu_normals_config* cfg) { return set_module(h, &ModuleSet::normals, cfg); }
int lsgpu_icp_set_covariance(lsgpu_icp* h, const lsgpu_covariance_config* cfg) { return set_module(h, &ModuleSet::covariance, cfg); }
int lsgpu_icp_set_chain_cuts(lsgpu_icp* h, const lsgpu_chain_cuts* cuts) { return set_module(h, &ModuleSet::cuts, cuts); }
int lsgpu_icp_set_max_density(lsgpu_icp* h, const lsgpu_max_density_config* cfg) { return set_module(h, &ModuleSet::max_density, cfg); }
int lsgpu_icp_set_shadow(lsgpu_icp* h, const lsgpu_shadow_config* cfg) { return set_module(h, &ModuleSet::shadow, cfg); }
int lsgpu_icp_set_cov_sampling(lsgpu_icp* h, const lsgpu_cov_sampling_config* cfg) { return set_module(h, &ModuleSet::cov_sampling, cfg); }
int lsgpu_icp_set_motion(lsgpu_icp* h, const lsgpu_motion_config* cfg) { return set_module(h, &ModuleSet::motion, cfg); }

int lsgpu_icp_set_modules(lsgpu_icp* h, const lsgpu_chain_modules* set) {
  if (!h || !set) return LSGPU_BAD_ARG;
  lsgpu_covariance_config cov;
  lsgpu_covariance_config_default(&cov);
  lsgpu_max_density_config md;
  lsgpu_max_density_config_default(&md);
  const bool has_cov = lsgpu_loaded_chain_covariance(&set->chain, &cov.sensor_std_dev) != 0;
  const bool has_md = lsgpu_loaded_chain_max_density(&set->chain, &md.max_density) != 0;
  ModuleSet m = module_set(h);
  int rc = m.robust(set->chain.has_robust ? &set->chain.robust : nullptr);
  if (!rc) rc = m.normals(set->chain.has_normals ? &set->chain.normals : nullptr);
  if (!rc) rc = m.covariance(has_cov ? &cov : nullptr);
  if (!rc) rc = m.cuts(&set->cuts);
  if (!rc) rc = m.max_density(has_md ? &md : nullptr);
  if (!rc) rc = m.shadow(&set->shadow);
  if (!rc) rc = m.cov_sampling(&set->cov_sampling);
  if (!rc) rc = m.motion(&set->motion);
  return commit_modules(h, m, rc);
}

int lsgpu_icp_get_robust_trace(lsgpu_icp* h, lsgpu_robust_trace* out, int cap) {
  return h ? fetch_trace(h, h->rb_trace_dev.p, h->rb_trace_n, out, cap) : 0;
}

int lsgpu_icp_get_quality(lsgpu_icp* h, lsgpu_icp_quality* out) {
  if (!h || !out) return LSGPU_BAD_ARG;
  h->err.clear();
  if (!h->mods.cov_on) { h->err = "get_quality: the covariance is not switched on (lsgpu_icp_set_covariance / PointToPlaneWithCovErrorMinimizer)"; return LSGPU_BAD_CONFIG; }
  if (h->quality_state == 0) { h->err = "get_quality: no alignment of this handle has returned LSGPU_OK since the covariance was switched on"; return LSGPU_NO_CONVERGENCE; }
  if (h->quality_state == 2) { h->err = "get_quality: H is singular (the pairs of the last iteration do not determine the pose)"; return LSGPU_NO_CONVERGENCE; }
  *out = h->quality;
  return LSGPU_OK;
}

int lsgpu_icp_get_normal_angle_trace(lsgpu_icp* h, lsgpu_normal_angle_trace* out, int cap) {
  return h ? fetch_trace(h, h->na_trace_dev.p, h->na_trace_n, out, cap) : 0;
}

int lsgpu_abi_version(void) { return LSGPU_ABI_VERSION; }

const char* lsgpu_strerror(int code) {
  switch (code) {
    case LSGPU_OK: return "ok";
    case LSGPU_NO_CONVERGENCE: return "ICP did not converge (PointMatcher::ConvergenceError)";
    case LSGPU_BAD_CONFIG: return "bad configuration";
    case LSGPU_HIP_ERROR: return "HIP runtime error";
    case LSGPU_BAD_ARG: return "bad argument";
    default: return "unknown";
  }
}

const char* lsgpu_last_error(lsgpu_icp* h) { return h ? h->err.c_str() : "null handle"; }

int lsgpu_icp_create(const lsgpu_icp_config* cfg, int device, lsgpu_icp** out) {
  if (!cfg || !out) return LSGPU_BAD_ARG;
  *out = nullptr;
  if (!(cfg->trim_ratio > 0.f && cfg->trim_ratio <= 1.f) || cfg->max_iterations < 1 ||
      cfg->smooth_length < 1 ||
      (cfg->error_minimizer != LSGPU_MINIMIZER_POINT_TO_PLANE && cfg->error_minimizer != LSGPU_MINIMIZER_POINT_TO_POINT) ||
      cfg->matcher_knn < 0 || cfg->matcher_knn > LSGPU_MATCHER_KNN_MAX)
    return LSGPU_BAD_CONFIG;
  // the chain's thresholds: 0 = absent; negative / NaN never; +inf only where it means "no bound" (the two maxDist)
  if (!(cfg->matcher_max_dist >= 0.f) || !(cfg->outlier_max_dist >= 0.f) ||
      !(cfg->outlier_min_dist >= 0.f) || std::isinf(cfg->outlier_min_dist) ||
      !(cfg->outlier_median_factor >= 0.f) || std::isinf(cfg->outlier_median_factor))
    return LSGPU_BAD_CONFIG;
  // the level-0 cell edge: <= 0 automatic, any finite positive value legal; NaN / +inf have no grid (hf = inf, inv_hf = 0)
  if (std::isnan(cfg->cell_size) || (std::isinf(cfg->cell_size) && cfg->cell_size > 0.f)) return LSGPU_BAD_CONFIG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    return LSGPU_HIP_ERROR;  // no silent CPU path: the caller must see that there is no GPU
  }
  lsgpu_icp* h = new lsgpu_icp();
  h->cfg = *cfg;
  h->device = device;
  std::memset(&h->grid, 0, sizeof(h->grid));
  if (hipSetDevice(device) != hipSuccess ||
      h->stream.ensure() != hipSuccess || h->pin.reserve(1) != hipSuccess ||
      h->ev0.ensure(hipEventDefault) != hipSuccess || h->ev1.ensure(hipEventDefault) != hipSuccess) {
    (void)hipGetLastError();
    delete h;   // (gives back what was made)
    return LSGPU_HIP_ERROR;
  }
  h->lane = h->main_lane();
  *out = h;
  return LSGPU_OK;
}

void lsgpu_icp_destroy(lsgpu_icp* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  // (waited for here, not only where the members go: nothing depends on the order they are declared in)
  for (const Stream* s : {&h->stream, &h->copy_stream, &h->draw_stream, &h->side_stream})
    if (*s) (void)hipStreamSynchronize(*s);
  if (h->comm && rccl_api()) (void)rccl_api()->CommDestroy(h->comm);
  delete h;
}

}  // extern "C"

// ---------------------------------------------------------------- internals

static int scan_u32(lsgpu_icp* h, const uint32_t* in, uint32_t* out, size_t n, bool inclusive = false, bool nonzero = false);

template <int ITEMS>
static void radix_pass(lsgpu_icp* h, const uint64_t* kin, const uint32_t* vin, uint64_t* kout, uint32_t* vout, int64_t n,
                       int shift, uint32_t mask, int nblocks) {
  uint32_t* bh = h->lane.scratch->sort_hist.p;
  uint32_t* dtot = bh + (size_t)256 * nblocks;
  // (the scan as the tail of k_rs_hist -- last block, ticket -- was measured 2 % slower end to end than this launch)
  hipLaunchKernelGGL(k_rs_hist<ITEMS>, dim3(nblocks), dim3(256), 0, h->lane.stream, kin, n, shift, mask, bh, nblocks);
  hipLaunchKernelGGL(k_rs_scan, dim3(256), dim3(256), 0, h->lane.stream, bh, nblocks, dtot);
  hipLaunchKernelGGL(k_rs_scatter<ITEMS>, dim3(nblocks), dim3(256), 0, h->lane.stream, kin, vin, kout, vout, n, shift, mask,
                     bh, dtot, nblocks);
}

// Stable sort of (h->lane.scratch->keys, h->lane.scratch->vals)[0..n) by the low `nbits` key bits; the result is in h->lane.scratch->keys_alt / h->lane.scratch->vals_alt
// (callers re-read those members: the two buffer pairs may have changed places).
static int sort_pairs(lsgpu_icp* h, int64_t n, int nbits) {
  HIPC(h->lane.scratch->keys_alt.reserve(n));
  HIPC(h->lane.scratch->vals_alt.reserve(n));
  const int items_env = tuning().sort_items;
  const int items = items_env ? items_env : n >= (1 << 21) ? 16 : n >= (1 << 19) ? 8 : 4;
  const int nblocks = (int)((n + 256 * items - 1) / (256 * items));
  HIPC(h->lane.scratch->sort_hist.reserve((size_t)256 * nblocks + 256));
  const int passes = std::max(1, (nbits + 7) / 8);   // (no key bits: one pass over an all-zero digit = a stable copy)
  uint64_t *kin = h->lane.scratch->keys.p, *kout = h->lane.scratch->keys_alt.p;
  uint32_t *vin = h->lane.scratch->vals.p, *vout = h->lane.scratch->vals_alt.p;
  for (int p = 0; p < passes; ++p) {
    const int shift = 8 * p, width = std::max(0, std::min(8, nbits - shift));
    const uint32_t mask = (1u << width) - 1u;
    if (items == 16) radix_pass<16>(h, kin, vin, kout, vout, n, shift, mask, nblocks);
    else if (items == 8) radix_pass<8>(h, kin, vin, kout, vout, n, shift, mask, nblocks);
    else radix_pass<4>(h, kin, vin, kout, vout, n, shift, mask, nblocks);
    std::swap(kin, kout); std::swap(vin, vout);
  }
  HIPC(hipGetLastError());
  if ((passes & 1) == 0) { std::swap(h->lane.scratch->keys, h->lane.scratch->keys_alt); std::swap(h->lane.scratch->vals, h->lane.scratch->vals_alt); }  // result is in `keys`
  return LSGPU_OK;  // sorted: keys_alt / vals_alt
}

// Stage an array of the caller's on the device (`count` elements of T): a device pointer is taken as it is, host memory is
// copied into `buf` on the current stream.  Returns a device pointer valid on that stream.
template <class T, class U>
static int stage_in(lsgpu_icp* h, const U* src, size_t count, DevBuf<T>& buf, const T** out) {
  if (is_device_ptr(src)) { *out = reinterpret_cast<const T*>(src); return LSGPU_OK; }
  HIPC(buf.reserve(count));
  HIPC(hipMemcpyAsync(buf.p, src, count * sizeof(T), hipMemcpyHostToDevice, h->lane.stream));
  *out = buf.p;
  return LSGPU_OK;
}
static int stage_points(lsgpu_icp* h, const float* src, int64_t n, DevBuf<float4>& buf, const float4** out) {
  return stage_in(h, src, (size_t)n, buf, out);
}

static int ensure_loop_buffers(lsgpu_icp* h, int64_t nq) {
  HIPC(h->ids.reserve(nq));
  HIPC(h->d2.reserve(nq));
  HIPC(h->strag.reserve(nq));
  HIPC(h->hist.reserve(3 * kHistBins));
  HIPC(h->sel.reserve(4));
  HIPC(h->hist_med.reserve(3 * kHistBins)); HIPC(h->sel_med.reserve(4));
  HIPC(h->ne_partials.reserve((size_t)kNeBlocksMax * 32));
  HIPC(h->ne_gpartials.reserve((size_t)(kNeBlocksMax / kNeGroup + 1) * 32));
  HIPC(h->ne_tickets.reserve((size_t)(kNeBlocksMax / kNeGroup + 2)));
  HIPC(h->ne_out.reserve(32));
  HIPC(h->limit_dev.reserve(4));
  HIPC(h->counters.reserve(64));
  return LSGPU_OK;
}

// Sort the reading coarsely (own frame), move it by T (rows) -> h->rdq (w = caller index).
// (gather == false: everything but the last kernel, which needs T -- lsgpu_icp_compute launches it once the reference's
// mean is known)
static int prepare_queries(lsgpu_icp* h, const float* q_xyz1, int64_t nq, const Mat34& T, bool gather = true) {
  const float4* src = nullptr;
  int rc = stage_points(h, q_xyz1, nq, h->q_in, &src);
  if (rc) return rc;
  HIPC(h->lane.scratch->keys.reserve(nq));
  HIPC(h->lane.scratch->vals.reserve(nq));
  HIPC(h->rdq.reserve(nq));
  HIPC(h->prev.reserve(nq));
  HIPC(h->lb.reserve(nq));
  // order of the queries inside the waves: chosen on the device from the cloud's angular sampling density
  const int qorder = tuning().query_order;   // -1: automatic
  const float qelev = tuning().q_elev, qsect = tuning().q_sect;   // 0: automatic
  HIPC(h->ang_cells.reserve(kDecCells + 8));
  HIPC(hipMemsetAsync(h->ang_cells.p, 0, (kDecCells + 8) * sizeof(uint32_t), h->lane.stream));
  if (qorder != 0) hipLaunchKernelGGL(k_query_ang_hist, dim3(nblk(nq)), dim3(256), 0, h->lane.stream, src, nq, h->ang_cells.p);
  hipLaunchKernelGGL(k_query_order, dim3(1), dim3(1024), 0, h->lane.stream, h->ang_cells.p, qorder, qelev, qsect);
  hipLaunchKernelGGL(k_query_keys, dim3(nblk(nq)), dim3(256), 0, h->lane.stream, src, nq, h->lane.scratch->keys.p, h->lane.scratch->vals.p,
                     h->ang_cells.p + kDecCells + 2);
  rc = sort_pairs(h, nq, 48);
  if (rc) return rc;
  if (gather) {
    hipLaunchKernelGGL(k_query_gather, dim3(nblk(nq)), dim3(256), 0, h->lane.stream, src, nq,
                       h->lane.scratch->vals_alt.p, T, h->rdq.p);
    HIPC(hipGetLastError());
  }
  h->nq = nq;
  {  // per-tile probe cache: new generation, tags cleared when (re)allocated
    const size_t nt = (size_t)((nq + 63) / 64);
    const bool grow = nt > h->cell_tags.cap;
    HIPC(h->cell_cache.reserve(nt * 64));
    HIPC(h->cell_tags.reserve(nt));
    if (grow) HIPC(hipMemsetAsync(h->cell_tags.p, 0, h->cell_tags.cap * sizeof(ulonglong2), h->lane.stream));
    if (++h->cache_gen == 0) h->cache_gen = 1;
  }
  h->dbg_launch_no = 0;
  return ensure_loop_buffers(h, nq);
}

static int run_select(lsgpu_icp* h, const float* d2, int n, uint32_t k, bool zero_hist, const IcpState* st,
                      bool use_comm, bool predicted, int passes = 3, float rank_ratio = 0.f, bool with_median = false);

// KDTreeMatcher maxDist of the handle, squared (one float multiply); +inf: none
static float matcher_max_d2(const lsgpu_icp* h) {
  const float m = h->cfg.matcher_max_dist;
  return (m > 0.f && !std::isinf(m)) ? m * m : INFINITY;
}
// does the handle take the chain plan (lsgpu_policy.h)?
static bool chain_on(const lsgpu_icp* h) {
  return policy::chain_fields(h->cfg.matcher_max_dist, h->cfg.outlier_max_dist, h->cfg.outlier_min_dist, h->cfg.outlier_median_factor,
                              h->mods.robust_on, h->mods.normals_on && h->mods.normals.max_angle >= 0.f);
}

static float price_share(const lsgpu_icp* h) {   // heavy lanes / searching lanes of the priced launch (its counters are on the host)
  uint64_t heavy = 0, searching = 0;
  for (int i = 0; i < kPriceSlots; ++i) { heavy += h->pin->price[i * kPriceStride]; searching += h->pin->price[i * kPriceStride + 1]; }
  return searching ? (float)((double)heavy / (double)searching) : 0.f;
}

// the next event record of a profiled align (a pool, reused across aligns), its first event on the stream
static int knn_event_begin(lsgpu_icp* h, lsgpu_icp::KnnEv** ev) {
  if (h->knn_events_used == h->knn_events.size()) {
    lsgpu_icp::KnnEv n;   // (a failure part-way: `n` takes what it has with it)
    for (Event* e : {&n.a, &n.b, &n.c, &n.d, &n.e}) HIPC(e->ensure(hipEventDefault));
    h->knn_events.push_back(std::move(n));
  }
  *ev = &h->knn_events[h->knn_events_used++];
  (*ev)->second = false;
  HIPC(hipEventRecord((*ev)->a, h->stream));
  return LSGPU_OK;
}

static KnnArgs knn_args(lsgpu_icp* h, const Mat34& T) {
  KnnArgs a;
  a.rdq = h->rdq.p; a.nq = (int)h->nq; a.T = T; a.g = h->grid; a.pts = h->pts.p;
  a.chunks = h->chunks.p; a.cgroups = h->chunk_groups.p; a.soa = reinterpret_cast<const float4*>(h->soa.p); a.chunk_soa = h->soa_base.p; a.ids = h->ids.p; a.d2 = h->d2.p; a.prev = h->prev.p;
  a.strag = h->strag.p; a.strag_count = h->counters.p + 32;
  a.r_cap = 1.0f; a.group_r = 0.75f; a.cap2 = INFINITY; a.st = nullptr; a.use_state_cap = 0; a.lb = nullptr;
  a.spread_route_r = 0.f; a.route_chunks = 1 << 30; a.route_dense = 1 << 30; a.route_heavy_max = -1; a.sel_hist2 = nullptr; a.sel_below = nullptr;
  a.sel_hist3w = nullptr; a.sel_force = 0; a.write_all = 1; a.spread_flag = nullptr; a.spread_list = nullptr; a.spread_cnt = nullptr; a.front_blocks = 0;
  a.price.count = nullptr;
  a.gap = tuning().gap;
  a.ntiles = (int)((h->nq + 63) / 64); a.pad_index = (int)h->nr;
  a.chunk_budget = tuning().chunk_budget;
  a.cell_cache = h->cell_cache.p; a.cell_tags = h->cell_tags.p; a.cache_gen = h->cache_gen;
  a.dbg = h->knn_dbg.p;
  a.dbg_wave = h->knn_dbg_wave.p;
  { a.dbg_flags = tuning().knn_dbg;
    if ((a.dbg_flags & (64 | 128 | 256 | 512 | 1024 | 2048)) && h->dbg_launch_no < 6) a.dbg_flags = 0; }  // early-exit ablations from launch 6 on
  return a;
}

// findClosests for the queries in h->rdq: fills h->ids (sorted-reference index), h->d2, h->prev.
//   T / st   : the transform comes from the argument (kernel-level API) or from the loop state
//   seed     : the queries have no warm start yet (first iteration, kernel-level API)
//   capped   : search cap from the loop state (exact below cap, see lsgpu_knn.hip.h); otherwise uncapped,
//              followed by the straggler fallback
//   it       : what the launch policy decided for this iteration (lsgpu_policy.h); the kernel-level API passes a seeded,
//              uncapped, wide search outside any loop
static int run_knn(lsgpu_icp* h, const Mat34& T, const IcpState* st, const policy::Iteration& it, bool timed,
                   uint32_t seed_rank = 0xFFFFFFFFu) {
  const bool seed = it.seed, capped = it.capped, wide = it.wide, predicted = it.predicted, committed = it.committed;
  policy::State& pol = h->pol;
  const policy::Config& pc = h->pol_cfg;
  const int nq = (int)h->nq;
  KnnArgs a = knn_args(h, T);
  h->dbg_launch_no++;
  a.st = st;
  a.lb = st ? h->lb.p : nullptr;
  a.use_state_cap = capped ? 1 : 0;
  a.write_all = (seed || !capped || !st) ? 1 : 0;
  if (capped) a.r_cap = INFINITY;  // capped balls are never larger than the cap: no straggler by radius
  // `wide`: the balls may still be large (first iterations of an align, retries, kernel-level API): spread
  // waves with wide balls go to the wave-per-query pass, which is launched after the tile kernel
  const Tuning& tn = tuning();
  const bool settled = capped && !wide && st;   // (capped, balls already small)
  a.spread_route_r = wide ? tn.route_r : 0.f;
  a.chunk_budget = wide ? tn.chunk_budget_wide : tn.chunk_budget;
  // front rows: spread tiles are remembered from the first searches on and searched row-wise by the first workgroups
  // of the settled launches themselves -- no hand-over, no second launch
  if (st && h->spread_cnt.p) {   // (lsgpu_icp_align reserves the list before its loop)
    a.spread_flag = h->spread_flag.p; a.spread_list = h->spread_list.p; a.spread_cnt = h->spread_cnt.p;
    // (the front is sized from the list's length as the host last saw it -- it travels with the state every few
    // iterations --, from a guess before that: surplus workgroups exit at once, a listed tile beyond the front, or one
    // that turns spread late, searches per lane inside the kernel)
    if (settled) {
      const int tiles = h->n_spread_known ? (int)h->n_spread_host : std::min(tn.front_guess, a.ntiles);
      a.front_blocks = kFrontPerTile * tiles;
    }
  }
  if (predicted && !wide && capped && st) { a.sel_hist2 = h->hist.p + kHistBins; a.sel_below = h->sel_aux.p; }
  if (committed && a.sel_below) { a.sel_hist3w = (h->comm || !tuning().fused_select) ? h->sel_win.p : nullptr; a.sel_force = 1; }   // (the window table: aligned mode only)
  a.route_chunks = tn.route_chunks;
  a.route_heavy_max = st ? tn.route_heavy_max : -1;   // (the ticket lives in the loop's scratch, re-armed every iteration)
  a.route_dense = tn.route_dense;
  // the search before the first one through the direction index prices the index (lsgpu_knn.hip.h: cone_price)
  const bool pricing = pol.pricing(pc, it, st != nullptr);
  if (pricing) {
    constexpr size_t kPriceBytes = (size_t)kPriceSlots * kPriceStride * sizeof(uint32_t);
    HIPC(h->price_cnt.reserve((size_t)kPriceSlots * kPriceStride));
    HIPC(hipMemsetAsync(h->price_cnt.p, 0, kPriceBytes, h->stream));
    a.price.ox = h->cone.ox; a.price.oy = h->cone.oy; a.price.oz = h->cone.oz; a.price.rs = h->cone.rs; a.price.cs = h->cone.cs;
    a.price.dens4 = (float)(0.25 * (double)h->nr / ((double)h->cone.rows * (double)h->cone.cols));
    a.price.heavy = tn.cone_heavy_steps; a.price.count = h->price_cnt.p;
  }
  if (seed && !st) HIPC(hipMemsetAsync(a.strag_count, 0, sizeof(uint32_t), h->stream));  // (align: k_align_init, then re-armed by k_normal_eq_loop)
  if (seed) hipLaunchKernelGGL(k_knn_seed, dim3(nblk(nq)), dim3(256), 0, h->stream, a);
  if (seed && capped && st && seed_rank != 0xFFFFFFFFu) {
    // first iteration of an align: cap = trim quantile of the seed distances (k_knn_seed left them in d2)
    const int rs = run_select(h, h->d2.p, nq, seed_rank, false /* k_align_init armed the tables */, st, true, false, 2);
    if (rs) return rs;
    hipLaunchKernelGGL(k_seed_cap, dim3(1), dim3(256), 0, h->stream, h->hist.p, h->sel.p + 1, h->state.p);
  }
  // two launches of every alignment are timed for policy::index_not_paying (not in profiled runs: they time everything)
  const bool pay_probe = !timed && st && pol.cone_ok && h->ev_pay[0];
  const bool pay_voxel = pay_probe && !seed && it.ordinal == pc.cone_from - 1 && !h->pay_voxel_timed;
  if (pay_voxel) HIPC(hipEventRecord(h->ev_pay[0], h->stream));
  lsgpu_icp::KnnEv* ev = nullptr;
  if (timed) { const int re = knn_event_begin(h, &ev); if (re) return re; }
  if (pol.wants_occupancy(it, st != nullptr)) {
    // first search through the index for this reference: is it worth it?  The windows of a lane grow with the number of
    // reference points per direction -- measured on local maps of K scans of 1 M points (devtools/cone_density.py), kNN
    // per settled launch: K = 1: 48 us against 82 with the voxel grid, K = 3: 69 / 107, K = 8: 423 / 186.  Points per
    // occupied bin: 2, 3, 8.  (The wait is for a copy queued behind the build; the device is in the first iterations.)
    HIPC(hipEventSynchronize(h->cone_occ_ready));
    const uint32_t occ = h->pin->cone_occ;
    pol.set_occupancy(pc, occ ? (float)((double)h->nr / (double)occ) : 1e9f);
    h->cone_occupancy = pol.cone_occupancy; h->cone_dense = pol.cone_dense; h->cone_decided = true;   // (per reference: a reused reference keeps the verdict)
  }
  if (pol.wants_first_price(it)) {
    // ... and what would this align pay for it?  The search before this one counted the lanes whose windows would be long
    // (wide balls next to O: a wall a metre from the sensor; a sparse reading on a dense map that converges in steps of
    // millimetres): the index evaluates each lane's windows alone, the voxel kernel shares one candidate stream among 64
    // lanes whose balls overlap -- measured on such clouds 1.6-2.0 ms per search against 0.6.  A RE-pricing
    // count (an alignment that was priced off) is not taken here: it belongs to the look it was launched in front of.
    HIPC(hipEventSynchronize(h->price_ready));
    pol.set_first_price(pc, price_share(h));
  }
  const policy::KnnKernel kern = pol.kernel(pc, it, st != nullptr);
  if (kern != policy::KnnKernel::Tile) {
    // settled launch: every lane searches its own windows of the direction-sorted reference (lsgpu_cone.hip.h)
    if (h->cone_pending) {   // (built on the side stream beside the first iterations: lsgpu_icp_compute)
      HIPC(hipStreamWaitEvent(h->stream, h->cone_done, 0));
      h->cone_pending = false;
    }
    a.front_blocks = 0;
    const bool pay_index = pay_probe && kern == policy::KnnKernel::Cone && h->pay_voxel_timed && !h->pay_index_timed;
    if (pay_index) HIPC(hipEventRecord(h->ev_pay[2], h->stream));
    if (kern == policy::KnnKernel::ConeProbe)   // balls as wide as the last ICP step: a probe of the query's own direction first
      hipLaunchKernelGGL((k_knn_cone<LSGPU_CONE_WAVES, true>), dim3((a.ntiles + LSGPU_CONE_WAVES - 1) / LSGPU_CONE_WAVES), dim3(LSGPU_CONE_WAVES * 64), (size_t)h->cone.rows * sizeof(float4), h->stream, a, h->cone);
    else
      hipLaunchKernelGGL((k_knn_cone<LSGPU_CONE_WAVES, false>), dim3((a.ntiles + LSGPU_CONE_WAVES - 1) / LSGPU_CONE_WAVES), dim3(LSGPU_CONE_WAVES * 64), (size_t)h->cone.rows * sizeof(float4), h->stream, a, h->cone);
    if (timed) HIPC(hipEventRecord(ev->b, h->stream));
    if (pay_index) { HIPC(hipEventRecord(h->ev_pay[3], h->stream)); h->pay_index_timed = true; }
    HIPC(hipGetLastError());
    return LSGPU_OK;
  }
  if (wide && tn.lazy_need)   // balls still as wide as the last ICP step: the instantiation that re-tests chunks before fetching them
    hipLaunchKernelGGL((k_knn_tile<1, true>), dim3(a.ntiles + a.front_blocks), dim3(64), 0, h->stream, a);
  else if (!wide && tn.lane_split)   // settled: most tiles have fewer than 32 searching lanes -- their candidates are shared out over the idle ones
    hipLaunchKernelGGL((k_knn_tile<1, false, true>), dim3(a.ntiles + a.front_blocks), dim3(64), 0, h->stream, a);
  else
    hipLaunchKernelGGL((k_knn_tile<1, false>), dim3(a.ntiles + a.front_blocks), dim3(64), 0, h->stream, a);
  if (timed) HIPC(hipEventRecord(ev->b, h->stream));
  // stragglers (balls > r_cap) only exist in uncapped launches, routed waves only in wide ones: capped launches that
  // are not wide hand nothing over
  const bool second = !capped || a.spread_route_r > 0.f;
  if (second) hipLaunchKernelGGL(k_knn_fallback, dim3(kFallbackBlocks), dim3(256), 0, h->stream, a);
  if (timed && second) { ev->second = true; HIPC(hipEventRecord(ev->c, h->stream)); }   // (an event pair around nothing still reads ~5 us)
  if (pay_voxel) { HIPC(hipEventRecord(h->ev_pay[1], h->stream)); h->pay_voxel_timed = true; }
  if (pricing) {
    HIPC(h->price_ready.ensure(hipEventDisableTiming));
    HIPC(hipMemcpyAsync(h->pin->price, h->price_cnt.p, (size_t)kPriceSlots * kPriceStride * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPC(hipEventRecord(h->price_ready, h->stream));
    pol.priced();
  }
  HIPC(hipGetLastError());
  return LSGPU_OK;
}

// ---- k nearest matches (lsgpu_knn_k.hip.h): the k-best search of the queries in h->rdq into h->kmatch / h->kd2.
//   st    : loop state (T from it, `done` exits) or nullptr (T from the argument: kernel-level API)
//   seed  : the queries have no warm start yet (first iteration of an align, kernel-level API)
template <int K, bool MAXD>
static void launch_knn_k_(lsgpu_icp* h, const KnnKArgs& a, bool seed) {
  const int nq = a.nq;
  if (seed) hipLaunchKernelGGL((k_knnk_seed<K, MAXD>), dim3(nblk(nq)), dim3(256), 0, h->stream, a);
  hipLaunchKernelGGL((k_knnk_tile<K, MAXD>), dim3((nq + 63) / 64), dim3(64), 0, h->stream, a);
  hipLaunchKernelGGL((k_knnk_fallback<K, MAXD>), dim3(kFallbackBlocks), dim3(256), 0, h->stream, a);
}
template <int K>
static void launch_knn_k(lsgpu_icp* h, const KnnKArgs& a, bool seed) {
  if (a.max_d2 < INFINITY) launch_knn_k_<K, true>(h, a, seed);   // KDTreeMatcher maxDist: every bound cut to it
  else launch_knn_k_<K, false>(h, a, seed);
}

template <size_t... I>
static void launch_knn_k_any(lsgpu_icp* h, const KnnKArgs& a, bool seed, int k, std::index_sequence<I...>) {
  static void (*const tab[])(lsgpu_icp*, const KnnKArgs&, bool) = {launch_knn_k<(int)I + 1>...};   // k = 1 .. kKnnKMax
  tab[k - 1](h, a, seed);
}

static int run_knn_k(lsgpu_icp* h, int k, const Mat34& T, const IcpState* st, bool seed, bool timed) {
  const int64_t nq = h->nq;
  HIPC(h->kmatch.reserve((size_t)k * nq)); HIPC(h->kd2.reserve((size_t)k * nq));
  KnnKArgs a;
  a.rdq = h->rdq.p; a.nq = (int)nq; a.T = T; a.st = st; a.g = h->grid; a.pts = h->pts.p; a.chunks = h->chunks.p;
  a.kmatch = h->kmatch.p; a.kd2 = h->kd2.p; a.strag = h->strag.p; a.strag_count = h->counters.p + 32;
  a.r_cap = kKnnKRCap; a.max_d2 = matcher_max_d2(h);
  if (!st) HIPC(hipMemsetAsync(a.strag_count, 0, sizeof(uint32_t), h->stream));  // (align: k_align_init, then the normal equations re-arm it)
  lsgpu_icp::KnnEv* ev = nullptr;
  if (timed) { const int re = knn_event_begin(h, &ev); if (re) return re; }   // (the same event record as run_knn: main launches a..b, fallback b..c)
  if (k < 1 || k > kKnnKMax) { h->err = "knn_k: k out of range"; return LSGPU_BAD_ARG; }
  launch_knn_k_any(h, a, seed, k, std::make_index_sequence<kKnnKMax>{});
  if (timed) { HIPC(hipEventRecord(ev->b, h->stream)); }
  HIPC(hipGetLastError());
  return LSGPU_OK;
}

#define RCCLC(expr)                                                                     \
  do {                                                                                  \
    ncclResult_t r__ = (expr);                                                          \
    if (r__ != ncclSuccess) {                                                           \
      h->err = std::string("RCCL: ") + (rccl_api()->GetErrorString ? rccl_api()->GetErrorString(r__) : "error"); \
      return LSGPU_HIP_ERROR;                                                           \
    }                                                                                   \
  } while (0)

// TrimmedDist order statistic of d2[0..n) -> rank k; leaves hist3 + sel[2] for select_limit().
// rank_ratio > 0: the rank is not `k` but taken on the device from the number of FINITE distances (k_chain_rank:
// quantiles skip invalid matches); with_median: a second run of the refining passes finds the 0.5 quantile into
// hist_med / sel_med.  Neither in the split-scan mode.
static int run_select(lsgpu_icp* h, const float* d2, int n, uint32_t k, bool zero_hist, const IcpState* st,
                      bool use_comm, bool predicted, int passes, float rank_ratio, bool with_median) {
  if (zero_hist) HIPC(hipMemsetAsync(h->hist.p, 0, 3 * kHistBins * sizeof(uint32_t), h->stream));
  if (zero_hist && !(rank_ratio > 0.f)) {  // sel[0] = {0, k}: constant during an align, uploaded once
    h->pin->sel0 = SelState{0u, k};
    HIPC(hipMemcpyAsync(h->sel.p, &h->pin->sel0, sizeof(SelState), hipMemcpyHostToDevice, h->stream));
  }
  const int nb = std::min(kHistBlocks, nblk(n));
  const int pr = predicted && st ? 1 : 0;
  hipLaunchKernelGGL(k_hist1<HistPlain>, dim3(nb), dim3(256), 0, h->stream, d2, n, h->hist.p, st, pr, HistPlain{});
  if (rank_ratio > 0.f) {
    hipLaunchKernelGGL(k_chain_rank, dim3(1), dim3(256), 0, h->stream, h->hist.p, st, rank_ratio, h->sel.p,
                       with_median ? h->sel_med.p : (SelState*)nullptr, h->hist_med.p);
    if (with_median) {   // the median's run: same first table, its own second and third
      hipLaunchKernelGGL((k_hist_refine<2, HistPlain>), dim3(nb), dim3(256), 0, h->stream, d2, n, h->hist.p,
                         h->sel_med.p, h->sel_med.p + 1, h->hist_med.p + kHistBins, st, 0, h->sel_aux.p, HistPlain{});
      hipLaunchKernelGGL((k_hist_refine<3, HistPlain>), dim3(nb), dim3(256), 0, h->stream, d2, n, h->hist_med.p + kHistBins,
                         h->sel_med.p + 1, h->sel_med.p + 2, h->hist_med.p + 2 * kHistBins, st, 0, h->sel_aux.p, HistPlain{});
    }
  }
  if (use_comm && h->comm) { comm_mark(h, true); RCCLC(rccl_api()->AllReduce(h->hist.p, h->hist.p, kHistBins, ncclUint32, ncclSum, h->comm, h->stream)); comm_mark(h, false); }
  hipLaunchKernelGGL((k_hist_refine<2, HistPlain>), dim3(nb), dim3(256), 0, h->stream, d2, n, h->hist.p,
                     h->sel.p, h->sel.p + 1, h->hist.p + kHistBins, st, pr, h->sel_aux.p, HistPlain{});
  if (use_comm && h->comm) { comm_mark(h, true); RCCLC(rccl_api()->AllReduce(h->hist.p + kHistBins, h->hist.p + kHistBins, kHistBins, ncclUint32, ncclSum, h->comm, h->stream)); comm_mark(h, false); }
  if (passes < 3) { HIPC(hipGetLastError()); return LSGPU_OK; }   // (fused select: k_normal_eq_loop settles the limit inside its slice)
  hipLaunchKernelGGL((k_hist_refine<3, HistPlain>), dim3(nb), dim3(256), 0, h->stream, d2, n,
                     h->hist.p + kHistBins, h->sel.p + 1, h->sel.p + 2, h->hist.p + 2 * kHistBins, st, pr,
                     h->sel_aux.p, HistPlain{});
  if (use_comm && h->comm) { comm_mark(h, true); RCCLC(rccl_api()->AllReduce(h->hist.p + 2 * kHistBins, h->hist.p + 2 * kHistBins, kHistBins, ncclUint32, ncclSum, h->comm, h->stream)); comm_mark(h, false); }
  HIPC(hipGetLastError());
  return LSGPU_OK;
}

// RobustOutlierFilter's MAD, behind a run_select with the median (hist / hist_med still hold this iteration's tables): the
// three passes of the select over |d2 - median| with rank m / 2; the weighted k_normal_eq_loop reads the result.
static int run_mad(lsgpu_icp* h, const float* d2, int n, const IcpState* st) {
  const int nb = std::min(kHistBlocks, nblk(n));
  hipLaunchKernelGGL(k_mad_begin, dim3(1), dim3(256), 0, h->stream, h->hist.p, st, h->hist_med.p, h->sel_med.p, h->rb_state.p,
                     h->rb_sel.p, h->rb_hist.p);
  const HistAbsDev x{&h->rb_state.p->median};
  hipLaunchKernelGGL(k_hist1<HistAbsDev>, dim3(nb), dim3(256), 0, h->stream, d2, n, h->rb_hist.p, st, 0, x);
  hipLaunchKernelGGL((k_hist_refine<2, HistAbsDev>), dim3(nb), dim3(256), 0, h->stream, d2, n, h->rb_hist.p, h->rb_sel.p,
                     h->rb_sel.p + 1, h->rb_hist.p + kHistBins, st, 0, h->sel_aux.p, x);
  hipLaunchKernelGGL((k_hist_refine<3, HistAbsDev>), dim3(nb), dim3(256), 0, h->stream, d2, n, h->rb_hist.p + kHistBins,
                     h->rb_sel.p + 1, h->rb_sel.p + 2, h->rb_hist.p + 2 * kHistBins, st, 0, h->sel_aux.p, x);
  HIPC(hipGetLastError());
  return LSGPU_OK;
}

// Direction index of the current reference (lsgpu_cone.hip.h) on the handle's current stream / sort scratch: keys of
// the Morton-sorted points, three radix passes, SoA copy + position map + (row, column) table + zeta range per row.
// is a direction index built for the current reference at all?  (host-side facts only)
static bool cone_wanted(const lsgpu_icp* h) {
  const int64_t nr = h->nr;
  if (h->cfg.matcher_knn >= 2 || chain_on(h)) return false;   // (the k-match loop and the chain plan search the voxel grid only)
  if (!(tuning().cone && h->cone_origin_inside && nr >= 1024)) return false;
  // a reference with more points than 0.6 x the occupancy limit x the number of bins cannot come out below the limit
  // (measured: 4.3 / 6.3 / 8.5 points per occupied bin at 3.0 / 4.0 / 5.0 per bin): spare it the build (1.8 ms at 8 M points)
  return !((double)nr > 0.6 * (double)tuning().cone_max_occupancy * (double)tuning().cone_rows * (double)tuning().cone_cols);
}
static int build_cone_index(lsgpu_icp* h) {
  const int64_t nr = h->nr;
  h->cone_ok = false;
  if (!cone_wanted(h)) return LSGPU_OK;
  ConeDev c;
  std::memset(&c, 0, sizeof(c));
  c.ox = -h->mean[0]; c.oy = -h->mean[1]; c.oz = -h->mean[2];
  c.rows = tuning().cone_rows; c.cols = tuning().cone_cols;
  const float zr = std::max(h->cone_zeta_hi - h->cone_zeta_lo, 1e-3f);
  c.z0 = h->cone_zeta_lo - 1e-5f - 1e-4f * zr;
  c.rs = (float)c.rows / (zr * 1.0002f + 2e-5f);
  c.cs = (float)c.cols * 0.25f;
  const size_t npad = (((size_t)nr + 3) & ~(size_t)3) + kConePad, nkeys = (size_t)c.rows * (size_t)c.cols;
  HIPC(h->cone_soa.reserve((size_t)kConeGF4 * npad));
  HIPC(h->cone_map.reserve(npad));
  HIPC(h->cone_tab.reserve(nkeys + 1)); HIPC(h->cone_rowz.reserve((size_t)c.rows));
  HIPC(h->lane.scratch->keys.reserve(nr)); HIPC(h->lane.scratch->vals.reserve(nr));
  c.soa = reinterpret_cast<const float4*>(h->cone_soa.p); c.map = h->cone_map.p; c.tab = h->cone_tab.p; c.rowz = h->cone_rowz.p;
  hipLaunchKernelGGL(k_cone_keys, dim3(nblk(nr)), dim3(256), 0, h->lane.stream, h->pts.p, nr, c,
                     h->lane.scratch->keys.p, h->lane.scratch->vals.p);
  int nbits = 1;
  while (((size_t)1 << nbits) < nkeys) ++nbits;
  const int rc = sort_pairs(h, nr, nbits);
  if (rc) return rc;
  HIPC(h->cone_occ.reserve(1));
  HIPC(hipMemsetAsync(h->cone_occ.p, 0, sizeof(uint32_t), h->lane.stream));
  hipLaunchKernelGGL(k_cone_gather, dim3(nblk((int64_t)npad)), dim3(256), 0, h->lane.stream, h->pts.p, h->lane.scratch->vals_alt.p,
                     h->lane.scratch->keys_alt.p, nr, c, h->cone_soa.p, h->cone_map.p, h->cone_tab.p);
  hipLaunchKernelGGL(k_cone_rows, dim3(c.rows), dim3(256), 0, h->lane.stream, c, h->cone_rowz.p, h->cone_occ.p);
  HIPC(hipGetLastError());
  // the number of occupied bins travels to the host behind the build; lsgpu_icp_align looks at it before its first
  // search through the index (the device is busy with the first two iterations by then)
  // (an earlier build's copy may still be in flight on the side stream when the next one starts -- wait for it before the
  // word is reset)
  if (!h->cone_occ_ready) HIPC(h->cone_occ_ready.ensure(hipEventDisableTiming));
  else if (hipEventSynchronize(h->cone_occ_ready) != hipSuccess) (void)hipGetLastError();
  uint32_t* ho = &h->pin->cone_occ;
  *ho = 0u;
  HIPC(hipMemcpyAsync(ho, h->cone_occ.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->lane.stream));
  HIPC(hipEventRecord(h->cone_occ_ready, h->lane.stream));
  h->cone = c;
  h->cone_ok = true;
  h->cone_decided = false;
  return LSGPU_OK;
}

static uint32_t trim_rank(int64_t n, float ratio) {
  int64_t k = (int64_t)((float)n * ratio);  // values.size() * ratio, truncated
  if (k >= n) k = n - 1;
  if (k < 0) k = 0;
  return (uint32_t)k;
}

// What the callers inside this file know about the align they start and its C signature does not carry: the queries are
// ordered and moved already, on the side lane (the loop's stream waits for side_done); h->rd_nrm holds the normals of this
// very reading; the direction index's build goes to the side lane behind the first iteration.
struct AlignExtras { bool queries_prepared, reading_normals, build_index_on_side; };
static int align_run(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float T_init[16], float T_out[16], lsgpu_icp_stats* stats, AlignExtras extras);

// The reference's grid (steps 2-3) in two halves around its one host round trip; lsgpu_icp_compute enqueues the reading's
// side between and behind them.  First half: staging, stats and geometry, keys, sort, gather, chunks, cell counts -> host.
// Second half, behind the wait for those counts: table sizes, chunk bounds and boxes, the SoA copy, the cell tables -- the
// handle has its grid then; the direction index is build_cone_index's, called by whoever wants it built now.
static int ref_build_front(lsgpu_icp* h, const float* ref_xyz1, const float* ref_normals, int64_t nr) {
  h->nr = 0;
  h->have_normals = ref_normals != nullptr;
  const float4* src = nullptr;
  int rc = stage_points(h, ref_xyz1, nr, h->ref_in, &src);
  if (rc) return rc;
  const float* nsrc = nullptr;
  if (ref_normals && (rc = stage_in(h, ref_normals, (size_t)3 * nr, h->nrm_in, &nsrc))) return rc;
  // ---- mean + bounding box (step 2) and the grid geometry, all on the device: nothing below waits for the host
  // until the cell counts are needed (one round trip per set_reference; there used to be two)
  HIPC(h->stat_partials.reserve(kStatBlocks + 1));
  HIPC(h->geom.reserve(1));
  const int sb = std::min(kStatBlocks, nblk(nr));
  hipLaunchKernelGGL(k_ref_stats, dim3(sb), dim3(256), 0, h->stream, src, nr, h->stat_partials.p);
  hipLaunchKernelGGL(k_ref_stats_final, dim3(1), dim3(64), 0, h->stream, h->stat_partials.p, sb,
                     h->stat_partials.p + kStatBlocks, nr, h->cfg.cell_size, h->geom.p);
  // ---- keys, sort, gather: 16 key bits per axis in total (`bits` address level-0 cells, `fine` order points inside
  // a cell; the split is chosen by k_ref_stats_final), i.e. always 48 key bits
  HIPC(h->lane.scratch->keys.reserve(nr)); HIPC(h->lane.scratch->vals.reserve(nr));
  HIPC(h->pts.reserve(nr + 8)); HIPC(h->nrm.reserve(nr)); HIPC(h->ref_inv.reserve(nr));
  hipLaunchKernelGGL(k_ref_keys, dim3(nblk(nr)), dim3(256), 0, h->stream, src, nr, h->geom.p, h->lane.scratch->keys.p, h->lane.scratch->vals.p);
  rc = sort_pairs(h, nr, 48);
  if (rc) return rc;
  hipLaunchKernelGGL(k_ref_gather, dim3(nblk(nr + 8)), dim3(256), 0, h->stream, src, nsrc, nr,
                     h->lane.scratch->vals_alt.p, h->geom.p, h->pts.p, h->nrm.p, h->ref_inv.p);
  // ---- chunks: flags -> inclusive scan -> bounds
  HIPC(h->flags.reserve(nr)); HIPC(h->cidx.reserve(nr));
  hipLaunchKernelGGL(k_chunk_flags, dim3(nblk(nr)), dim3(256), 0, h->stream, h->lane.scratch->keys_alt.p, nr, h->geom.p,
                     h->flags.p);
  rc = scan_u32(h, h->flags.p, h->cidx.p, (size_t)nr, /*inclusive*/ true);
  if (rc) return rc;
  // ---- cell counts per level (+ chunk count, + the geometry) -> host, to size the tables
  HIPC(h->counters.reserve(64));
  HIPC(hipMemsetAsync(h->counters.p, 0, 64 * sizeof(uint32_t), h->stream));
  hipLaunchKernelGGL(k_cells_count, dim3(std::min(512, nblk(nr))), dim3(256), 0, h->stream, h->lane.scratch->keys_alt.p, nr, h->geom.p,
                     h->counters.p);
  {
    static_assert(sizeof(GeomDev) % 4 == 0, "copied word by word");
    ToHost c{}; int used = 0;
    to_host_add(&c, &used, h->counters.p, h->pin->cells, sizeof h->pin->cells);
    to_host_add(&c, &used, h->cidx.p + (nr - 1), &h->pin->nchunks, sizeof(uint32_t));
    to_host_add(&c, &used, h->geom.p, &h->pin->geom, sizeof(GeomDev));
    hipLaunchKernelGGL(k_to_host, dim3(1), dim3(64), 0, h->stream, c);
    HIPC(hipGetLastError());
  }
  return LSGPU_OK;
}
static int ref_build_back(lsgpu_icp* h, int64_t nr) {
  const uint32_t* hc = h->pin->cells;
  const GeomDev* hg = &h->pin->geom;
  HIPC(hipStreamSynchronize(h->stream));
  if (hg->bad) { h->err = "set_reference: non-finite coordinates"; return LSGPU_BAD_ARG; }
  for (int d = 0; d < 3; ++d) h->mean[d] = hg->mean[d];
  const int bits = hg->bits, fine = hg->fine;
  const float h0 = hg->h0;
  GridDev g;
  std::memset(&g, 0, sizeof(g));
  g.ox = hg->ox; g.oy = hg->oy; g.oz = hg->oz;
  g.h0 = h0; g.hf = hg->hf; g.inv_hf = hg->inv_hf; g.fine = fine; g.bits = bits;
  const uint32_t nchunks = h->pin->nchunks;
  size_t total = 0, off[kMaxLevels];
  uint32_t cap[kMaxLevels], ncell[kMaxLevels];
  for (int l = 0; l <= bits; ++l) ncell[l] = hc[l];
  for (int l = 0; l <= bits; ++l) {
    uint32_t c = 4;
    while (c < 4u * ncell[l]) c <<= 1;   // (load <= 0.25: the longest probe chain of the benchmark scan's tables is 7 slots)
    cap[l] = c; off[l] = total; total += c;
  }
  HIPC(h->bounds.reserve((size_t)nchunks + 1));
  HIPC(h->chunks.reserve(nchunks));
  hipLaunchKernelGGL(k_chunk_bounds, dim3(nblk(nr)), dim3(256), 0, h->stream, h->flags.p, h->cidx.p,
                     nr, h->bounds.p);
  hipLaunchKernelGGL(k_chunk_boxes, dim3((nchunks + 3) / 4), dim3(256), 0, h->stream, h->pts.p,
                     h->bounds.p, nchunks, h->chunks.p);
  // chunk-blocked SoA copy for the broadcast evaluation: <= 3 rounding slots per chunk
  HIPC(h->soa_cnt4.reserve(nchunks)); HIPC(h->soa_first.reserve(nchunks)); HIPC(h->soa_base.reserve(nchunks));
  HIPC(h->soa.reserve(3 * ((size_t)nr + 3 * (size_t)nchunks) + 16));
  HIPC(h->chunk_groups.reserve((size_t)nchunks / kChunkGroup + 1));
  hipLaunchKernelGGL(k_chunk_cnt4, dim3((nchunks + 255) / 256), dim3(256), 0, h->stream, h->bounds.p, nchunks,
                     h->soa_cnt4.p, (const ChunkDesc*)h->chunks.p, h->chunk_groups.p);
  const int rc = scan_u32(h, h->soa_cnt4.p, h->soa_first.p, nchunks);
  if (rc) return rc;
  hipLaunchKernelGGL(k_soa_fill, dim3((nchunks + 3) / 4), dim3(256), 0, h->stream, h->pts.p, h->bounds.p,
                     h->soa_first.p, nchunks, h->soa.p, h->soa_base.p);
  HIPC(h->tables.reserve(total));
  HIPC(hipMemsetAsync(h->tables.p, 0xFF, total * sizeof(HashEntry), h->stream));
  TableSet ts;
  std::memset(&ts, 0, sizeof(ts));
  for (int l = 0; l <= bits; ++l) {
    ts.tab[l] = h->tables.p + off[l]; ts.mask[l] = cap[l] - 1;
    g.tab[l] = ts.tab[l]; g.mask[l] = ts.mask[l];
  }
  if (getenv("LSGPU_CELLS_SPLIT")) {   // (dev: one launch per level, to time them)
    for (int l = 0; l <= bits; ++l)
      hipLaunchKernelGGL(k_cells_fill, dim3((nchunks + 255) / 256, 1), dim3(256), 0, h->stream, h->lane.scratch->keys_alt.p, h->bounds.p, nchunks, fine, bits, ts, l);
  } else
  hipLaunchKernelGGL(k_cells_fill, dim3((nchunks + 255) / 256, bits + 1), dim3(256), 0, h->stream, h->lane.scratch->keys_alt.p,
                     h->bounds.p, nchunks, fine, bits, ts, 0);
  HIPC(hipGetLastError());  // (no sync: align / knn follow on the same stream)
  h->grid = g;
  h->nr = nr;
  h->nchunks = nchunks;
  h->cone_ok = false; h->cone_pending = false;   // (no direction index of this reference yet)
  h->cone_zeta_lo = hg->zeta_lo; h->cone_zeta_hi = hg->zeta_hi; h->cone_origin_inside = hg->origin_inside != 0;
  std::memset(&h->info, 0, sizeof(h->info));
  h->info.n_reference = nr;
  h->info.bits_per_axis = bits;
  h->info.fine_bits = fine;
  h->info.cell_size = h0;
  h->info.n_chunks = nchunks;
  for (int l = 0; l <= bits; ++l) h->info.cells[l] = ncell[l];
  h->info.table_bytes = total * sizeof(HashEntry);
  return LSGPU_OK;
}

extern "C" {

int lsgpu_icp_get_reference_mean(lsgpu_icp* h, float mean[3]) {
  if (!h || !mean) return LSGPU_BAD_ARG;
  if (h->nr <= 0) return LSGPU_BAD_ARG;
  std::memcpy(mean, h->mean, 3 * sizeof(float));
  return LSGPU_OK;
}

int lsgpu_icp_set_reference(lsgpu_icp* h, const float* ref_xyz1, const float* ref_normals,
                            int64_t nr) {
  if (!h) return LSGPU_BAD_ARG;
  h->err.clear();
  if (!ref_xyz1 || nr <= 0 || nr > 0x7FFFFFF0ll) { h->err = "set_reference: empty or oversize cloud"; h->nr = 0; return LSGPU_BAD_ARG; }
  HIPC(hipSetDevice(h->device));
  int rc = ref_build_front(h, ref_xyz1, ref_normals, nr);
  if (!rc) rc = ref_build_back(h, nr);
  // the direction index for the settled launches (after k_cells_fill: its sort reuses the Morton keys' buffers)
  return rc ? rc : build_cone_index(h);
}

int lsgpu_comm_get_unique_id(void* id) {
  if (!id) return LSGPU_BAD_ARG;
  RcclApi* api = rccl_api();
  if (!api) return LSGPU_HIP_ERROR;
  ncclUniqueId u;
  if (api->GetUniqueId(&u) != ncclSuccess) return LSGPU_HIP_ERROR;
  static_assert(sizeof(u) == LSGPU_COMM_ID_BYTES, "unique id size");
  std::memcpy(id, &u, sizeof(u));
  return LSGPU_OK;
}

int lsgpu_icp_comm_init(lsgpu_icp* h, int rank, int nranks, const void* id) {
  if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks) return LSGPU_BAD_ARG;
  h->err.clear();
  RcclApi* api = rccl_api();
  ModuleSet m = module_set(h);
  m.f.comm = true;   // (the handle as it would be behind this call)
  if (m.ask(modules::kCommInit) != LSGPU_OK) { h->err = m.err; return LSGPU_BAD_CONFIG; }
  if (!api) { h->err = "librccl.so.1 could not be loaded"; return LSGPU_HIP_ERROR; }
  HIPC(hipSetDevice(h->device));
  if (h->comm) { (void)api->CommDestroy(h->comm); h->comm = nullptr; }
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  HIPC(h->comm_tmp.reserve(4));  // entry handshake of every align (allocated here: the handshake itself must not fail locally)
  RCCLC(api->CommInitRank(&h->comm, nranks, u, rank));
  h->comm_rank = rank; h->comm_size = nranks;
  return LSGPU_OK;
}

int lsgpu_icp_get_policy_info(lsgpu_icp* h, lsgpu_policy_info* out) {
  if (!h || !out) return LSGPU_BAD_ARG;
  std::memset(out, 0, sizeof(*out));
  out->index_rest = h->index_rest; out->pay_voxel_us = h->pay_voxel_us; out->pay_index_us = h->pay_index_us;
  out->ssn_sort_fallbacks = h->ssn_sort_fallbacks; out->ssn_calls = h->ssn_calls;
  return LSGPU_OK;
}

int lsgpu_icp_get_info(lsgpu_icp* h, lsgpu_icp_info* out) {
  if (!h || !out || h->nr <= 0) return LSGPU_BAD_ARG;
  *out = h->info;
  return LSGPU_OK;
}

int lsgpu_knn(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16], int32_t* ids,
              float* d2) {
  if (!h) return LSGPU_BAD_ARG;
  h->err.clear();
  if (h->nr <= 0) { h->err = "knn: no reference set"; return LSGPU_BAD_ARG; }
  if (nq == 0) return LSGPU_OK;
  if (!query_xyz1 || !ids || !d2 || nq < 0 || nq > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const Mat34 Tm = to_mat34(T ? T : I);
  // the transform is applied inside the search kernels; sorting uses the raw coordinates
  const Mat34 Id = to_mat34(I);
  int rc = prepare_queries(h, query_xyz1, nq, Id);
  if (rc) return rc;
  const bool maxd = matcher_max_d2(h) < INFINITY;   // KDTreeMatcher maxDist: the bounded k-best search with k = 1
  if (maxd) {
    rc = run_knn_k(h, 1, Tm, nullptr, true, false);
    if (rc) return rc;
  }
  policy::Iteration probe;   // a seeded, uncapped, wide search outside any loop
  probe.seed = true; probe.capped = false; probe.wide = true;
  h->pol.begin_align(false, false, false, 0.f);
  if (!maxd) rc = run_knn(h, Tm, nullptr, probe, false);
  if (rc) return rc;
  const bool dev_out = is_device_ptr(ids);
  int* ids_o = ids; float* d2_o = d2;
  if (!dev_out) {
    HIPC(h->ids_io.reserve(nq)); HIPC(h->d2_io.reserve(nq));
    ids_o = h->ids_io.p; d2_o = h->d2_io.p;
  }
  if (maxd)
    hipLaunchKernelGGL(k_knnk_unpermute, dim3(nblk(nq)), dim3(256), 0, h->stream, h->rdq.p, (int)nq, 1, h->kmatch.p,
                       h->kd2.p, h->pts.p, ids_o, d2_o);
  else
    hipLaunchKernelGGL(k_knn_unpermute, dim3(nblk(nq)), dim3(256), 0, h->stream, h->rdq.p, (int)nq,
                       h->ids.p, h->d2.p, h->pts.p, ids_o, d2_o);
  HIPC(hipGetLastError());
  if (!dev_out) {
    HIPC(hipMemcpyAsync(ids, ids_o, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipMemcpyAsync(d2, d2_o, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_knn_k(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16], int k, int32_t* ids, float* d2) {
  if (!h) return LSGPU_BAD_ARG;
  h->err.clear();
  if (h->nr <= 0) { h->err = "knn_k: no reference set"; return LSGPU_BAD_ARG; }
  if (k < 1 || k > LSGPU_MATCHER_KNN_MAX) { h->err = "knn_k: k must be in [1, 8]"; return LSGPU_BAD_ARG; }
  if (h->nr < k) { h->err = "knn_k: the reference has fewer points than k"; return LSGPU_BAD_ARG; }
  if (nq == 0) return LSGPU_OK;
  if (!query_xyz1 || !ids || !d2 || nq < 0 || nq > 0x7FFFFFF0ll / k) {
    if (nq > 0x7FFFFFF0ll / k) h->err = "knn_k: k x nq exceeds the 32-bit pair count";
    return LSGPU_BAD_ARG;
  }
  HIPC(hipSetDevice(h->device));
  float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const Mat34 Tm = to_mat34(T ? T : I);
  int rc = prepare_queries(h, query_xyz1, nq, to_mat34(I));   // (the transform is applied inside the search kernels)
  if (rc) return rc;
  rc = run_knn_k(h, k, Tm, nullptr, true, false);
  if (rc) return rc;
  const int64_t np = (int64_t)k * nq;
  const bool dev_out = is_device_ptr(ids);
  int* ids_o = ids; float* d2_o = d2;
  if (!dev_out) {
    HIPC(h->ids_io.reserve(np)); HIPC(h->d2_io.reserve(np));
    ids_o = h->ids_io.p; d2_o = h->d2_io.p;
  }
  hipLaunchKernelGGL(k_knnk_unpermute, dim3(nblk(np)), dim3(256), 0, h->stream, h->rdq.p, (int)np, k, h->kmatch.p,
                     h->kd2.p, h->pts.p, ids_o, d2_o);
  HIPC(hipGetLastError());
  if (!dev_out) {
    HIPC(hipMemcpyAsync(ids, ids_o, (size_t)np * 4, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipMemcpyAsync(d2, d2_o, (size_t)np * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_trim_limit(lsgpu_icp* h, const float* d2, int64_t n, float ratio, float* limit) {
  if (!h || !limit) return LSGPU_BAD_ARG;
  h->err.clear();
  if (n <= 0 || !d2) return LSGPU_NO_CONVERGENCE;  // "no outlier to filter"
  if (n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  int rc = ensure_loop_buffers(h, 1);
  if (rc) return rc;
  const float* src = nullptr;
  if ((rc = stage_in(h, d2, (size_t)n, h->d2_io, &src))) return rc;
  // ratio > 0: the rank over the FINITE distances, taken on the device (Matches::getDistsQuantile skips invalid matches; the
  // host's rank argument is not read on that route).  A ratio that is not positive asks for rank 0 whatever the count: the
  // host-side rank, as before.
  if (ratio > 0.f) rc = run_select(h, src, (int)n, 0u, true, nullptr, false, false, 3, ratio, false);
  else rc = run_select(h, src, (int)n, trim_rank(n, ratio), true, nullptr, false, false);
  if (rc) return rc;
  hipLaunchKernelGGL(k_limit_out, dim3(1), dim3(256), 0, h->stream, h->hist.p + 2 * kHistBins,
                     h->sel.p + 2, h->limit_dev.p);
  HIPC(hipMemcpyAsync(&h->pin->limit, h->limit_dev.p, 4, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  *limit = h->pin->limit;
  if (*limit == INFINITY) { h->err = "trim_limit: no finite distance (no outlier to filter)"; return LSGPU_NO_CONVERGENCE; }
  return LSGPU_OK;
}

// the stand-alone accumulation of either minimizer (lsgpu_normal_eq / lsgpu_point_to_point): 29 sums of the pairs with
// d2 <= limit, ids indexing the reference as given to set_reference
extern "C++" template <int MIN>
static int stand_alone_sums(lsgpu_icp* h, const char* what, const float* query_xyz1, int64_t nq, const float T[16],
                            const int32_t* ids, const float* d2, float limit, double out[29]) {
  if (!h || !out) return LSGPU_BAD_ARG;
  h->err.clear();
  if (h->nr <= 0) { h->err = std::string(what) + ": no reference set"; return LSGPU_BAD_ARG; }
  if (nq <= 0 || !query_xyz1 || !ids || !d2 || nq > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  int rc = ensure_loop_buffers(h, nq);
  if (rc) return rc;
  const float4* q = nullptr;
  rc = stage_points(h, query_xyz1, nq, h->q_in, &q);
  if (rc) return rc;
  const int* idp = nullptr; const float* dp = nullptr;
  if ((rc = stage_in(h, ids, (size_t)nq, h->ids_io, &idp))) return rc;
  if ((rc = stage_in(h, d2, (size_t)nq, h->d2_io, &dp))) return rc;
  float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const Mat34 Tm = to_mat34(T ? T : I);
  const int nb = std::min(kNeBlocks, nblk(nq));
  if constexpr (MIN == kPointToPlane4Dof || MIN == kPointToPlane2D) {   // (lsgpu_icp_set_motion refuses such a handle the weighted filter)
    hipLaunchKernelGGL((k_normal_eq<true, false, MIN>), dim3(nb), dim3(256), 0, h->stream, q, (int)nq, Tm,
                       idp, dp, h->pts.p, h->nrm.p, h->ref_inv.p,
                       (const uint32_t*)nullptr, (const SelState*)nullptr, limit, (float*)nullptr, h->ne_partials.p,
                       robust::Params{}, 1.f);
  } else if (h->mods.robust_on) {
    // RobustOutlierFilter: the pairs' weights go into the sums; the scale is the MAD of the distances given (host twin)
    const robust::Params rp = robust::params(h->mods.robust);
    if (rp.plane && !h->have_normals) { h->err = std::string(what) + ": RobustOutlierFilter distanceType point2plane needs reference normals"; return LSGPU_BAD_CONFIG; }
    float scale = 1.f, med = 0.f;
    if (rp.mad) {
      std::vector<float> hd((size_t)nq);
      HIPC(hipMemcpyAsync(hd.data(), dp, (size_t)nq * 4, hipMemcpyDeviceToHost, h->stream));
      HIPC(hipStreamSynchronize(h->stream));
      if (lsgpu_robust_scale(hd.data(), nq, &med, &scale) != LSGPU_OK || !(scale > 0.f)) {
        h->err = std::string(what) + ": RobustOutlierFilter has no valid match or a MAD scale of 0";
        return LSGPU_NO_CONVERGENCE;
      }
    }
    hipLaunchKernelGGL((k_normal_eq<true, false, MIN, true>), dim3(nb), dim3(256), 0, h->stream, q, (int)nq, Tm,
                       idp, dp, h->pts.p, (MIN == kPointToPoint && !rp.plane) ? (const float4*)nullptr : h->nrm.p, h->ref_inv.p,
                       (const uint32_t*)nullptr, (const SelState*)nullptr, limit, (float*)nullptr, h->ne_partials.p, rp, scale);
  } else {
    hipLaunchKernelGGL((k_normal_eq<true, false, MIN>), dim3(nb), dim3(256), 0, h->stream, q, (int)nq, Tm,
                       idp, dp, h->pts.p, MIN == kPointToPoint ? (const float4*)nullptr : h->nrm.p, h->ref_inv.p,
                       (const uint32_t*)nullptr, (const SelState*)nullptr, limit, (float*)nullptr, h->ne_partials.p,
                       robust::Params{}, 1.f);
  }
  hipLaunchKernelGGL(k_ne_final, dim3(1), dim3(1024), 0, h->stream, h->ne_partials.p, nb, h->ne_out.p);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h->pin->ne, h->ne_out.p, kNe * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  std::memcpy(out, h->pin->ne, kNe * sizeof(double));
  return LSGPU_OK;
}

int lsgpu_normal_eq(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16],
                    const int32_t* ids, const float* d2, float limit, double out[29]) {
  // (a force2D / force4DOF handle: the sums of its mode -- force2D forms b with the planar residual)
  if (h && h->mods.dof() == LSGPU_MOTION_DOF_3) return stand_alone_sums<kPointToPlane2D>(h, "normal_eq", query_xyz1, nq, T, ids, d2, limit, out);
  if (h && h->mods.dof() == LSGPU_MOTION_DOF_4) return stand_alone_sums<kPointToPlane4Dof>(h, "normal_eq", query_xyz1, nq, T, ids, d2, limit, out);
  return stand_alone_sums<kPointToPlane>(h, "normal_eq", query_xyz1, nq, T, ids, d2, limit, out);
}

int lsgpu_point_to_point(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16],
                         const int32_t* ids, const float* d2, float limit, double out[29]) {
  return stand_alone_sums<kPointToPoint>(h, "point_to_point", query_xyz1, nq, T, ids, d2, limit, out);
}

// The covariance sums of the pairs (q, ids, d2: device pointers, the caller's order, ids indexing the reference as given)
// into h->pin->cov, on return.  lsgpu_point_to_plane_cov and the pass after the loop both end here: same grid, same order.
static int cov_sums(lsgpu_icp* h, const float4* q, int64_t nq, const Mat34& Tm, const int* ids, const float* d2,
                                 float limit, const float dT[16]) {
  HIPC(h->cov_partials.reserve((size_t)kNeBlocksMax * kCovStride));
  HIPC(h->cov_out.reserve(kCovStride));
  float wt[6];
  cov::step_params(dT, wt);
  CovStep step;
  for (int d = 0; d < 3; ++d) { step.w[d] = wt[d]; step.t[d] = wt[3 + d]; }
  const int nb = std::min(kNeBlocks, nblk(nq));
  const float lo2 = h->cfg.outlier_min_dist * h->cfg.outlier_min_dist;   // MinDistOutlierFilter (0: none), as the loop's ChainArgs
  hipLaunchKernelGGL((k_cov<true>), dim3(nb), dim3(256), 0, h->stream, q, (int)nq, Tm, ids, d2, h->pts.p, h->nrm.p,
                     h->ref_inv.p, (uint32_t)h->nr, limit, lo2, step, h->cov_partials.p);
  hipLaunchKernelGGL(k_cov_final, dim3(1), dim3(1024), 0, h->stream, h->cov_partials.p, nb, h->cov_out.p);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h->pin->cov, h->cov_out.p, kCov * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_point_to_plane_cov(lsgpu_icp* h, const float* query_xyz1, int64_t nq, const float T[16], const int32_t* ids,
                             const float* d2, float limit, const float dT[16], double out[44]) {
  if (!h || !out) return LSGPU_BAD_ARG;
  h->err.clear();
  if (h->nr <= 0) { h->err = "point_to_plane_cov: no reference set"; return LSGPU_BAD_ARG; }
  if (!h->have_normals) { h->err = "point_to_plane_cov: the reference has no normals"; return LSGPU_BAD_ARG; }
  if (nq <= 0 || !query_xyz1 || !ids || !d2 || nq > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  int rc = ensure_loop_buffers(h, nq);
  if (rc) return rc;
  const float4* q = nullptr;
  rc = stage_points(h, query_xyz1, nq, h->q_in, &q);
  if (rc) return rc;
  const int* idp = nullptr; const float* dp = nullptr;
  if ((rc = stage_in(h, ids, (size_t)nq, h->ids_io, &idp))) return rc;
  if ((rc = stage_in(h, d2, (size_t)nq, h->d2_io, &dp))) return rc;
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  rc = cov_sums(h, q, nq, to_mat34(T ? T : I), idp, dp, limit, dT ? dT : I);
  if (rc) return rc;
  std::memcpy(out, h->pin->cov, kCov * sizeof(double));
  return LSGPU_OK;
}

int lsgpu_transform_points(lsgpu_icp* h, const float T[16], const float* xyz1, int64_t n,
                           float* out) {
  if (!h || !T || !out) return LSGPU_BAD_ARG;
  h->err.clear();
  if (n == 0) return LSGPU_OK;
  if (!xyz1 || n < 0) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr;
  int rc = stage_points(h, xyz1, n, h->q_in, &src);
  if (rc) return rc;
  const bool dev_out = is_device_ptr(out);
  float4* dst = reinterpret_cast<float4*>(out);
  if (!dev_out) { HIPC(h->rdq.reserve(n)); dst = h->rdq.p; }
  hipLaunchKernelGGL(k_transform, dim3(nblk(n)), dim3(256), 0, h->stream, src, n, to_mat34(T), dst);
  HIPC(hipGetLastError());
  if (!dev_out) HIPC(hipMemcpyAsync(out, dst, (size_t)n * 16, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_rotate_descriptors(lsgpu_icp* h, const float T[16], const float* desc3, int64_t n, float* out) {
  if (!h || !T) return LSGPU_BAD_ARG;
  h->err.clear();
  if (n == 0) return LSGPU_OK;
  if (!desc3 || !out || n < 0 || n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  if (!lsgpu_check_rigid(T)) { h->err = "rotate_descriptors: the matrix is not rigid"; return LSGPU_BAD_ARG; }   // TransformationError upstream
  HIPC(hipSetDevice(h->device));
  const float* src = nullptr;
  const int rc = stage_in(h, desc3, (size_t)3 * n, h->flt_nrm, &src);
  if (rc) return rc;
  const bool dev_out = is_device_ptr(out);
  float* dst = out;
  if (!dev_out) { HIPC(h->ssn_box_normal.reserve(3 * n)); dst = h->ssn_box_normal.p; }
  hipLaunchKernelGGL(k_rotate3, dim3(nblk(n)), dim3(256), 0, h->stream, src, n, to_mat34(T), dst);
  HIPC(hipGetLastError());
  if (!dev_out) HIPC(hipMemcpyAsync(out, dst, (size_t)n * 12, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

}  // extern "C"

// prefix sum of n uint32 on the handle's current stream (lsgpu_scan.hip.h; in == out is fine)
static int scan_u32(lsgpu_icp* h, const uint32_t* in, uint32_t* out, size_t n, bool inclusive, bool nonzero) {
  if (n == 0) return LSGPU_OK;
  const int nb = (int)((n + kScanTile - 1) / kScanTile);
  uint32_t* sums = nullptr;
  if (nb > 1) {
    HIPC(h->lane.scratch->sort_tmp.reserve((size_t)nb * sizeof(uint32_t)));
    sums = reinterpret_cast<uint32_t*>(h->lane.scratch->sort_tmp.p);
    if (nonzero) hipLaunchKernelGGL(k_scan_sums<true>, dim3(nb), dim3(256), 0, h->lane.stream, in, n, sums);
    else hipLaunchKernelGGL(k_scan_sums<false>, dim3(nb), dim3(256), 0, h->lane.stream, in, n, sums);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, h->lane.stream, sums, nb);
  }
  if (nonzero) hipLaunchKernelGGL((k_scan_write<false, true>), dim3(nb), dim3(256), 0, h->lane.stream, in, out, n, (const uint32_t*)sums);   // (exclusive: the one use)
  else if (inclusive) hipLaunchKernelGGL((k_scan_write<true, false>), dim3(nb), dim3(256), 0, h->lane.stream, in, out, n, (const uint32_t*)sums);
  else hipLaunchKernelGGL((k_scan_write<false, false>), dim3(nb), dim3(256), 0, h->lane.stream, in, out, n, (const uint32_t*)sums);
  HIPC(hipGetLastError());
  return LSGPU_OK;
}

// Up to `kmax` draws of the library stream -> h->ssn_draws, speculatively: the stream stays locked until
// the caller commits the number the sequential filter would have consumed (DrawStream::commit).
static int upload_draws_begin(lsgpu_icp* h, int64_t seed, size_t kmax) {
  HIPC(h->draws_pinned.reserve(kmax + 1));
  HIPC(h->ssn_draws.reserve(kmax + 1));
  DrawStream::global().begin(seed, kmax, h->draws_pinned.p);
  if (kmax) {
    const hipError_t e = hipMemcpyAsync(h->ssn_draws.p, h->draws_pinned.p, kmax * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) { DrawStream::global().commit(0); HIPC(e); }
  }
  return LSGPU_OK;
}

// The same, produced AHEAD on a helper thread while the calling thread enqueues the kernels that come before the draws
// are needed (the ~1.3 ns a draw costs used to sit on the stream's critical path: the device idled ~0.3 ms per 200 k
// points in front of k_ssn_select and again in front of k_draw_select, profiles/r03_bench.stats.txt).  begin() locks
// the stream and starts the helper, ready() joins it and enqueues the H2D of all draws on the handle's stream, the
// destructor consumes `used` draws -- what the sequential filters would have made -- and unlocks.  One DrawAhead can
// serve consecutive filters: lsgpu_icp_compute draws for the reference filter and the reading filter in one go, the
// reading filter's draws start where the reference filter's end (known once its kernels ran).
struct DrawAhead {
  lsgpu_icp* h = nullptr;
  size_t kmax = 0, used = 0, kfirst = 0;
  bool open = false, waited = false, unlocked_early = false;
  hipError_t upload_err = hipSuccess;
  std::atomic<int> first_sent{0};   // the first `kfirst` draws are on their way to the device (their own event)
  std::thread worker;
  DrawAhead() = default;
  DrawAhead(const DrawAhead&) = delete;
  DrawAhead& operator=(const DrawAhead&) = delete;
  // (k_first: draws [0, k_first) are sent off and can be waited for -- ready(k_first) -- before the rest exists)
  int begin(lsgpu_icp* hh, int64_t seed, size_t k, size_t k_first = 0) {
    h = hh; kmax = k; kfirst = (k_first && k_first < k) ? k_first : 0;
    first_sent.store(0, std::memory_order_relaxed);
    HIPC(h->draws_pinned.reserve(kmax + 1));
    HIPC(h->ssn_draws.reserve(kmax + 1));
    HIPC(h->draw_stream.ensure());
    HIPC(h->draws_done.ensure(hipEventDisableTiming));
    HIPC(h->draws_first_done.ensure(hipEventDisableTiming));
    order_after_tail(h, h->draw_stream);
    DrawStream::global().lock(seed);
    open = true;
    if (kmax) {
      // the helper produces the draws and sends them off on a stream of their own right away: the H2D (8 MB for two
      // 1 M-point clouds) used to sit on the filter's stream in front of k_ssn_select, 0.18 ms of idle device
      lsgpu_icp* hh2 = h;
      auto produce = [hh2, k, this] {
        hipError_t e = hipSetDevice(hh2->device);
        const size_t kf = kfirst;
        if (kf) {
          // the first filter's share leaves as soon as it exists; the rest is still being produced
          DrawStream::global().generate(k, hh2->draws_pinned.p, kf, [&] {
            if (e == hipSuccess) e = hipMemcpyAsync(hh2->ssn_draws.p, hh2->draws_pinned.p, kf * sizeof(float), hipMemcpyHostToDevice, hh2->draw_stream);
            if (e == hipSuccess) e = hipEventRecord(hh2->draws_first_done, hh2->draw_stream);
            upload_err = e;
            first_sent.store(1, std::memory_order_release);
          });
          if (e == hipSuccess) e = hipMemcpyAsync(hh2->ssn_draws.p + kf, hh2->draws_pinned.p + kf, (k - kf) * sizeof(float), hipMemcpyHostToDevice, hh2->draw_stream);
        } else {
          DrawStream::global().generate(k, hh2->draws_pinned.p);
          if (e == hipSuccess) e = hipMemcpyAsync(hh2->ssn_draws.p, hh2->draws_pinned.p, k * sizeof(float), hipMemcpyHostToDevice, hh2->draw_stream);
        }
        if (e == hipSuccess) e = hipEventRecord(hh2->draws_done, hh2->draw_stream);
        upload_err = e;
        first_sent.store(1, std::memory_order_release);
      };
      try {
        worker = std::thread(produce);
      } catch (const std::system_error&) {   // no thread to be had: produce the draws here
        produce();
      }
    }
    return LSGPU_OK;
  }
  int ready(size_t upto = ~(size_t)0) {   // the stream the caller enqueues on (h->lane.stream) waits for the draws [0, upto)
    if (kmax && kfirst && upto <= kfirst) {   // the first part has its own event: no need for the rest to exist yet
      while (!first_sent.load(std::memory_order_acquire)) std::this_thread::yield();
      if (upload_err != hipSuccess) { (void)hipGetLastError(); HIPC(upload_err); }
      HIPC(hipStreamWaitEvent(h->lane.stream, h->draws_first_done, 0));
      return LSGPU_OK;
    }
    if (worker.joinable()) worker.join();
    if (kmax) {
      if (upload_err != hipSuccess) { (void)hipGetLastError(); HIPC(upload_err); }
      HIPC(hipStreamWaitEvent(h->lane.stream, h->draws_done, 0));
      waited = true;
    }
    return LSGPU_OK;
  }
  // The number of draws the filters will have consumed is known: consume them and unlock NOW -- the values are
  // already on their way to the device, the filters that still have to run only read them there.  (The process-wide
  // stream used to stay locked from the first filter to the end of the last, i.e. across the whole grid build and its
  // host round trip: compute calls on other handles -- other robots' tracks, a loop-closure ICP -- took turns there.)
  void commit_now(size_t total) {
    if (worker.joinable()) worker.join();
    if (open) DrawStream::global().commit(std::min(total, kmax));
    if (open) unlocked_early = true;
    open = false;
  }
  void finish() {   // consume + unlock now (the stream must not stay locked while the ICP loop runs)
    if (worker.joinable()) worker.join();
    if (open) DrawStream::global().commit(std::min(used, kmax));
    if ((open || unlocked_early) && kmax && !waited && h->draw_stream) (void)hipStreamSynchronize(h->draw_stream);   // (nobody waited for the upload: the staging buffer must be free on return)
    open = false; unlocked_early = false;
  }
  ~DrawAhead() { finish(); }
};

// totals of two exclusive scans (last scanned value + last input) -> four pinned words, behind the scans ...
// (`extra`: up to two more ranges that travel with them)
static int scan_totals_enqueue(lsgpu_icp* h, const uint32_t* in_a, const uint32_t* sc_a, size_t na,
                               const uint32_t* in_b, const uint32_t* sc_b, size_t nb,
                               const void* extra_src = nullptr, void* extra_dst = nullptr, size_t extra_bytes = 0) {
  uint32_t* hp = h->pin->totals[h->lane.totals_row];
  hp[0] = hp[1] = hp[2] = hp[3] = 0;
  ToHost c{}; int used = 0;
  if (in_a) {
    to_host_add(&c, &used, in_a + (na - 1), hp, 4);
    to_host_add(&c, &used, sc_a + (na - 1), hp + 1, 4);
  }
  to_host_add(&c, &used, in_b + (nb - 1), hp + 2, 4);
  to_host_add(&c, &used, sc_b + (nb - 1), hp + 3, 4);
  if (extra_src) to_host_add(&c, &used, extra_src, extra_dst, extra_bytes);
  hipLaunchKernelGGL(k_to_host, dim3(1), dim3(64), 0, h->lane.stream, c);
  HIPC(hipGetLastError());
  return LSGPU_OK;
}
// ... and the host's wait for them (synchronises the current stream)
static int scan_totals_wait(lsgpu_icp* h, uint32_t* tot_a, uint32_t* tot_b, bool b_flags = false) {
  const uint32_t* hp = h->pin->totals[h->lane.totals_row];
  HIPC(hipStreamSynchronize(h->lane.stream));
  *tot_a = hp[0] + hp[1];
  *tot_b = (b_flags ? (hp[2] ? 1u : 0u) : hp[2]) + hp[3];   // (b_flags: the scanned words are flags, any non-zero word counts 1)
  return LSGPU_OK;
}
static int scan_totals(lsgpu_icp* h, const uint32_t* in_a, const uint32_t* sc_a, size_t na,
                       const uint32_t* in_b, const uint32_t* sc_b, size_t nb, uint32_t* tot_a, uint32_t* tot_b,
                       const void* extra_src = nullptr, void* extra_dst = nullptr, size_t extra_bytes = 0, bool b_flags = false) {
  const int rc = scan_totals_enqueue(h, in_a, sc_a, na, in_b, sc_b, nb, extra_src, extra_dst, extra_bytes);
  return rc ? rc : scan_totals_wait(h, tot_a, tot_b, b_flags);
}

// The filters' compaction on the current stream: the keep flags in h->ssn_keep -> their exclusive scan in h->ssn_out_pos ->
// the kept points of src at the front of dst, order preserved, and the number kept on its way to the totals words ...
static int compact_kept_enqueue(lsgpu_icp* h, const float4* src, int64_t n, float4* dst) {
  const int rc = scan_u32(h, h->ssn_keep.p, h->ssn_out_pos.p, (size_t)n);
  if (rc) return rc;
  hipLaunchKernelGGL(k_compact_points, dim3(nblk(n)), dim3(256), 0, h->lane.stream, src, (int)n, h->ssn_keep.p, h->ssn_out_pos.p, dst);
  HIPC(hipGetLastError());
  return scan_totals_enqueue(h, nullptr, nullptr, 0, h->ssn_keep.p, h->ssn_out_pos.p, (size_t)n);
}
// ... and the host's wait for that number (lsgpu_icp_compute puts the rest of the grid build on the other stream in between)
static int compact_kept_wait(lsgpu_icp* h, int64_t* kept) {
  uint32_t unused = 0, k = 0;
  const int rc = scan_totals_wait(h, &unused, &k);
  if (rc) return rc;
  *kept = k;
  return LSGPU_OK;
}
static int compact_kept(lsgpu_icp* h, const float4* src, int64_t n, float4* dst, int64_t* kept) {
  const int rc = compact_kept_enqueue(h, src, n, dst);
  return rc ? rc : compact_kept_wait(h, kept);
}

// host twin of float_from_order_key (lsgpu_ssn.hip.h)
static float host_float_from_order_key(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// Minimum and maximum of a cloud on the device (n points, current stream; waits for it).  A NaN's ordered key lies beyond
// the infinities', so a cloud with any NaN or infinity has a bound that is not finite: the verdict is the caller's.
static int cloud_bounds(lsgpu_icp* h, const float4* src, int64_t n, float lo[3], float hi[3]) {
  HIPC(h->ssn_bb.reserve(8));
  HIPC(hipMemsetAsync(h->ssn_bb.p, 0xFF, 12, h->lane.stream));
  HIPC(hipMemsetAsync(h->ssn_bb.p + 3, 0, 12, h->lane.stream));
  hipLaunchKernelGGL(k_ssn_bounds, dim3(std::min(nblk(n), 256)), dim3(256), 0, h->lane.stream, src, (int)n, h->ssn_bb.p);
  HIPC(hipMemcpyAsync(h->pin->bounds, h->ssn_bb.p, sizeof h->pin->bounds, hipMemcpyDeviceToHost, h->lane.stream));
  HIPC(hipStreamSynchronize(h->lane.stream));
  for (int d = 0; d < 3; ++d) { lo[d] = host_float_from_order_key(h->pin->bounds[d]); hi[d] = host_float_from_order_key(h->pin->bounds[3 + d]); }
  return LSGPU_OK;
}

// Where an entry point's kernels write a result of the caller's: into the caller's buffer if that is device memory, or
// else into a buffer of the handle, from which copy_back() sends the elements that count to the host.
template <class T>
struct OutStage {
  void* user = nullptr;
  T* p = nullptr;        // what the kernels write
  bool staged = false;
  void classify(void* out) { user = out; p = static_cast<T*>(out); staged = !is_device_ptr(out); }
  int open(lsgpu_icp* h, void* out, DevBuf<T>& buf, size_t room) {
    classify(out);
    if (staged) { HIPC(buf.reserve(room)); p = buf.p; }
    return LSGPU_OK;
  }
  // n elements of `from` (device) to the caller's buffer, wherever that is
  int send(lsgpu_icp* h, const T* from, size_t n) {
    if (n) HIPC(hipMemcpyAsync(user, from, n * sizeof(T), staged ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
    return LSGPU_OK;
  }
  int copy_back(lsgpu_icp* h, size_t n) { return staged ? send(h, p, n) : LSGPU_OK; }
};

// SamplingSurfaceNormal on device memory: src (n points) -> out_xyz1 / out_nrm (device, room for n)
// (`ahead`: draws begun by the caller, this filter's first at ahead->used; nullptr: the filter draws for itself)
static int ssn_device(lsgpu_icp* h, const float4* src, int64_t n, int knn, float ratio, int64_t seed,
                      float4* out_xyz1, float* out_nrm, int64_t* n_out, DrawAhead* ahead = nullptr, bool force_sort_levels = false) {
  *n_out = 0;
  if (!force_sort_levels) ++h->ssn_calls;
  DrawAhead own;
  if (!ahead) {   // at most one draw per point, produced while the levels below are enqueued and run
    const int rc0 = own.begin(h, seed, (size_t)n);
    if (rc0) return rc0;
    ahead = &own;
  }
  const size_t first_draw = ahead->used;
  int levels = 0;
  for (int64_t c = n; c > knn; c -= c / 2) ++levels;  // the largest child keeps count - count / 2 points
  const size_t nseg = (size_t)1 << levels;
  HIPC(h->ssn_seg_a.reserve(nseg));
  HIPC(h->ssn_seg_b.reserve(nseg));
  HIPC(h->ssn_seg_of.reserve(n));
  HIPC(h->ssn_box_pts.reserve(nseg));
  HIPC(h->ssn_box_base.reserve(nseg));
  HIPC(h->ssn_box_normal.reserve(3 * nseg));
  HIPC(h->ssn_keep.reserve(n));
  HIPC(h->ssn_out_pos.reserve(n));
  HIPC(h->ssn_bb.reserve(8));
  HIPC(h->lane.scratch->keys.reserve(n));
  HIPC(h->lane.scratch->vals.reserve(n));
  {   // the cloud's bounds and the root segment in one launch (k_ssn_bounds_root: a ticket that is zero between calls)
    const bool fresh = h->ssn_bounds_ws.cap == 0;
    HIPC(h->ssn_bounds_ws.reserve(8 + 6 * kSsnBoundsBlocks));
    if (fresh) HIPC(hipMemsetAsync(h->ssn_bounds_ws.p, 0, 8 * sizeof(uint32_t), h->stream));
    hipLaunchKernelGGL(k_ssn_bounds_root, dim3(std::min(nblk(n), kSsnBoundsBlocks)), dim3(256), 0, h->stream, src, (int)n, h->ssn_bounds_ws.p,
                       h->ssn_bb.p, h->ssn_seg_a.p);
  }
  SsnSeg* cur = h->ssn_seg_a.p;
  SsnSeg* nxt = h->ssn_seg_b.p;
  const uint32_t* idx = nullptr;
  const int* root_axis = nullptr;   // per root of the in-workgroup levels: the axis its order follows (segmented level sorts)
  // levels [0, glevels) with global passes; the rest inside one workgroup per segment (k_ssn_tree) once a segment holds
  // at most root_max points and log2(root_max / 8) levels to go
  int glevels = 0;
  // (one workgroup per root: 8192-point roots leave half the chip idle on a scan of a million points -- 128 roots, 248 us --
  // where 4096-point roots and one more global level take 50 us less; a three-scan sub-map has 383 roots of 8192)
  const int root_auto = n >= 200ll * 8192 ? 8192 : n >= 200ll * 4096 ? 4096 : 2048;
  const int root_max = tuning().ssn_root ? tuning().ssn_root : root_auto;
  int root_levels = 0;
  while ((8 << root_levels) < root_max) ++root_levels;
  {
    int64_t c = n;
    while (glevels < levels && !(c <= root_max && levels - glevels <= root_levels)) { c -= c / 2; ++glevels; }
  }
  // the sort-free levels hand SETS over (points in original-index order + a signature) to k_ssn_tree; the segmented
  // sorts (LSGPU_SSN_SORT_LEVELS, and the fallback below) hand it a sorted order
  const bool select_levels = !force_sort_levels && !tuning().ssn_sort_levels && glevels > 0;
  const uint32_t* root_sig = nullptr;   // per root of the in-workgroup levels: its signature (sort-free upper levels)
  if (select_levels) {
    // Sort-free upper levels (lsgpu_ssn_select.hip.h): a segment is a set + a signature, a level is the exact median in the
    // segment's total order (two 8-bit histogram passes over the range its points span + a per-segment selection among the
    // candidates left) and one stable partition: five launches per level, no sort.
    if (h->gs_plan_n != n || h->gs_plan_levels != glevels) {   // block tables: static for a cloud size
      // every level's number of blocks and first row (sizes of a level: c -> c - c / 2, c / 2)
      std::vector<uint32_t> sizes{(uint32_t)n}, next;
      h->gs_lvl_first.clear(); h->gs_lvl_blocks.clear();
      uint32_t rows = 0, segs = 0;
      for (int L = 0; L < glevels; ++L) {
        uint32_t fb = 0;
        next.clear();
        for (uint32_t c : sizes) {
          fb += (c + kGsTile - 1u) / kGsTile;
          next.push_back(c - c / 2u); next.push_back(c / 2u);
        }
        h->gs_lvl_first.push_back(rows); h->gs_lvl_blocks.push_back(fb);
        rows += fb; segs += (uint32_t)sizes.size();
        sizes.swap(next);
      }
      HIPC(h->gs_tab.reserve(rows)); HIPC(h->gs_sblk.reserve(segs));
      if (glevels <= kGsPlanLevels && ((size_t)1 << (glevels - 1)) <= kGsPlanSegs) {   // the rows themselves: on the device
        GsPlanArgs pa{};
        for (int L = 0; L < glevels; ++L) pa.first[L] = h->gs_lvl_first[L];
        hipLaunchKernelGGL(k_gs_plan, dim3(glevels), dim3(1024), 0, h->stream, (uint32_t)n, pa, h->gs_tab.p, h->gs_sblk.p);
        HIPC(hipGetLastError());
      } else {                                            // (more than 8192 segments in a level: 67 M points)
        std::vector<GsBlock> tab;
        std::vector<GsSegBlocks> sblk;
        std::vector<std::pair<uint32_t, uint32_t>> segsz{{0u, (uint32_t)n}};
        for (int L = 0; L < glevels; ++L) {
          uint32_t fb = 0;
          std::vector<std::pair<uint32_t, uint32_t>> nx;
          for (uint32_t sidx = 0; sidx < segsz.size(); ++sidx) {
            const uint32_t st = segsz[sidx].first, c = segsz[sidx].second;
            const uint32_t nb = (c + kGsTile - 1u) / kGsTile;
            sblk.push_back(GsSegBlocks{fb, nb, st, c});
            for (uint32_t k = 0; k < nb; ++k)
              tab.push_back(GsBlock{st + k * kGsTile, std::min(kGsTile, c - k * kGsTile), sidx, st, c, fb, nb, 0u});
            fb += nb;
            const uint32_t left = c - c / 2u;
            nx.push_back({st, left}); nx.push_back({st + left, c - left});
          }
          segsz.swap(nx);
        }
        // (pageable source: the copy returns when the staging is done)
        HIPC(hipMemcpyAsync(h->gs_tab.p, tab.data(), tab.size() * sizeof(GsBlock), hipMemcpyHostToDevice, h->stream));
        HIPC(hipMemcpyAsync(h->gs_sblk.p, sblk.data(), sblk.size() * sizeof(GsSegBlocks), hipMemcpyHostToDevice, h->stream));
        HIPC(hipStreamSynchronize(h->stream));
      }
      h->gs_plan_n = n; h->gs_plan_levels = glevels;
    }
    const size_t nseg_g = (size_t)1 << glevels;
    int cap = 1;
    for (uint32_t v : h->gs_lvl_blocks) cap = std::max(cap, (int)v);
    for (auto& bf : h->gs_e) HIPC(bf.reserve(n));
    for (auto& bf : h->gs_k) HIPC(bf.reserve(n));
    HIPC(h->gs_hist.reserve(4 * 256 * (nseg_g + 1))); HIPC(h->gs_median.reserve(nseg_g)); HIPC(h->gs_cand_n.reserve(2 * nseg_g + 2));
    const size_t cand_room = std::max<size_t>(nseg_g / 2, 1) * kGsCandRoom;
    HIPC(h->gs_cand.reserve(cand_room)); HIPC(h->gs_cand_blk.reserve(cand_room));
    HIPC(h->gs_cl.reserve((size_t)2 * cap)); HIPC(h->gs_err.reserve(8)); HIPC(h->gs_rng.reserve(2 * nseg_g + 2));
    HIPC(h->ssn_axis_a.reserve(nseg_g)); HIPC(h->ssn_axis_b.reserve(nseg_g));
    uint32_t* cand_n[2] = {h->gs_cand_n.p, h->gs_cand_n.p + nseg_g + 1};
    uint32_t* sig_cur = reinterpret_cast<uint32_t*>(h->ssn_axis_a.p);
    uint32_t* sig_nxt = reinterpret_cast<uint32_t*>(h->ssn_axis_b.p);
    GsSet in, out;
    in.e = h->gs_e[0].p; out.e = h->gs_e[1].p;
    for (int d = 0; d < 3; ++d) { in.k[d] = h->gs_k[d].p; out.k[d] = h->gs_k[3 + d].p; }
    uint2* rng_cur = h->gs_rng.p;
    uint2* rng_nxt = h->gs_rng.p + nseg_g + 1;
    // per segment two 256-bin histograms; a level zeroes its children's (the root's: here)
    uint32_t* gh1[2] = {h->gs_hist.p, h->gs_hist.p + 256 * (nseg_g + 1)};
    uint32_t* gh2[2] = {h->gs_hist.p + 2 * 256 * (nseg_g + 1), h->gs_hist.p + 3 * 256 * (nseg_g + 1)};
    hipLaunchKernelGGL(k_gs_init, dim3(nblk(n)), dim3(256), 0, h->stream, src, (int)n, in, out.e, (const SsnSeg*)cur, (const uint32_t*)h->ssn_bb.p, rng_cur,
                       gh1[0], gh2[0], cand_n[0], sig_cur, h->gs_err.p);
    for (int L = 0; L < glevels; ++L) {
      const int ns = 1 << L, nb = (int)h->gs_lvl_blocks[L], par = L & 1;
      const GsBlock* tab = h->gs_tab.p + h->gs_lvl_first[L];
      const GsSegBlocks* sblk = h->gs_sblk.p + (ns - 1);
      hipLaunchKernelGGL(k_gs_hist<1>, dim3(nb), dim3(256), 0, h->stream, tab, cur, (const uint2*)rng_cur, in, gh1[par], gh2[par], h->gs_err.p);
      hipLaunchKernelGGL(k_gs_hist<2>, dim3(nb), dim3(256), 0, h->stream, tab, cur, (const uint2*)rng_cur, in, gh1[par], gh2[par], h->gs_err.p);
      // (candidates per segment: the list's room shared out among the level's segments -- kGsCandRoom at the last level, i.e.
      //  as many as the segment has points, and so at every level above it: a wall square to a frame axis puts 12 000 points
      //  of a sub-map into one bin of the first levels, a lattice a fifth of a segment)
      const uint32_t lvl_cap = (uint32_t)std::min<size_t>(cand_room / (size_t)ns, (size_t)1 << 22);
      hipLaunchKernelGGL(k_gs_collect, dim3(nb), dim3(256), 0, h->stream, tab, cur, (const uint2*)rng_cur, (const uint32_t*)sig_cur, in,
                         (const uint32_t*)gh1[par], (const uint32_t*)gh2[par], cand_n[par], h->gs_cand.p, h->gs_cand_blk.p, lvl_cap, h->gs_cl.p);
      hipLaunchKernelGGL(k_gs_select, dim3(ns), dim3(L < 3 ? 1024 : 256), 0, h->stream, sblk, src, cur, (const uint32_t*)sig_cur, gh1[par], gh2[par],
                         gh1[par ^ 1], gh2[par ^ 1], cand_n[par], (const GsMedian*)h->gs_cand.p, (const uint32_t*)h->gs_cand_blk.p, lvl_cap, h->gs_cl.p,
                         h->gs_cl.p + cap, h->gs_median.p, nxt, sig_nxt, cand_n[par ^ 1], rng_nxt, h->gs_err.p);
      hipLaunchKernelGGL(k_gs_part, dim3(nb), dim3(kGsPartThreads), 0, h->stream, tab, cur, (const uint32_t*)sig_cur, in, out,
                         (const GsMedian*)h->gs_median.p, (const uint32_t*)(h->gs_cl.p + cap), (const SsnSeg*)nxt, rng_nxt, h->gs_err.p);
      std::swap(in, out);
      std::swap(cur, nxt);
      std::swap(sig_cur, sig_nxt);
      std::swap(rng_cur, rng_nxt);
    }
    idx = in.e;          // every root's points, in original-index order
    root_sig = sig_cur;
    HIPC(hipGetLastError());
  } else if (glevels > 0) {
    // segmented sorts (lsgpu_segsort.hip.h): per level only the segments that cut along a new axis, four passes of
    // (uint32 key, uint32 index) pairs, every segment inside its own range of the arrays
    const size_t nseg_g = (size_t)1 << glevels;
    const int cap = (int)(n / kSegTile + (int64_t)(nseg_g / 2) + 2);
    HIPC(h->lane.scratch->vals_alt.reserve(n));
    HIPC(h->ssn_axis_a.reserve(nseg_g)); HIPC(h->ssn_axis_b.reserve(nseg_g)); HIPC(h->ssn_seg_fb.reserve(nseg_g));
    HIPC(h->ssn_blocktab.reserve((size_t)cap)); HIPC(h->lane.scratch->sort_hist.reserve((size_t)256 * cap + 256 + 4));
    uint32_t* keyA = reinterpret_cast<uint32_t*>(h->lane.scratch->keys.p);
    uint32_t* keyB = keyA + n;
    uint32_t* valA = h->lane.scratch->vals.p;
    uint32_t* valB = h->lane.scratch->vals_alt.p;
    uint32_t* bh = h->lane.scratch->sort_hist.p;
    uint32_t* dtot = bh + (size_t)256 * cap;
    uint32_t* nblocks_dev = dtot + 256;
    int* ax_cur = h->ssn_axis_a.p;
    int* ax_nxt = h->ssn_axis_b.p;
    HIPC(hipMemsetAsync(ax_cur, 0xFF, sizeof(int), h->stream));   // the root's order follows no axis (-1)
    for (int L = 0; L < glevels; ++L) {
      const int ns = 1 << L;
      const int grid = (int)std::min<int64_t>(cap, n / kSegTile + ns + 1);
      hipLaunchKernelGGL(k_ssn_plan, dim3(1), dim3(256), 0, h->stream, cur, ns, knn, ax_cur, h->ssn_seg_fb.p,
                         h->ssn_blocktab.p, nblocks_dev);
      hipLaunchKernelGGL(k_ssn_keys32, dim3(nblk(n)), dim3(256), 0, h->stream, src, (int)n, valA, h->ssn_seg_of.p, cur,
                         h->ssn_seg_fb.p, L == 0 ? 1 : 0, keyA);
      for (int pass = 0; pass < 4; ++pass) {
        const uint32_t* kin = (pass & 1) ? keyB : keyA; const uint32_t* vin = (pass & 1) ? valB : valA;
        uint32_t* kout = (pass & 1) ? keyA : keyB; uint32_t* vout = (pass & 1) ? valA : valB;
        hipLaunchKernelGGL(k_seg_hist<kSegItems>, dim3(grid), dim3(256), 0, h->stream, kin, h->ssn_blocktab.p, nblocks_dev, 8 * pass, bh, cap);
        hipLaunchKernelGGL(k_seg_scan, dim3(256), dim3(256), 0, h->stream, bh, cap, nblocks_dev, dtot);
        hipLaunchKernelGGL((k_seg_scatter<kSegItems>), dim3(grid), dim3(256), 0, h->stream, kin, vin, kout, vout,
                           h->ssn_blocktab.p, nblocks_dev, 8 * pass, bh, dtot, cap);
      }
      idx = valA;
      hipLaunchKernelGGL(k_ssn_split, dim3(nblk(ns)), dim3(256), 0, h->stream, src, idx, cur, ns, knn, nxt, (const int*)ax_cur, ax_nxt);
      hipLaunchKernelGGL(k_ssn_assign, dim3(nblk(n)), dim3(256), 0, h->stream, (int)n, cur, knn, h->ssn_seg_of.p, L == 0 ? 1 : 0);
      std::swap(cur, nxt);
      std::swap(ax_cur, ax_nxt);
    }
    root_axis = ax_cur;
    HIPC(hipGetLastError());
  }
  if (glevels < levels) {
    if (glevels == 0) {  // the whole cloud fits one workgroup: identity order to start from
      hipLaunchKernelGGL(k_ssn_keys, dim3(nblk(n)), dim3(256), 0, h->stream, src, (int)n, (const uint32_t*)nullptr,
                         (const uint32_t*)nullptr, cur, knn, h->lane.scratch->keys.p, h->lane.scratch->vals.p);
      idx = h->lane.scratch->vals.p;
    }
    uint32_t* idx_rw = const_cast<uint32_t*>(idx);
    if (root_max == 8192)
      hipLaunchKernelGGL(k_ssn_tree<8192>, dim3(1 << glevels), dim3(1024), 0, h->stream, src, idx_rw, cur, knn, levels - glevels, h->ssn_seg_of.p, nxt, root_axis, root_sig);
    else if (root_max == 4096)
      hipLaunchKernelGGL(k_ssn_tree<4096>, dim3(1 << glevels), dim3(512), 0, h->stream, src, idx_rw, cur, knn, levels - glevels, h->ssn_seg_of.p, nxt, root_axis, root_sig);
    else
      hipLaunchKernelGGL(k_ssn_tree<2048>, dim3(1 << glevels), dim3(256), 0, h->stream, src, idx_rw, cur, knn, levels - glevels, h->ssn_seg_of.p, nxt, root_axis, root_sig);
    std::swap(cur, nxt);
  }
  if (levels == 0) {  // a single box: identity order
    hipLaunchKernelGGL(k_ssn_keys, dim3(nblk(n)), dim3(256), 0, h->stream, src, (int)n, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr, cur, knn, h->lane.scratch->keys.p, h->lane.scratch->vals.p);
    HIPC(hipMemsetAsync(h->ssn_seg_of.p, 0, (size_t)n * 4, h->stream));
    idx = h->lane.scratch->vals.p;
  }
  hipLaunchKernelGGL(k_ssn_boxes, dim3((int)((nseg + 127) / 128)), dim3(128), 0, h->stream, src, idx, cur, (int)nseg,
                     h->ssn_box_normal.p, h->ssn_box_pts.p);
  HIPC(hipGetLastError());
  int rc = scan_u32(h, h->ssn_box_pts.p, h->ssn_box_base.p, nseg);
  if (rc) return rc;
  // the draws: at most one per point; produced on the helper thread while the kernels above were enqueued
  rc = ahead->ready(first_draw + (size_t)n);
  if (rc) return rc;
  hipLaunchKernelGGL(k_ssn_select, dim3(nblk(n)), dim3(256), 0, h->stream, (int)n, idx, h->ssn_seg_of.p, cur,
                     h->ssn_box_pts.p, h->ssn_box_base.p, h->ssn_draws.p + first_draw, ratio, h->ssn_keep.p);
  rc = scan_u32(h, h->ssn_keep.p, h->ssn_out_pos.p, (size_t)n, false, /*nonzero*/ true);
  if (rc == LSGPU_OK) {
    hipLaunchKernelGGL(k_ssn_emit, dim3(nblk(n)), dim3(256), 0, h->stream, src, (int)n,
                       h->ssn_box_normal.p, h->ssn_keep.p, h->ssn_out_pos.p, out_xyz1, out_nrm);
  }
  uint32_t n_draws = 0, kept = 0;
  if (rc == LSGPU_OK)
    // (the sort-free levels' error words travel with the totals)
    rc = scan_totals(h, h->ssn_box_pts.p, h->ssn_box_base.p, nseg, h->ssn_keep.p, h->ssn_out_pos.p, (size_t)n, &n_draws, &kept,
                     select_levels ? h->gs_err.p : nullptr, h->pin->gs_err, sizeof h->pin->gs_err, /*b_flags*/ true);
  if (rc) return rc;
  if (select_levels && h->pin->gs_err[0]) {
    if (getenv("LSGPU_GS_DEBUG")) fprintf(stderr, "lsgpu: sort-free levels gave up (n %lld): code %u seg %u a %u b %u | part %u seg %u dst %u\n", (long long)n,
                                          h->pin->gs_err[1], h->pin->gs_err[2], h->pin->gs_err[3], h->pin->gs_err[4], h->pin->gs_err[5], h->pin->gs_err[6], h->pin->gs_err[7]);
    // thousands of equal coordinates around a median (more candidates than a workgroup selects among): the segmented
    // sorts do not care -- the same filter again with them (same draws: nothing has been consumed yet).  Counted:
    // lsgpu_icp_get_policy_info shows a handle that pays the filter twice on every call.
    ++h->ssn_sort_fallbacks;
    return ssn_device(h, src, n, knn, ratio, seed, out_xyz1, out_nrm, n_out, ahead, true);
  }
  ahead->used = first_draw + (size_t)n_draws;  // dropped boxes drew nothing
  HIPC(hipGetLastError());
  *n_out = kept;
  return LSGPU_OK;
}

// RandomSampling on device memory (order preserved)
// (defer_wait: everything is enqueued, the host's wait for the number of points kept is left to compact_kept_wait)
static int random_sampling_device(lsgpu_icp* h, const float4* src, int64_t n, float prob, int64_t seed,
                                  float4* out_xyz1, int64_t* n_out, DrawAhead* ahead = nullptr, bool defer_wait = false) {
  *n_out = 0;
  HIPC(h->ssn_keep.reserve(n));
  HIPC(h->ssn_out_pos.reserve(n));
  DrawAhead own;
  int rc = LSGPU_OK;
  if (!ahead) {
    rc = own.begin(h, seed, (size_t)n);
    if (rc) return rc;
    ahead = &own;
  }
  const size_t first_draw = ahead->used;
  ahead->used = first_draw + (size_t)n;  // one draw per point, whatever happens next
  rc = ahead->ready();
  if (rc) return rc;
  hipLaunchKernelGGL(k_draw_select, dim3(nblk(n)), dim3(256), 0, h->lane.stream, (int)n, h->ssn_draws.p + first_draw, prob, h->ssn_keep.p);
  rc = compact_kept_enqueue(h, src, n, out_xyz1);
  if (rc || defer_wait) return rc;
  return compact_kept_wait(h, n_out);
}

// The cut modules of one filter section as the pass takes them (rs: RandomSampling stands among the reading's)
static CutSectionDev cut_section_of(const lsgpu_chain_cuts& c, int side, bool rs) {
  CutSectionDev d;
  std::memset(&d, 0, sizeof(d));
  const lsgpu_point_filter* m = side == 0 ? c.reading : c.reference;
  d.n = std::max(0, std::min(side == 0 ? c.n_reading : c.n_reference, kCutMax));
  d.n_pre = side == 0 && rs ? std::max(0, std::min(c.reading_sampling_at, d.n)) : d.n;
  for (int k = 0; k < d.n; ++k) {
    d.m[k].type = m[k].type; d.m[k].dim = m[k].dim; d.m[k].flag = m[k].flag;
    for (int i = 0; i < 6; ++i) d.m[k].v[i] = m[k].v[i];
  }
  return d;
}
// A filter section in one pass on the current lane (lsgpu_chain_cut.hip.h): src (n points, device) -> the kept points at the
// front of dst (device, room for n, not src), order preserved; rs: keep = pre && draws[rank of pre] < prob && post, `draws`
// (device) holding at least n.  The launches are the same whatever cs holds; the totals are on their way to the host ...
// nrm / dst_nrm (device, both or neither): the normals beside src, kept with their points (dst_nrm: room for 3 n, not nrm)
static int cut_section_enqueue(lsgpu_icp* h, const CutSectionDev& cs, bool rs, float prob, const float* draws, const float4* src,
                               int64_t n, float4* dst, const float* nrm = nullptr, float* dst_nrm = nullptr) {
  const int nb = nblk(n);
  const size_t row = ((size_t)nb + 3) & ~(size_t)3;
  HIPC(h->cut_blk.reserve(4 * row));
  uint32_t *cnt_a = h->cut_blk.p, *off_a = cnt_a + row, *cnt_b = off_a + row, *off_b = cnt_b + row;
  hipStream_t st = h->lane.stream;
  const float* const no_nrm = nullptr; float* const no_out_nrm = nullptr;
  hipLaunchKernelGGL((k_cut_pass<0, false>), dim3(nb), dim3(256), 0, st, src, (int)n, cs, (const float*)nullptr, 0.f,
                     (const uint32_t*)nullptr, (const uint32_t*)nullptr, cnt_a, (float4*)nullptr, no_nrm, no_out_nrm);
  int rc = scan_u32(h, cnt_a, off_a, (size_t)nb);
  if (rc) return rc;
  if (!rs) {
    if (nrm)
      hipLaunchKernelGGL((k_cut_pass<2, false, true>), dim3(nb), dim3(256), 0, st, src, (int)n, cs, (const float*)nullptr, 0.f,
                         (const uint32_t*)nullptr, (const uint32_t*)off_a, (uint32_t*)nullptr, dst, nrm, dst_nrm);
    else
    hipLaunchKernelGGL((k_cut_pass<2, false>), dim3(nb), dim3(256), 0, st, src, (int)n, cs, (const float*)nullptr, 0.f,
                       (const uint32_t*)nullptr, (const uint32_t*)off_a, (uint32_t*)nullptr, dst, no_nrm, no_out_nrm);
    HIPC(hipGetLastError());
    return scan_totals_enqueue(h, nullptr, nullptr, 0, cnt_a, off_a, (size_t)nb);
  }
  hipLaunchKernelGGL((k_cut_pass<1, true>), dim3(nb), dim3(256), 0, st, src, (int)n, cs, draws, prob, (const uint32_t*)off_a,
                     (const uint32_t*)nullptr, cnt_b, (float4*)nullptr, no_nrm, no_out_nrm);
  rc = scan_u32(h, cnt_b, off_b, (size_t)nb);
  if (rc) return rc;
  if (nrm)
    hipLaunchKernelGGL((k_cut_pass<2, true, true>), dim3(nb), dim3(256), 0, st, src, (int)n, cs, draws, prob, (const uint32_t*)off_a,
                       (const uint32_t*)off_b, (uint32_t*)nullptr, dst, nrm, dst_nrm);
  else
  hipLaunchKernelGGL((k_cut_pass<2, true>), dim3(nb), dim3(256), 0, st, src, (int)n, cs, draws, prob, (const uint32_t*)off_a,
                     (const uint32_t*)off_b, (uint32_t*)nullptr, dst, no_nrm, no_out_nrm);
  HIPC(hipGetLastError());
  return scan_totals_enqueue(h, cnt_a, off_a, (size_t)nb, cnt_b, off_b, (size_t)nb);
}
// ... and the host's wait for them: the points kept, and `pre` -- the points that reached RandomSampling, one draw each
// (without it: the points kept)
static int cut_section_wait(lsgpu_icp* h, bool rs, int64_t* pre, int64_t* kept) {
  uint32_t a = 0, b = 0;
  const int rc = scan_totals_wait(h, &a, &b);
  if (rc) return rc;
  *kept = b;
  *pre = rs ? a : b;
  return LSGPU_OK;
}

// SurfaceNormalDataPointsFilter on the reference the handle holds (set_reference has just been enqueued on h->stream):
// normals of the sorted points into h->nrm; ids / d2 (device, nullable) in the order the cloud was given.
// dens (device, nullable): keepDensities 1 -- the density of every point, in the order the cloud was given (the DENS kernels)
template <int K, bool DENS>
static void launch_snf_(lsgpu_icp* h, const SnfArgs& a) {
  hipLaunchKernelGGL((k_snf_tile<K, DENS>), dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, h->stream, a);
  hipLaunchKernelGGL((k_snf_fallback<K, DENS>), dim3((unsigned)std::min((a.n + 63) / 64, 4096)), dim3(64), 0, h->stream, a);   // (strides over the list: usually short)
}
template <int K>
static void launch_snf(lsgpu_icp* h, const SnfArgs& a) {
  if (a.dens) launch_snf_<K, true>(h, a); else launch_snf_<K, false>(h, a);
}
static int snf_device(lsgpu_icp* h, int knn, int* ids, float* d2, float* dens = nullptr) {
  const int64_t n = h->nr;
  if (knn < kSnfMinKnn || knn > kSnfMaxKnn || n < knn) {
    h->err = "SurfaceNormalDataPointsFilter: knn must be in [3, 32] and the cloud must hold at least knn points";
    return LSGPU_BAD_ARG;
  }
  HIPC(h->snf_strag.reserve(n)); HIPC(h->snf_count.reserve(1));
  HIPC(hipMemsetAsync(h->snf_count.p, 0, sizeof(uint32_t), h->stream));
  SnfArgs a;
  a.n = (int)n; a.knn = knn; a.g = h->grid; a.pts = h->pts.p; a.inv = h->ref_inv.p; a.chunks = h->chunks.p;
  a.nrm = h->nrm.p; a.ids = ids; a.d2 = ids ? d2 : nullptr;
  a.strag = h->snf_strag.p; a.strag_count = h->snf_count.p; a.r_cap = kSnfRCap; a.dens = dens;
  // list lengths: the first knn entries of the next larger list are exact (lsgpu_snf.hip.h)
  if (knn <= 4) launch_snf<4>(h, a);
  else if (knn <= 8) launch_snf<8>(h, a);
  else if (knn <= 16) launch_snf<16>(h, a);
  else launch_snf<32>(h, a);
  HIPC(hipGetLastError());
  return LSGPU_OK;
}

// MaxDensityDataPointsFilter on the current lane (lsgpu_max_density.hip.h): src (n points, device, as given) with the densities
// dens (device, the cloud's order) -> the kept points at the front of out_pts, their normals -- gathered from the handle's
// sorted normals through h->ref_inv (normals false: none are read or written) -- in out_nrm; draws (device): at least n.  The
// totals are on their way to the host ...
static int max_density_enqueue(lsgpu_icp* h, const float4* src, int64_t n, const float* dens, float max_density,
                               const float* draws, bool normals, float4* out_pts, float* out_nrm) {
  const int nb = nblk(n);
  const size_t row = ((size_t)nb + 3) & ~(size_t)3;
  HIPC(h->md_blk.reserve(4 * row)); HIPC(h->md_stat.reserve(1));
  uint32_t *cnt_a = h->md_blk.p, *off_a = cnt_a + row, *cnt_b = off_a + row, *off_b = cnt_b + row;
  hipStream_t st = h->lane.stream;
  HIPC(hipMemsetAsync(h->md_stat.p, 0, sizeof(MdStat), st));
  HIPC(hipMemsetAsync(&h->md_stat.p->lo, 0xFF, sizeof(uint32_t), st));
  const uint32_t* inv = h->ref_inv.p;
  const float4* nrm = normals ? h->nrm.p : nullptr;
  hipLaunchKernelGGL((k_md_pass<0>), dim3(nb), dim3(256), 0, st, src, dens, (int)n, max_density, (const float*)nullptr, h->md_stat.p,
                     (const uint32_t*)nullptr, (const uint32_t*)nullptr, cnt_a, inv, nrm, (float4*)nullptr, (float*)nullptr);
  int rc = scan_u32(h, cnt_a, off_a, (size_t)nb);
  if (rc) return rc;
  hipLaunchKernelGGL((k_md_pass<1>), dim3(nb), dim3(256), 0, st, src, dens, (int)n, max_density, draws, h->md_stat.p,
                     (const uint32_t*)off_a, (const uint32_t*)nullptr, cnt_b, inv, nrm, (float4*)nullptr, (float*)nullptr);
  rc = scan_u32(h, cnt_b, off_b, (size_t)nb);
  if (rc) return rc;
  hipLaunchKernelGGL((k_md_pass<2>), dim3(nb), dim3(256), 0, st, src, dens, (int)n, max_density, draws, h->md_stat.p,
                     (const uint32_t*)off_a, (const uint32_t*)off_b, (uint32_t*)nullptr, inv, nrm, out_pts, out_nrm);
  HIPC(hipGetLastError());
  return scan_totals_enqueue(h, cnt_a, off_a, (size_t)nb, cnt_b, off_b, (size_t)nb);
}
// ... and the host's wait for them: the dense points (one draw each) and the points kept
static int max_density_wait(lsgpu_icp* h, int64_t* n_dense, int64_t* kept) {
  uint32_t a = 0, b = 0;
  const int rc = scan_totals_wait(h, &a, &b);
  if (rc) return rc;
  *n_dense = a; *kept = b;
  return LSGPU_OK;
}

// ShadowDataPointsFilter on the current lane (lsgpu_shadow.hip.h): src (n points, device, as given to the section) with the
// normals nrm3 (device, 3 floats per point in the cloud's order) -- or, nrm3 == nullptr, with the handle's sorted normals
// gathered through h->ref_inv (the snf kernels have just written them for this cloud) -> the kept points at the front of
// out_pts, their normals in out_nrm (device, room for n points each, not the inputs).  The total is on its way to the host ...
static int shadow_enqueue(lsgpu_icp* h, const float4* src, const float* nrm3, int64_t n, float eps, float4* out_pts, float* out_nrm) {
  const int nb = nblk(n);
  const size_t row = ((size_t)nb + 3) & ~(size_t)3;
  HIPC(h->sh_blk.reserve(2 * row));
  uint32_t *cnt = h->sh_blk.p, *off = cnt + row;
  hipStream_t st = h->lane.stream;
  const uint32_t* inv = h->ref_inv.p;
  const float4* nrm4 = h->nrm.p;
  if (nrm3)
    hipLaunchKernelGGL((k_shadow_pass<0, false>), dim3(nb), dim3(256), 0, st, src, nrm3, (const uint32_t*)nullptr, (const float4*)nullptr,
                       (int)n, eps, (const uint32_t*)nullptr, cnt, (float4*)nullptr, (float*)nullptr);
  else
    hipLaunchKernelGGL((k_shadow_pass<0, true>), dim3(nb), dim3(256), 0, st, src, (const float*)nullptr, inv, nrm4,
                       (int)n, eps, (const uint32_t*)nullptr, cnt, (float4*)nullptr, (float*)nullptr);
  const int rc = scan_u32(h, cnt, off, (size_t)nb);
  if (rc) return rc;
  if (nrm3)
    hipLaunchKernelGGL((k_shadow_pass<2, false>), dim3(nb), dim3(256), 0, st, src, nrm3, (const uint32_t*)nullptr, (const float4*)nullptr,
                       (int)n, eps, (const uint32_t*)off, (uint32_t*)nullptr, out_pts, out_nrm);
  else
    hipLaunchKernelGGL((k_shadow_pass<2, true>), dim3(nb), dim3(256), 0, st, src, (const float*)nullptr, inv, nrm4,
                       (int)n, eps, (const uint32_t*)off, (uint32_t*)nullptr, out_pts, out_nrm);
  HIPC(hipGetLastError());
  return scan_totals_enqueue(h, nullptr, nullptr, 0, cnt, off, (size_t)nb);
}
// ... and the host's wait for it: the points kept
static int shadow_wait(lsgpu_icp* h, int64_t* kept) {
  uint32_t unused = 0, k = 0;
  const int rc = scan_totals_wait(h, &unused, &k);
  if (rc) return rc;
  *kept = k;
  return LSGPU_OK;
}

extern "C" {

int lsgpu_icp_filter_shadow(lsgpu_icp* h, const float* xyz1, const float* normals, int64_t n, float eps, float* out_xyz1,
                            float* out_normals, int64_t* n_out) {
  if (!h || !n_out) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  if (n < 0 || n > 0x7FFFFFF0ll / 3 || (n > 0 && (!xyz1 || !normals || !out_xyz1 || !out_normals))) return LSGPU_BAD_ARG;
  if (n > 0 && (static_cast<const void*>(out_xyz1) == static_cast<const void*>(xyz1) || static_cast<const void*>(out_normals) == static_cast<const void*>(normals))) {
    h->err = "filter_shadow: the outputs must not be the inputs";
    return LSGPU_BAD_ARG;
  }
  if (!shadow::eps_ok(eps)) { h->err = "ShadowDataPointsFilter: eps must be in [0, 3.1416]"; return LSGPU_BAD_CONFIG; }
  if (n == 0) { h->err = "filter_shadow: no points to filter"; return LSGPU_NO_CONVERGENCE; }
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr; const float* nsrc = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (!rc) rc = stage_in(h, normals, (size_t)3 * n, h->sh_nrm_in, &nsrc);
  if (rc) return rc;
  OutStage<float4> ox; OutStage<float> on;
  if ((rc = ox.open(h, out_xyz1, h->sh_ref, n))) return rc;
  if ((rc = on.open(h, out_normals, h->sh_nrm, 3 * n))) return rc;
  int64_t kept = 0;
  rc = shadow_enqueue(h, src, nsrc, n, eps, ox.p, on.p);
  if (!rc) rc = shadow_wait(h, &kept);
  if (rc) return rc;
  *n_out = kept;
  if ((rc = ox.copy_back(h, (size_t)kept))) return rc;
  if ((rc = on.copy_back(h, 3 * (size_t)kept))) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  if (kept <= 0) { h->err = "filter_shadow: the filter left no point"; return LSGPU_NO_CONVERGENCE; }
  return LSGPU_OK;
}

}  // extern "C"

// One sums pass of CovarianceSamplingDataPointsFilter on the current lane (lsgpu_cov_sampling.hip.h): its columns are in
// h->pin->cs on return -- the host needs them to parametrise the next pass.
template <int PASS>
static int cov_sampling_sums(lsgpu_icp* h, const float4* src, const float* nrm3, int64_t n, const CsParams& q) {
  const int nb = std::min(nblk(n), kCsBlocksMax);
  hipStream_t st = h->lane.stream;
  hipLaunchKernelGGL((k_cs_pass<PASS>), dim3(nb), dim3(256), 0, st, src, nrm3, (int)n, q, h->cs_partials.p);
  hipLaunchKernelGGL(k_cs_final, dim3(1), dim3(1024), 0, st, (const double*)h->cs_partials.p, nb, PASS, h->cs_out.p);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h->pin->cs, h->cs_out.p, (size_t)cs_cols(PASS) * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  return LSGPU_OK;
}

// CovarianceSamplingDataPointsFilter on the current lane: src (n points, device, as given to the section) with the normals nrm3
// (device, 3 floats per point) -> the nb chosen points, normals and indices in pick order at the front of out_pts / out_nrm /
// out_ids (device, room for nb, not the inputs); 1 <= nb < n.  sums: the 32 doubles of lsgpu_icp_filter_cov_sampling.  Three
// short waits for sums, one for the heads of the sorted lists; the gather is enqueued, not waited for.  ms (nullable): wall
// time of the four phases -- sums, projections and sorts, heads download and walk, upload and gather (enqueue only).
static int cov_sampling_run(lsgpu_icp* h, const float4* src, const float* nrm3, int64_t n, int64_t nb, int torque_norm,
                            float4* out_pts, float* out_nrm, int32_t* out_ids, double sums[covs::kSums], double ms[4]) {
  const double t0 = wall_ms();
  hipStream_t st = h->lane.stream;
  // (the kernels hold a point's index in an int: the entry's limit holds for a section of a compute too)
  if (n > covs::kPointsMax) { h->err = "CovarianceSamplingDataPointsFilter: more than (2^31 - 16) / 6 points"; return LSGPU_BAD_ARG; }
  HIPC(h->cs_partials.reserve((size_t)kCsBlocksMax * kCsStride));
  HIPC(h->cs_out.reserve(kCsStride));
  std::fill(sums, sums + covs::kSums, 0.0);
  sums[covs::kSumN] = (double)n;
  CsParams q{};
  int rc = cov_sampling_sums<0>(h, src, nrm3, n, q);
  if (rc) return rc;
  std::memcpy(sums, h->pin->cs, 9 * sizeof(double));
  if (!covs::finite_sums(sums)) { h->err = "CovarianceSamplingDataPointsFilter: a coordinate that is not finite"; return LSGPU_BAD_ARG; }
  covs::centre(sums, n, q.c);
  if (torque_norm == 1) {
    if ((rc = cov_sampling_sums<1>(h, src, nrm3, n, q))) return rc;
    sums[covs::kSumLen] = h->pin->cs[0];
  }
  const float L = covs::lnorm(torque_norm, sums, n);
  if (!(L != 0.f) || !std::isfinite(L)) { h->err = "CovarianceSamplingDataPointsFilter: Lnorm is 0 or not finite (torqueNorm " + std::to_string(torque_norm) + ")"; return LSGPU_BAD_ARG; }
  q.invL = 1.f / L;
  if ((rc = cov_sampling_sums<2>(h, src, nrm3, n, q))) return rc;
  std::memcpy(sums + covs::kSumC, h->pin->cs, 21 * sizeof(double));
  if (!covs::finite_sums(sums)) { h->err = "CovarianceSamplingDataPointsFilter: a point or normal that is not finite"; return LSGPU_BAD_ARG; }
  covs::Eig e;
  covs::eigen(sums + covs::kSumC, e.X, nullptr);
  const double t1 = wall_ms();

  const int64_t m = nb;   // (< n)
  HIPC(h->cs_mag.reserve(6 * (size_t)n));
  HIPC(h->cs_heads.reserve(6 * (size_t)m));
  HIPC(h->cs_heads_pin.reserve(6 * (size_t)m));
  HIPC(h->cs_ids_pin.reserve((size_t)m));
  HIPC(h->cs_ids.reserve((size_t)m));
  HIPC(h->lane.scratch->keys.reserve(n));
  HIPC(h->lane.scratch->vals.reserve(n));
  hipLaunchKernelGGL(k_cs_project, dim3(nblk(n)), dim3(256), 0, st, src, nrm3, (int)n, q, e, h->cs_mag.p);
  for (int k = 0; k < 6; ++k) {   // (sort_pairs may exchange the scratch's buffer pairs: the members are read anew every time)
    hipLaunchKernelGGL(k_cs_keys, dim3(nblk(n)), dim3(256), 0, st, (const float*)h->cs_mag.p, (int)n, k, h->lane.scratch->keys.p,
                       h->lane.scratch->vals.p);
    if ((rc = sort_pairs(h, n, 32))) return rc;
    hipLaunchKernelGGL(k_cs_heads, dim3(nblk(m)), dim3(256), 0, st, (const uint32_t*)h->lane.scratch->vals_alt.p, (int)m, (int)n,
                       (const float*)h->cs_mag.p, h->cs_heads.p + (size_t)k * (size_t)m);
  }
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(h->cs_heads_pin.p, h->cs_heads.p, 6 * (size_t)m * sizeof(covs::Head), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  const double t2 = wall_ms();
  if (covs::walk(h->cs_heads_pin.p, m, n, nb, h->cs_ids_pin.p, h->cs_chosen) != nb) {
    h->err = "CovarianceSamplingDataPointsFilter: a sorted list ran out before nbSample points were chosen";
    return LSGPU_HIP_ERROR;
  }
  const double t3 = wall_ms();
  HIPC(hipMemcpyAsync(h->cs_ids.p, h->cs_ids_pin.p, (size_t)nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_cs_gather, dim3(nblk(nb)), dim3(256), 0, st, src, nrm3, (const uint32_t*)h->cs_ids.p, (int)nb, (int)n, out_pts,
                     out_nrm, out_ids);
  HIPC(hipGetLastError());
  if (ms) { ms[0] = t1 - t0; ms[1] = t2 - t1; ms[2] = t3 - t2; ms[3] = wall_ms() - t3; }
  return LSGPU_OK;
}

extern "C" {

int lsgpu_icp_filter_cov_sampling(lsgpu_icp* h, const float* xyz1, const float* normals, int64_t n, int nb_sample, int torque_norm,
                                  float* out_xyz1, float* out_normals, int32_t* out_ids, int64_t* n_out, double sums_out[32]) {
  if (!h || !n_out) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  if (n < 0 || n > covs::kPointsMax || (n > 0 && (!xyz1 || !normals || !out_xyz1 || !out_normals))) return LSGPU_BAD_ARG;
  if (n > 0 && (static_cast<const void*>(out_xyz1) == static_cast<const void*>(xyz1) || static_cast<const void*>(out_normals) == static_cast<const void*>(normals))) {
    h->err = "filter_cov_sampling: the outputs must not be the inputs";
    return LSGPU_BAD_ARG;
  }
  if (!covs::nb_sample_ok(nb_sample)) { h->err = "CovarianceSamplingDataPointsFilter: nbSample must be in [1, 2147483632]"; return LSGPU_BAD_CONFIG; }
  if (!covs::torque_norm_ok(torque_norm)) { h->err = "CovarianceSamplingDataPointsFilter: torqueNorm must be 0, 1 or 2"; return LSGPU_BAD_CONFIG; }
  if (n == 0) { h->err = "filter_cov_sampling: no points to filter"; return LSGPU_NO_CONVERGENCE; }
  HIPC(hipSetDevice(h->device));
  if ((int64_t)nb_sample >= n) {   // the cloud passes unchanged, nothing is computed
    HIPC(hipMemcpyAsync(out_xyz1, xyz1, (size_t)n * 16, hipMemcpyDefault, h->stream));
    HIPC(hipMemcpyAsync(out_normals, normals, (size_t)n * 12, hipMemcpyDefault, h->stream));
    if (out_ids) {
      HIPC(h->cs_ids_pin.reserve((size_t)n));
      for (int64_t i = 0; i < n; ++i) h->cs_ids_pin.p[i] = (uint32_t)i;
      HIPC(hipMemcpyAsync(out_ids, h->cs_ids_pin.p, (size_t)n * 4, hipMemcpyDefault, h->stream));
    }
    HIPC(hipStreamSynchronize(h->stream));
    if (sums_out) { std::fill(sums_out, sums_out + covs::kSums, 0.0); sums_out[covs::kSumN] = (double)n; }
    *n_out = n;
    return LSGPU_OK;
  }
  const float4* src = nullptr; const float* nsrc = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (!rc) rc = stage_in(h, normals, (size_t)3 * n, h->cs_nrm_in, &nsrc);
  if (rc) return rc;
  const size_t nb = (size_t)nb_sample;
  OutStage<float4> ox; OutStage<float> on; OutStage<int32_t> oi;
  if ((rc = ox.open(h, out_xyz1, h->cs_pts_out, nb))) return rc;
  if ((rc = on.open(h, out_normals, h->cs_nrm_out, 3 * nb))) return rc;
  if (out_ids) { if ((rc = oi.open(h, out_ids, h->cs_ids_out, nb))) return rc; }
  else { HIPC(h->cs_ids_out.reserve(nb)); oi.p = h->cs_ids_out.p; }
  double sums[covs::kSums];
  if ((rc = cov_sampling_run(h, src, nsrc, n, (int64_t)nb, torque_norm, ox.p, on.p, oi.p, sums, h->cs_ms))) return rc;
  if ((rc = ox.copy_back(h, nb))) return rc;
  if ((rc = on.copy_back(h, 3 * nb))) return rc;
  if (out_ids && (rc = oi.copy_back(h, nb))) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  if (sums_out) std::memcpy(sums_out, sums, sizeof sums);
  *n_out = (int64_t)nb;
  return LSGPU_OK;
}

int lsgpu_icp_cov_sampling_phase_ms(lsgpu_icp* h, double ms[4]) {
  if (!h || !ms) return LSGPU_BAD_ARG;
  std::memcpy(ms, h->cs_ms, sizeof h->cs_ms);
  return LSGPU_OK;
}

}  // extern "C"

// lsgpu_icp_filter_reference_normals, with the densities of keepDensities 1 if the caller asks for them
static int filter_reference_normals_run(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float* out_normals, int32_t* out_ids,
                                        float* out_d2, float* out_densities);

extern "C" {

int lsgpu_icp_filter_reference_normals(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float* out_normals,
                                       int32_t* out_ids, float* out_d2) {
  return filter_reference_normals_run(h, xyz1, n, knn, out_normals, out_ids, out_d2, nullptr);
}

int lsgpu_icp_filter_reference_normals_densities(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float* out_normals,
                                                 int32_t* out_ids, float* out_d2, float* out_densities) {
  return filter_reference_normals_run(h, xyz1, n, knn, out_normals, out_ids, out_d2, out_densities);
}

int lsgpu_icp_filter_reference_max_density(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float max_density, int64_t seed,
                                           float* out_xyz1, float* out_normals, float* out_densities, int64_t* n_out,
                                           int64_t* n_dense) {
  if (!h || !out_xyz1 || !out_normals || !n_out || !n_dense) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0; *n_dense = 0;
  lsgpu_max_density_config mc{};
  mc.max_density = max_density;
  if (const char* why = lsgpu_max_density_config_why(&mc, kSnfMinKnn)) { h->err = why; return LSGPU_BAD_CONFIG; }
  if (knn < kSnfMinKnn || knn > kSnfMaxKnn) { h->err = "filter_reference_max_density: knn must be in [3, 32]"; return LSGPU_BAD_ARG; }
  if (!xyz1 || n < knn) { h->err = "filter_reference_max_density: the cloud has fewer points than knn"; return LSGPU_BAD_ARG; }
  if (n > 0x7FFFFFF0ll / knn) { h->err = "filter_reference_max_density: knn x n exceeds the 32-bit pair count"; return LSGPU_BAD_ARG; }
  if (static_cast<const void*>(out_xyz1) == static_cast<const void*>(xyz1)) { h->err = "filter_reference_max_density: out_xyz1 must not be the input"; return LSGPU_BAD_ARG; }
  if (seed >= 0) DrawStream::global().take(seed, 0, nullptr);
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (!rc) rc = lsgpu_icp_set_reference(h, reinterpret_cast<const float*>(src), nullptr, n);
  if (rc) return rc;
  OutStage<float4> ox; OutStage<float> on;
  if ((rc = ox.open(h, out_xyz1, h->flt_ref, n))) return rc;
  if ((rc = on.open(h, out_normals, h->flt_nrm, 3 * n))) return rc;
  HIPC(h->dens.reserve(n));
  rc = snf_device(h, knn, nullptr, nullptr, h->dens.p);
  if (rc) return rc;
  h->have_normals = true;
  rc = upload_draws_begin(h, -1, (size_t)n);   // at most one draw per point; the stream stays locked until the commit
  if (rc) return rc;
  int64_t dense = 0, kept = 0;
  rc = max_density_enqueue(h, src, n, h->dens.p, max_density, h->ssn_draws.p, true, ox.p, on.p);
  if (!rc) rc = max_density_wait(h, &dense, &kept);
  DrawStream::global().commit(rc ? 0 : (size_t)dense);   // one draw per dense point
  if (rc) return rc;
  *n_out = kept; *n_dense = dense;
  if ((rc = ox.copy_back(h, (size_t)kept))) return rc;
  if ((rc = on.copy_back(h, 3 * (size_t)kept))) return rc;
  if (out_densities)
    HIPC(hipMemcpyAsync(out_densities, h->dens.p, (size_t)n * sizeof(float),
                        is_device_ptr(out_densities) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  if (kept <= 0) { h->err = "filter_reference_max_density: the filter left no point"; return LSGPU_NO_CONVERGENCE; }
  return LSGPU_OK;
}

}  // extern "C"

static int filter_reference_normals_run(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float* out_normals, int32_t* out_ids,
                                        float* out_d2, float* out_densities) {
  if (!h || !out_normals || (out_d2 && !out_ids)) return LSGPU_BAD_ARG;
  h->err.clear();
  if (knn < kSnfMinKnn || knn > kSnfMaxKnn) { h->err = "filter_reference_normals: knn must be in [3, 32]"; return LSGPU_BAD_ARG; }
  if (!xyz1 || n < knn) { h->err = "filter_reference_normals: the cloud has fewer points than knn"; return LSGPU_BAD_ARG; }
  if (n > 0x7FFFFFF0ll / knn) { h->err = "filter_reference_normals: knn x n exceeds the 32-bit pair count"; return LSGPU_BAD_ARG; }
  int rc = lsgpu_icp_set_reference(h, xyz1, nullptr, n);
  if (rc) return rc;
  const int64_t np = (int64_t)knn * n;
  OutStage<float> on; OutStage<int> oi; OutStage<float> od;
  if ((rc = on.open(h, out_normals, h->flt_nrm, 3 * n))) return rc;
  if (out_ids && (rc = oi.open(h, out_ids, h->ids_io, np))) return rc;
  if (out_ids && (rc = od.open(h, out_d2, h->d2_io, np))) return rc;   // (the kernels write both or neither: no out_d2, the handle's buffer)
  OutStage<float> odn;
  if (out_densities && (rc = odn.open(h, out_densities, h->dens_io, n))) return rc;   // (the kernels store at the original index: the caller's order)
  rc = snf_device(h, knn, oi.p, od.p, odn.p);
  if (rc) return rc;
  hipLaunchKernelGGL(k_snf_unpermute, dim3(nblk(n)), dim3(256), 0, h->stream, h->pts.p, (int)n, h->nrm.p, on.p);
  HIPC(hipGetLastError());
  if ((rc = on.copy_back(h, 3 * n))) return rc;
  if ((rc = oi.copy_back(h, np))) return rc;
  if (out_d2 && (rc = od.copy_back(h, np))) return rc;
  if (out_densities && (rc = odn.copy_back(h, n))) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

extern "C" {

int lsgpu_icp_filter_reference(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, float ratio,
                               int64_t seed, float* out_xyz1, float* out_normals, int64_t* n_out) {
  if (!h || !n_out || !out_xyz1 || !out_normals) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  if (knn < 3 || knn > kSsnMaxKnn) { h->err = "filter_reference: knn must be in [3, 32]"; return LSGPU_BAD_ARG; }
  if (seed >= 0) DrawStream::global().take(seed, 0, nullptr);
  if (n <= 0 || !xyz1) return LSGPU_OK;
  if (n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (rc) return rc;
  OutStage<float4> ox; OutStage<float> on;
  if ((rc = ox.open(h, out_xyz1, h->flt_ref, n))) return rc;
  if ((rc = on.open(h, out_normals, h->flt_nrm, 3 * n))) return rc;
  rc = ssn_device(h, src, n, knn, ratio, -1, ox.p, on.p, n_out);
  if (rc) return rc;
  if ((rc = ox.copy_back(h, *n_out))) return rc;
  if ((rc = on.copy_back(h, 3 * *n_out))) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_icp_filter_reading(lsgpu_icp* h, const float* xyz1, int64_t n, float prob, int64_t seed,
                             float* out_xyz1, int64_t* n_out) {
  if (!h || !n_out || !out_xyz1) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  if (seed >= 0) DrawStream::global().take(seed, 0, nullptr);
  if (n <= 0 || !xyz1) return LSGPU_OK;
  if (n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (rc) return rc;
  OutStage<float4> ox;
  if ((rc = ox.open(h, out_xyz1, h->flt_rd, n))) return rc;
  rc = random_sampling_device(h, src, n, prob, -1, ox.p, n_out);
  if (rc) return rc;
  if ((rc = ox.copy_back(h, *n_out))) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_icp_filter_section(lsgpu_icp* h, const lsgpu_chain_cuts* cuts, int side, float prob, const float* xyz1, int64_t n,
                             int64_t seed, float* out_xyz1, int64_t* n_out) {
  if (!h || !cuts || !n_out || (side != 0 && side != 1) || n < 0 || (n > 0 && (!xyz1 || !out_xyz1))) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  if (n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  const std::string why = chain_cuts_why(cuts);
  if (!why.empty()) { h->err = why; return LSGPU_BAD_CONFIG; }
  const bool rs = side == 0 && prob >= 0.f;
  if (rs && !(prob <= 1.f)) { h->err = "filter_section: RandomSamplingDataPointsFilter: prob must be in [0, 1]"; return LSGPU_BAD_CONFIG; }
  if (seed >= 0) DrawStream::global().take(seed, 0, nullptr);
  const CutSectionDev cs = cut_section_of(*cuts, side, rs);
  if (n == 0) {   // as lsgpu_apply_point_filters: an empty chain is a no-op, a module handed an empty cloud is an error
    if (cs.n == 0 && !rs) return LSGPU_OK;
    h->err = "filter_section: no points to filter";
    return LSGPU_NO_CONVERGENCE;
  }
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (rc) return rc;
  OutStage<float4> ox;
  // (the pass must not write where it reads: a caller's device buffer that is the input goes through the handle's)
  if (static_cast<const void*>(out_xyz1) == static_cast<const void*>(xyz1)) { ox.user = out_xyz1; ox.staged = false; HIPC(h->flt_rd.reserve(n)); ox.p = h->flt_rd.p; }
  else if ((rc = ox.open(h, out_xyz1, h->flt_rd, n))) return rc;
  if (rs) {
    rc = upload_draws_begin(h, -1, (size_t)n);   // at most one draw per point; the stream stays locked until the commit
    if (rc) return rc;
  }
  int64_t reached = 0, kept = 0;
  rc = cut_section_enqueue(h, cs, rs, prob, h->ssn_draws.p, src, n, ox.p);
  if (!rc) rc = cut_section_wait(h, rs, &reached, &kept);
  if (rs) DrawStream::global().commit(rc ? 0 : (size_t)reached);   // one draw per point that reached the module
  if (rc) return rc;
  *n_out = kept;
  if (ox.p != static_cast<float4*>(ox.user)) { if ((rc = ox.send(h, ox.p, (size_t)kept))) return rc; }
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_icp_reading_normals(lsgpu_icp* h, const float* xyz1, int64_t n, int knn, int orient, const float sensor[3],
                              float* out_normals) {
  if (!h || !out_normals || orient < 0 || orient > 2 || (orient && !sensor)) return LSGPU_BAD_ARG;
  h->err.clear();
  // a grid of its own: a second handle with this one's configuration, on its device -- the reference stays what it was
  lsgpu_icp* tmp = nullptr;
  lsgpu_icp_config cfg = h->cfg;
  cfg.profile_kernels = 0;
  int rc = lsgpu_icp_create(&cfg, h->device, &tmp);
  if (rc) { h->err = "reading_normals: no scratch handle"; return rc; }
  const bool dev_n = is_device_ptr(out_normals);
  float* on = out_normals;
  rc = LSGPU_OK;
  if (!dev_n) { if (tmp->rd_nrm.reserve((size_t)3 * std::max<int64_t>(n, 1)) != hipSuccess) rc = LSGPU_HIP_ERROR; on = tmp->rd_nrm.p; }
  if (!rc) rc = lsgpu_icp_filter_reference_normals(tmp, xyz1, n, knn, on, nullptr, nullptr);
  if (!rc && orient) {
    const float4* src = nullptr;
    rc = stage_points(tmp, xyz1, n, tmp->flt_in, &src);
    if (!rc) {
      hipLaunchKernelGGL(k_orient_normals, dim3(nblk(n)), dim3(256), 0, tmp->stream, src, (const float4*)nullptr, (int)n,
                         sensor[0], sensor[1], sensor[2], orient, on, (float4*)nullptr);
      if (hipGetLastError() != hipSuccess) rc = LSGPU_HIP_ERROR;
    }
  }
  if (!rc && !dev_n && hipMemcpyAsync(out_normals, on, (size_t)n * 12, hipMemcpyDeviceToHost, tmp->stream) != hipSuccess) rc = LSGPU_HIP_ERROR;
  if (!rc && hipStreamSynchronize(tmp->stream) != hipSuccess) rc = LSGPU_HIP_ERROR;
  if (rc) h->err = std::string("reading_normals: ") + (tmp->err.empty() ? lsgpu_strerror(rc) : tmp->err);
  lsgpu_icp_destroy(tmp);
  return rc;
}

int lsgpu_icp_align_normals(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float* reading_normals,
                            const float T_init[16], float T_out[16], lsgpu_icp_stats* stats) {
  if (!h) return LSGPU_BAD_ARG;
  AlignExtras extras{};
  if (reading_normals && reading_xyz1 && nq > 0 && nq <= 0x7FFFFFF0ll) {
    HIPC(hipSetDevice(h->device));
    HIPC(h->rd_nrm.reserve((size_t)3 * nq));
    HIPC(hipMemcpyAsync(h->rd_nrm.p, reading_normals, (size_t)nq * 12,
                        is_device_ptr(reading_normals) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    extras.reading_normals = true;
  }
  return align_run(h, reading_xyz1, nq, T_init, T_out, stats, extras);
}

int lsgpu_icp_get_reference_normals(lsgpu_icp* h, float* out_normals, int64_t cap_points) {
  if (!h || !out_normals) return LSGPU_BAD_ARG;
  h->err.clear();
  if (h->nr <= 0 || !h->have_normals || cap_points < h->nr) { h->err = "get_reference_normals: no reference normals, or too small a buffer"; return LSGPU_BAD_ARG; }
  HIPC(hipSetDevice(h->device));
  const int64_t n = h->nr;
  const bool dev_n = is_device_ptr(out_normals);
  float* on = out_normals;
  if (!dev_n) { HIPC(h->nrm_io.reserve((size_t)3 * n)); on = h->nrm_io.p; }
  hipLaunchKernelGGL(k_snf_unpermute, dim3(nblk(n)), dim3(256), 0, h->stream, h->pts.p, (int)n, h->nrm.p, on);
  HIPC(hipGetLastError());
  if (!dev_n) HIPC(hipMemcpyAsync(out_normals, on, (size_t)n * 12, hipMemcpyDeviceToHost, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

// one reference filter module, knn in [3, 32]; or none on a point-to-point handle, which needs no normals
// (ref_carried: the reference carries normals of its own, which stand in for the module's)
static bool chain_ok(const lsgpu_icp* h, const lsgpu_chain_config* chain, bool ref_carried = false) {
  return lsgpu_chain_config_check(chain, ref_carried ? LSGPU_MINIMIZER_POINT_TO_POINT : h->cfg.error_minimizer) == LSGPU_OK;
}
// somebody behind the reference's section reads its normals: the minimizer, the robust filter's residuals, the angle filter
static bool reference_normals_read(const lsgpu_icp* h) {
  const bool rb_plane = h->mods.robust_on && h->mods.robust.distance_type == LSGPU_ROBUST_DIST_POINT2PLANE;
  const bool na_filter = h->mods.normals_on && h->mods.normals.max_angle >= 0.f;
  return h->cfg.error_minimizer != LSGPU_MINIMIZER_POINT_TO_POINT || rb_plane || na_filter;
}

}  // extern "C"

// One call of lsgpu_icp_compute: what its phases share, and the phases in the order they run -- check, start_uploads,
// filter_reference, the reading's side in one of its three places (reading_on_side_lane in front of the grid build,
// reading_with_normals before the reference takes the grid, reading_filter after it), build_reference, finish.
struct ComputeRun {
  lsgpu_icp* const h;
  const float* const reading_xyz1; const int64_t nq; const float* const reference_xyz1; const int64_t nr;   // the call's arguments
  const float* const T_init; const lsgpu_chain_config* const chain;
  // lsgpu_icp_compute_clouds_upload: the reading's H2D goes into its slot instead of the staging buffer, and the caller
  // learns whether it went out (it reads the flag after the return: the uploader is joined by then)
  float4* const upload_into; bool* const upload_enqueued;
  // carried normals (include/lsgpu_icp.h): what the reading / the reference brings along, host or device, or nullptr; ref_nrm_owned:
  // the reference's are a buffer of the handle's that this call may write (the assembled sub-map's)
  const float* const rd_carried_nrm; const float* const ref_carried_nrm; const bool ref_nrm_owned;
  section::Plan plan;   // what the sections are made of (lsgpu_section_plan.h): check() asks, filter_reference() settles it
  const lsgpu_normals_config* nc = nullptr; double t0 = 0.0;
  DrawAhead draws; std::thread uploader; hipError_t upload_err = hipSuccess;
  bool overlap_upload = false, side_used = false;   // the copy stream / the side stream has work of this call
  struct Cloud { const float4* pts; float* nrm; int64_t n; };   // points, their normals beside them (or nullptr), how many
  const float4* src = nullptr; Cloud ref{};   // the reference on the device: as given, as the grid gets it
  const float4 *rd_src = nullptr, *rd_dev = nullptr; int64_t nqf = 0;   // the reading: as given, as the loop gets it; points kept
  AlignExtras extras{};   // what finish() tells the align
  // lsgpu_icp_set_chain_cuts: the sections' cut modules.  rd_pre_cuts: some stand in front of RandomSampling, so the number of
  // draws the reading consumes is the number of points that reach it -- known when the pass's totals are on the host
  // rd_pass: the reading's section runs as one cut pass -- it has cut modules, or RandomSampling on a reading whose normals travel
  const lsgpu_chain_cuts* cuts = nullptr; bool rd_cuts = false, ref_cuts = false, rd_rs = false, rd_pre_cuts = false, rd_pass = false;
  int64_t nrc = 0; size_t rd_first_draw = 0;   // the reference's points behind its cut modules; the reading's first draw
  // every return path drains the side stream, joins the uploader and drains its stream: a pinned host reading is read by DMA,
  // and the caller may free or reuse it as soon as this call has returned, error or not (after a completed alignment the
  // copy is long over and the wait returns at once)
  ~ComputeRun() {
    if (side_used && h->side_stream) (void)hipStreamSynchronize(h->side_stream);
    if (uploader.joinable()) uploader.join();
    if (overlap_upload && h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
  }

  int check() {
    const bool ref_given = ref_carried_nrm != nullptr, rd_given = rd_carried_nrm != nullptr;
    if ((ref_given || rd_given) && h->comm) {
      h->err = "compute: carried normals are not implemented on a split-scan handle (lsgpu_icp_set_reference takes the reference's normals there)";
      return LSGPU_BAD_CONFIG;
    }
    if (!chain_ok(h, chain, ref_given)) {
      h->err = "compute: one reference filter, ssn_knn or sn_knn in [3, 32] (none only with the point-to-point minimizer)";
      return LSGPU_BAD_CONFIG;
    }
    nc = h->mods.normals_on ? &h->mods.normals : nullptr;
    // who reads the reference normals behind the section: the minimizer, the robust filter's residuals, the angle filter
    const bool rb_plane = h->mods.robust_on && h->mods.robust.distance_type == LSGPU_ROBUST_DIST_POINT2PLANE;
    const bool na_filter = nc && nc->max_angle >= 0.f;
    if (nc && (na_filter || nc->reference_orient) && chain->ssn_knn == 0 && chain->sn_knn == 0 && !ref_given) {
      h->err = "compute: SurfaceNormalOutlierFilter / OrientNormalsDataPointsFilter need the normals of a reference filter";
      return LSGPU_BAD_CONFIG;
    }
    section::Inputs in;
    in.module = chain->ssn_knn != 0 ? section::Module::Sampling : chain->sn_knn != 0 ? section::Module::SurfaceNormal : section::Module::None;
    in.normals_read = h->cfg.error_minimizer != LSGPU_MINIMIZER_POINT_TO_POINT || rb_plane || na_filter;
    in.max_density = h->mods.md_on;
    in.ref_shadow = h->mods.sh_on && h->mods.sh_cfg.reference_eps >= 0.f; in.ref_cov_sampling = h->mods.cs_on && h->mods.cs_cfg.reference_nb_sample > 0;
    in.rd_normals = nc && nc->reading_sn_knn > 0;
    in.rd_shadow = h->mods.sh_on && h->mods.sh_cfg.reading_eps >= 0.f; in.rd_cov_sampling = h->mods.cs_on && h->mods.cs_cfg.reading_nb_sample > 0;
    in.ref_carried = ref_given; in.rd_carried = rd_given && na_filter;   // (the reading's normals: the angle filter alone reads them)
    in.comm = h->comm != nullptr; in.side_switch = tuning().side_stream;
    plan = section::plan(in);
    if (plan.refusal) { h->err = plan.refusal; return LSGPU_BAD_CONFIG; }
    if (chain->seed >= 0) DrawStream::global().take(chain->seed, 0, nullptr);
    if (nq <= 0 || nr <= 0 || !reading_xyz1 || !reference_xyz1) { h->err = "compute: empty cloud"; return LSGPU_NO_CONVERGENCE; }
    if (nq > 0x7FFFFFF0ll || nr > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
    if (nr < chain->sn_knn) { h->err = "compute: the reference has fewer points than SurfaceNormalDataPointsFilter's knn"; return LSGPU_BAD_ARG; }
    HIPC(hipSetDevice(h->device));
    t0 = wall_ms();
    cuts = h->mods.cuts_on ? &h->mods.cuts : nullptr;
    rd_rs = chain->reading_prob >= 0.f;
    rd_cuts = cuts && cuts->n_reading > 0; ref_cuts = cuts && cuts->n_reference > 0;
    rd_pre_cuts = rd_cuts && rd_rs && cut_section_of(*cuts, 0, true).n_pre > 0;
    rd_pass = rd_cuts || (plan.rd_carried && rd_rs);
    return LSGPU_OK;
  }

  int start_uploads() {
    // the draws of both filters, produced on a helper thread from now on: at most one per reference point, then one per reading point
    const size_t ref_draws = plan.draws_per_reference_point() ? (size_t)nr : (size_t)0;   // (MaxDensity: one per dense point)
    int rc = draws.begin(h, -1, ref_draws + (chain->reading_prob < 0.f ? (size_t)0 : (size_t)nq), ref_draws);   // (the reference filter's share first)
    if (!rc) rc = stage_points(h, reference_xyz1, nr, h->flt_in, &src);   // (step 1 starts here)
    if (rc) return rc;
    if (is_device_ptr(reading_xyz1)) { rd_src = reinterpret_cast<const float4*>(reading_xyz1); return LSGPU_OK; }
    // A reading handed over in HOST memory crosses PCIe while the reference is being filtered: its own stream, and its own
    // host thread, because a copy from pageable memory keeps the calling thread until the last chunk is staged
    // (SURVEY.md §8d counts H2D in scans/s).  The loop's stream waits for it right before the reading filter.
    HIPC(h->copy_stream.ensure());
    HIPC(h->copy_done.ensure(hipEventDisableTiming));
    float4* up_dst = upload_into;
    if (!up_dst) { HIPC(h->flt_in2.reserve(nq)); up_dst = h->flt_in2.p; }
    overlap_upload = true; rd_src = up_dst;
    order_after_tail(h, h->copy_stream);
    // the reference's own upload goes first: it is in front of everything, the reading is not needed before the reading
    // filter, and two copies at once share the link (from pinned buffers they did: the pinned path was the slower one)
    if (src != reinterpret_cast<const float4*>(reference_xyz1)) {
      HIPC(h->ref_up_done.ensure(hipEventDisableTiming));
      HIPC(hipEventRecord(h->ref_up_done, h->stream));
      HIPC(hipStreamWaitEvent(h->copy_stream, h->ref_up_done, 0));
    }
    auto upload = [this, up_dst] {
      hipError_t e = hipSetDevice(h->device);
      if (e == hipSuccess) e = hipMemcpyAsync(up_dst, reading_xyz1, (size_t)nq * 16, hipMemcpyHostToDevice, h->copy_stream);
      if (e == hipSuccess) e = hipEventRecord(h->copy_done, h->copy_stream);
      upload_err = e;
      if (e == hipSuccess && upload_enqueued) *upload_enqueued = true;
    };
    try { uploader = std::thread(upload); }
    catch (const std::system_error&) { upload(); }   // no thread to be had: copy here (no overlap)
    return LSGPU_OK;
  }

  // the section emptied its cloud: no reference to align against
  int left_points(int64_t n) {
    if (n > 0) return LSGPU_OK;
    h->err = "compute: the reference filter left no point"; h->nr = 0;
    return LSGPU_NO_CONVERGENCE;
  }

  // SurfaceNormalDataPointsFilter on a whole cloud: its grid (no direction index of it) and the normals on it, in the grid's
  // order (h->nrm); `dens`: the densities of keepDensities 1 beside them
  int normals_on_whole_cloud(const float4* pts, int64_t n, int knn, DevBuf<float>* dens) {
    int rc = ref_build_front(h, reinterpret_cast<const float*>(pts), nullptr, n);
    if (!rc) rc = ref_build_back(h, n);
    if (rc) return rc;
    if (dens) HIPC(dens->reserve(n));
    return snf_device(h, knn, nullptr, nullptr, dens ? dens->p : nullptr);
  }

  // A thinning stage takes the section's cloud and leaves what it kept; the normals are those of the stage in front of it
  // (nullptr behind a whole cloud's grid: read in the grid's order) and go on if the plan says that somebody reads them.
  // MaxDensity: the draws of the dense points are the section's, the reading's start behind them
  int max_density_stage(Cloud& c, bool emits) {
    HIPC(h->flt_ref.reserve(c.n)); HIPC(h->flt_nrm.reserve(3 * c.n));
    int rc = draws.ready((size_t)nr);
    int64_t n_dense = 0;
    if (!rc) rc = max_density_enqueue(h, c.pts, c.n, h->dens.p, h->mods.md_cfg.max_density, h->ssn_draws.p + draws.used, emits, h->flt_ref.p, h->flt_nrm.p);
    if (!rc) rc = max_density_wait(h, &n_dense, &c.n);
    if (rc) return rc;
    draws.used += (size_t)n_dense;
    c.pts = h->flt_ref.p; c.nrm = h->flt_nrm.p;
    return left_points(c.n);
  }
  // Shadow: points and normals compacted together; behind a whole cloud's grid the gather goes through the sort's inverse
  int shadow_stage(Cloud& c) {
    const bool gathered = plan.shadow_normals == section::ShadowNormals::Gathered;
    DevBuf<float4>& pts = gathered ? h->flt_ref : h->sh_ref; DevBuf<float>& nrm = gathered ? h->flt_nrm : h->sh_nrm;
    HIPC(pts.reserve(c.n)); HIPC(nrm.reserve(3 * c.n));
    int rc = shadow_enqueue(h, c.pts, c.nrm, c.n, h->mods.sh_cfg.reference_eps, pts.p, nrm.p);
    if (!rc) rc = shadow_wait(h, &c.n);
    if (rc) return rc;
    c.pts = pts.p; c.nrm = nrm.p;
    return left_points(c.n);
  }
  // CovarianceSampling, the section's last stage: fewer points than nbSample pass unchanged
  int cov_sampling_stage(Cloud& c) {
    const int64_t nb = h->mods.cs_cfg.reference_nb_sample;
    if (nb >= c.n) return LSGPU_OK;
    HIPC(h->cs_ref.reserve(nb)); HIPC(h->cs_ref_nrm.reserve(3 * nb)); HIPC(h->cs_pick.reserve(nb));
    double sums[covs::kSums];
    const int rc = cov_sampling_run(h, c.pts, c.nrm, c.n, nb, h->mods.cs_cfg.reference_torque_norm, h->cs_ref.p, h->cs_ref_nrm.p, h->cs_pick.p, sums, nullptr);
    if (rc) { h->nr = 0; return rc; }
    c = {h->cs_ref.p, h->cs_ref_nrm.p, nb};
    return LSGPU_OK;
  }

  int filter_reference() {   // step 1: reference filter (yaml:5-7)
    nrc = nr;
    // carried normals that somebody reads: on the device, and through the cut modules with their points
    const bool carried = plan.source == section::Source::Carried;
    const float* carried_nrm = nullptr;
    if (carried) {
      const int rc = stage_in(h, ref_carried_nrm, (size_t)3 * nr, h->car_ref_nrm, &carried_nrm);
      if (rc) return rc;
    }
    if (ref_cuts) {   // the cut modules stand in front of the normals module: the reference as handed over, before anything else
      HIPC(h->cut_ref.reserve(nr));
      if (carried) HIPC(h->cut_ref_nrm.reserve((size_t)3 * nr));
      int64_t reached = 0;
      int rc = cut_section_enqueue(h, cut_section_of(*cuts, 1, false), false, 0.f, nullptr, src, nr, h->cut_ref.p,
                                   carried_nrm, carried ? h->cut_ref_nrm.p : nullptr);
      if (!rc) rc = cut_section_wait(h, false, &reached, &nrc);   // (ssn_device and ref_build_front take the count on the host)
      if (!rc) rc = left_points(nrc);
      if (rc) return rc;
      if (nrc < chain->sn_knn) { h->err = "compute: the reference has fewer points than SurfaceNormalDataPointsFilter's knn"; return LSGPU_BAD_ARG; }
      src = h->cut_ref.p;
    }
    plan = section::settle(plan, h->mods.cs_cfg.reference_nb_sample, nrc);   // (the count is on the host: the plan is final from here on)
    ref = {src, nullptr, nrc};   // (no normals module, or normals on the final grid: the reference as given, no draw)
    if (carried) {
      // the reference's orientation pair flips normals where they stand: never in a buffer of the caller's
      const bool in_place = ref_nrm_owned || carried_nrm == h->car_ref_nrm.p || !(nc && nc->reference_orient);
      if (ref_cuts) ref.nrm = h->cut_ref_nrm.p;
      else if (in_place) ref.nrm = const_cast<float*>(carried_nrm);
      else {
        HIPC(h->car_ref_nrm.reserve((size_t)3 * nr));
        HIPC(hipMemcpyAsync(h->car_ref_nrm.p, carried_nrm, (size_t)nr * 12, hipMemcpyDeviceToDevice, h->stream));
        ref.nrm = h->car_ref_nrm.p;
      }
    } else if (plan.source == section::Source::Sampling) {
      HIPC(h->flt_ref.reserve(nrc)); HIPC(h->flt_nrm.reserve(3 * nrc));
      int rc = ssn_device(h, src, nrc, chain->ssn_knn, chain->ssn_ratio, -1, h->flt_ref.p, h->flt_nrm.p, &ref.n, &draws);
      if (!rc) rc = left_points(ref.n);
      if (rc) return rc;
      ref.pts = h->flt_ref.p; ref.nrm = h->flt_nrm.p;
    } else if (plan.whole_cloud()) {
      const int rc = normals_on_whole_cloud(src, nrc, chain->sn_knn, plan.source == section::Source::WholeCloudDensities ? &h->dens : nullptr);
      if (rc) return rc;
      if (plan.normals_copied_out()) {   // in the cloud's order
        HIPC(h->cs_whole_nrm.reserve(3 * nrc));
        hipLaunchKernelGGL(k_snf_unpermute, dim3(nblk(nrc)), dim3(256), 0, h->stream, h->pts.p, (int)nrc, h->nrm.p, h->cs_whole_nrm.p);
        HIPC(hipGetLastError());
        ref.nrm = h->cs_whole_nrm.p;
      }
    }
    for (int i = 0; i < plan.n_stages; ++i) {
      const section::Stage s = plan.stages[i];
      const int rc = s == section::Stage::MaxDensity ? max_density_stage(ref, plan.emits[i])
                   : s == section::Stage::Shadow     ? shadow_stage(ref)
                                                     : cov_sampling_stage(ref);
      if (rc) return rc;
      if (!plan.emits[i]) ref.nrm = nullptr;
    }
    // the reading filter draws once per reading point, whatever it keeps: the total is known, the stream can go
    // (not with cut modules in front of RandomSampling: reading_count_wait commits then)
    if (!rd_pre_cuts) draws.commit_now(draws.used + (chain->reading_prob < 0.f ? (size_t)0 : (size_t)nq));
    return LSGPU_OK;
  }

  // step 4, on the current lane: the reading's upload, if it is ours, has to be there; then the reading filter (yaml:1-3)
  int reading_filter(bool defer_wait) {
    if (overlap_upload) {
      if (uploader.joinable()) uploader.join();
      if (upload_err != hipSuccess) { h->err = std::string("compute: reading upload: ") + hipGetErrorString(upload_err); (void)hipGetLastError(); return LSGPU_HIP_ERROR; }
      HIPC(hipStreamWaitEvent(h->lane.stream, h->copy_done, 0));
    }
    rd_dev = rd_src;
    const float* rn = nullptr;   // the reading's carried normals on the device: kept with their points into h->rd_nrm
    if (plan.rd_carried) {
      const int rc = stage_in(h, rd_carried_nrm, (size_t)3 * nq, h->car_rd_nrm, &rn);
      if (rc) return rc;
      HIPC(h->rd_nrm.reserve((size_t)3 * nq));
      extras.reading_normals = true;
    }
    if (rd_pass) {   // the section in one pass, RandomSampling (if any) inside it; the slot / the caller's cloud is only read
      HIPC(h->flt_rd.reserve(nq));
      rd_dev = h->flt_rd.p;
      const float* dr = nullptr;
      if (rd_rs) {
        rd_first_draw = draws.used;
        if (!rd_pre_cuts) draws.used = rd_first_draw + (size_t)nq;   // one draw per point; else: per point that reaches the module
        const int rcd = draws.ready();
        if (rcd) return rcd;
        dr = h->ssn_draws.p + rd_first_draw;
      }
      CutSectionDev cs;   // (RandomSampling alone: a section of no cut module)
      std::memset(&cs, 0, sizeof(cs));
      if (rd_cuts) cs = cut_section_of(*cuts, 0, rd_rs);
      const int rc = cut_section_enqueue(h, cs, rd_rs, chain->reading_prob, dr, rd_src, nq, h->flt_rd.p, rn, rn ? h->rd_nrm.p : nullptr);
      return rc || defer_wait ? rc : reading_count_wait();
    }
    if (chain->reading_prob < 0.f) {
      if (rn) HIPC(hipMemcpyAsync(h->rd_nrm.p, rn, (size_t)nq * 12, hipMemcpyDeviceToDevice, h->lane.stream));
      // no readingDataPointsFilters section: upstream runs no module at all -- every point, NO rand() call (a
      // RandomSampling module with prob 1 would consume nq draws and drop the points whose draw rounds to 1.0f)
      nqf = nq;
      return LSGPU_OK;
    }
    HIPC(h->flt_rd.reserve(nq));
    rd_dev = h->flt_rd.p;
    return random_sampling_device(h, rd_src, nq, chain->reading_prob, -1, h->flt_rd.p, &nqf, &draws, defer_wait);
  }

  // the host's wait for the number of reading points kept (current lane); with cut modules in front of RandomSampling also
  // for the number that reached it: the draws the call consumes are known, the stream can go
  int reading_count_wait() {
    if (!rd_pass) return compact_kept_wait(h, &nqf);
    int64_t reached = 0;
    const int rc = cut_section_wait(h, rd_rs, &reached, &nqf);
    if (!rc && rd_pre_cuts) { draws.used = rd_first_draw + (size_t)reached; draws.commit_now(draws.used); }
    return rc;
  }

  // The reading's side with the side stream on.  Order of the host's work (round 5, from rocprofv3's timeline of a step).
  // The host thread that enqueues both chains is the scarce resource here (~4 us per launch), and what it waits for decides
  // what idles:
  //   1. the reading's filter goes out NOW, in front of the whole grid build (it only needs the draws and the upload);
  //   2. the ordering of the queries (~25 launches) goes out while the first half of the grid build runs, right before
  //      the host waits for the grid's cell counts -- the number of reading points kept is long there;
  //   3. the second half of the grid build goes out right behind that wait;
  //   4. the move of the queries into the reference's frame (it needs the mean) behind it.
  // Before, the host enqueued the reading's whole side -- a wait and ~60 launches -- between the grid's two halves: the
  // loop's stream sat idle for 0.3 ms behind the cell counts, then the loop waited for the queries.
  // (1 is reading_on_side_lane; build_reference does 2 to 4: order_queries_on_side_lane, ref_build_back, move_queries.)
  int reading_on_side_lane() {
    // (Tried: this stream at the lowest stream priority, so that the loop's short kernels never wait for a compute unit behind
    // the direction index's build.  Measured slower, 5.27 -> 5.41..5.60 ms per compute from host buffers, level from resident
    // ones: the reading's filter and query order run here too and ARE on the critical path.)
    HIPC(h->side_stream.ensure());
    HIPC(h->side_done.ensure(hipEventDisableTiming));
    order_after_tail(h, h->side_stream); side_used = true;
    LaneScope on_side(h, h->side_lane());
    return reading_filter(/*defer_wait*/ true);
  }
  int order_queries_on_side_lane() {
    LaneScope on_side(h, h->side_lane());
    const int rc = (chain->reading_prob >= 0.f || rd_pass) ? reading_count_wait() : LSGPU_OK;   // (the number of points kept)
    return rc || nqf <= 0 ? rc : prepare_queries(h, reinterpret_cast<const float*>(rd_dev), nqf, Mat34{}, /*gather*/ false);
  }
  int move_queries() {   // the mean is known and the main stream is busy -- now the queries' side
    if (nqf <= 0) return LSGPU_OK;
    float T_rm_in[16];
    std::memcpy(T_rm_in, T_init, sizeof(T_rm_in));
    for (int d = 0; d < 3; ++d) T_rm_in[12 + d] = T_init[12 + d] - h->mean[d];   // (as the align, step 5)
    hipLaunchKernelGGL(k_query_gather, dim3(nblk(nqf)), dim3(256), 0, h->side_stream, rd_dev, nqf, h->scr_side.vals_alt.p,
                       to_mat34(T_rm_in), h->rdq.p);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(h->side_done, h->side_stream));
    extras.queries_prepared = true;
    return LSGPU_OK;
  }

  // The reading's side when its normals are wanted: the reading's filter, then SurfaceNormalDataPointsFilter on the points
  // it kept -- the grid of the kept reading (no direction index of it), the normals on it, copied out in the reading's
  // order -- all on the main stream, before the reference's own grid build
  int reading_with_normals() {
    int rc = reading_filter(false);
    if (rc) return rc;
    if (nqf <= 0) { h->err = "compute: the reading filter left no point"; return LSGPU_NO_CONVERGENCE; }
    if (nqf < nc->reading_sn_knn) { h->err = "compute: the kept reading has fewer points than SurfaceNormalDataPointsFilter's knn"; return LSGPU_BAD_ARG; }
    rc = normals_on_whole_cloud(rd_dev, nqf, nc->reading_sn_knn, nullptr);
    if (rc) return rc;
    HIPC(h->rd_nrm.reserve((size_t)3 * nqf));
    float* rn = h->rd_nrm.p;   // (ShadowDataPointsFilter behind them: a buffer in front of the pass, which writes h->rd_nrm)
    if (plan.rd_shadow) { HIPC(h->sh_rd_nrm.reserve((size_t)3 * nqf)); rn = h->sh_rd_nrm.p; }
    hipLaunchKernelGGL(k_snf_unpermute, dim3(nblk(nqf)), dim3(256), 0, h->stream, h->pts.p, (int)nqf, h->nrm.p, rn);
    if (nc->reading_orient)
      hipLaunchKernelGGL(k_orient_normals, dim3(nblk(nqf)), dim3(256), 0, h->stream, rd_dev, (const float4*)nullptr, (int)nqf,
                         nc->reading_sensor[0], nc->reading_sensor[1], nc->reading_sensor[2], nc->reading_orient, rn, (float4*)nullptr);
    HIPC(hipGetLastError());
    if (plan.rd_shadow) {   // the loop and the angle filter see the kept points and their normals from here on
      HIPC(h->sh_rd.reserve(nqf));
      rc = shadow_enqueue(h, rd_dev, rn, nqf, h->mods.sh_cfg.reading_eps, h->sh_rd.p, h->rd_nrm.p);
      if (!rc) rc = shadow_wait(h, &nqf);
      if (rc) return rc;
      if (nqf <= 0) { h->err = "compute: the reading filter left no point"; return LSGPU_NO_CONVERGENCE; }
      rd_dev = h->sh_rd.p;
    }
    if (plan.rd_cov_sampling && h->mods.cs_cfg.reading_nb_sample < nqf) {   // behind the normals, their orientation and the Shadow pass
      const int64_t nb = h->mods.cs_cfg.reading_nb_sample;
      HIPC(h->cs_rd.reserve(nb)); HIPC(h->cs_rd_nrm.reserve(3 * nb)); HIPC(h->cs_pick.reserve(nb));
      double sums[covs::kSums];
      rc = cov_sampling_run(h, rd_dev, h->rd_nrm.p, nqf, nb, h->mods.cs_cfg.reading_torque_norm, h->cs_rd.p, h->cs_rd_nrm.p, h->cs_pick.p, sums, nullptr);
      if (rc) { h->nr = 0; return rc; }   // (the grid the handle holds is the reading's: no reference to align against)
      HIPC(hipMemcpyAsync(h->rd_nrm.p, h->cs_rd_nrm.p, (size_t)nb * 12, hipMemcpyDeviceToDevice, h->stream));   // (where the loop reads them)
      rd_dev = h->cs_rd.p; nqf = nb;
    }
    extras.reading_normals = true;
    return LSGPU_OK;
  }

  // steps 2-3: the reference's grid, the queries' side between and behind its halves, and the normals the chain computes on it
  int build_reference() {
    if (nc && nc->reference_orient && ref.nrm)   // the sampling filter's normals, beside its points
      hipLaunchKernelGGL(k_orient_normals, dim3(nblk(ref.n)), dim3(256), 0, h->stream, ref.pts, (const float4*)nullptr, (int)ref.n,
                         nc->reference_sensor[0], nc->reference_sensor[1], nc->reference_sensor[2], nc->reference_orient, ref.nrm, (float4*)nullptr);
    int rc = ref_build_front(h, reinterpret_cast<const float*>(ref.pts), ref.nrm, ref.n);
    if (!rc && plan.side) rc = order_queries_on_side_lane();
    if (!rc) rc = ref_build_back(h, ref.n);
    if (!rc && plan.side) rc = move_queries();
    if (!rc && !plan.side) rc = build_cone_index(h);
    if (!rc && plan.normals_on_final_grid) rc = snf_device(h, chain->sn_knn, nullptr, nullptr);
    if (rc) return rc;
    if (plan.normals_on_final_grid) {
      h->have_normals = true;
      if (nc && nc->reference_orient) {   // on the sorted normals; the position is the point as given (ref.pts, by the sorted point's index)
        hipLaunchKernelGGL(k_orient_normals, dim3(nblk(ref.n)), dim3(256), 0, h->stream, ref.pts, h->pts.p, (int)ref.n,
                           nc->reference_sensor[0], nc->reference_sensor[1], nc->reference_sensor[2], nc->reference_orient, (float*)nullptr, h->nrm.p);
        HIPC(hipGetLastError());
      }
    }
    if (plan.side) {
      // the direction index of the reference is not needed before the loop's third search: the align enqueues its
      // build on the side stream (behind the queries' order, with that stream's sort scratch) once the loop's first
      // iteration is out -- beside the first two iterations instead of in front of the loop (0.16 ms per 1 M-point
      // compute), and without holding the host back from starting the loop (round 5)
      HIPC(h->cone_done.ensure(hipEventDisableTiming));
      extras.build_index_on_side = true;
    }
    return LSGPU_OK;
  }

  int finish(float T_out[16], lsgpu_icp_stats* stats) {   // steps 5-7
    draws.finish();
    const double t_filters = wall_ms() - t0;
    if (nqf <= 0) { h->err = "compute: the reading filter left no point"; return LSGPU_NO_CONVERGENCE; }
    const int rc = align_run(h, reinterpret_cast<const float*>(rd_dev), nqf, T_init, T_out, stats, extras);
    if (stats) stats->t_reserved[0] = t_filters;
    return rc;
  }
};

// lsgpu_icp_compute, told by lsgpu_icp_compute_clouds_upload where the reading's upload goes (nullptr, nullptr otherwise)
static int compute_run(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float* reference_xyz1, int64_t nr,
                       const float T_init[16], const lsgpu_chain_config* chain, float T_out[16], lsgpu_icp_stats* stats,
                       float4* upload_into, bool* upload_enqueued, const float* reading_normals = nullptr,
                       const float* reference_normals = nullptr, bool ref_nrm_owned = false) {
  if (!h || !T_init || !T_out || !chain) return LSGPU_BAD_ARG;
  h->err.clear();
  std::memcpy(T_out, T_init, 16 * sizeof(float));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  ComputeRun run{h, reading_xyz1, nq, reference_xyz1, nr, T_init, chain, upload_into, upload_enqueued, reading_normals, reference_normals, ref_nrm_owned};
  int rc = run.check();
  if (!rc) rc = run.start_uploads();
  if (!rc) rc = run.filter_reference();
  if (!rc && run.plan.side) rc = run.reading_on_side_lane();
  if (!rc && run.plan.rd_normals) rc = run.reading_with_normals();
  if (!rc) rc = run.build_reference();
  if (!rc && !run.plan.side && !run.plan.rd_normals) rc = run.reading_filter(false);   // (the reading's side after the grid build)
  return rc ? rc : run.finish(T_out, stats);
}

extern "C" {

int lsgpu_icp_compute(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float* reference_xyz1,
                      int64_t nr, const float T_init[16], const lsgpu_chain_config* chain,
                      float T_out[16], lsgpu_icp_stats* stats) {
  return compute_run(h, reading_xyz1, nq, reference_xyz1, nr, T_init, chain, T_out, stats, nullptr, nullptr);
}

int lsgpu_icp_compute_normals(lsgpu_icp* h, const float* reading_xyz1, const float* reading_normals, int64_t nq,
                              const float* reference_xyz1, const float* reference_normals, int64_t nr, const float T_init[16],
                              const lsgpu_chain_config* chain, float T_out[16], lsgpu_icp_stats* stats) {
  return compute_run(h, reading_xyz1, nq, reference_xyz1, nr, T_init, chain, T_out, stats, nullptr, nullptr, reading_normals, reference_normals);
}

int lsgpu_filter_cylinder(lsgpu_icp* h, const float* xyz1, int64_t n, const float center[3], double radius_m,
                          double height_m, int remove_point_inside, float* out_xyz1, int64_t* n_out) {
  if (!h || !n_out || !center || !out_xyz1) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  if (n <= 0 || !xyz1) return LSGPU_OK;
  if (n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (rc) return rc;
  OutStage<float4> ox;
  if ((rc = ox.open(h, out_xyz1, h->flt_rd, n))) return rc;
  HIPC(h->ssn_keep.reserve(n));
  HIPC(h->ssn_out_pos.reserve(n));
  hipLaunchKernelGGL(k_cylinder_select, dim3(nblk(n)), dim3(256), 0, h->stream, src, (int)n, center[0], center[1],
                     center[2], radius_m * radius_m, height_m / 2.0, remove_point_inside, h->ssn_keep.p);
  rc = compact_kept(h, src, n, ox.p, n_out);
  if (rc) return rc;
  if ((rc = ox.copy_back(h, *n_out))) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_filter_voxel_grid(lsgpu_icp* h, const float* xyz1, int64_t n, const float leaf[3], int min_points,
                            float* out_xyz1, int64_t* n_out) {
  if (!h || !n_out || !leaf || !out_xyz1) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  if (!(leaf[0] > 0.f && leaf[1] > 0.f && leaf[2] > 0.f)) { h->err = "voxel_grid: leaf size must be positive"; return LSGPU_BAD_ARG; }
  if (n <= 0 || !xyz1) return LSGPU_OK;
  if (n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (rc) return rc;
  float lo[3], hi[3];   // getMinMax3D
  rc = cloud_bounds(h, src, n, lo, hi);
  if (rc) return rc;
  float inv[3];
  int minb[3], divb[3];
  for (int d = 0; d < 3; ++d) {
    inv[d] = 1.0f / leaf[d];
    minb[d] = (int)std::floor(lo[d] * inv[d]);
    const int maxb = (int)std::floor(hi[d] * inv[d]);
    divb[d] = maxb - minb[d] + 1;
  }
  if ((int64_t)divb[0] * (int64_t)divb[1] * (int64_t)divb[2] > 2147483647ll) {
    h->err = "voxel_grid: leaf size too small for the cloud, the voxel index would overflow";
    return LSGPU_BAD_ARG;
  }
  HIPC(h->lane.scratch->keys.reserve(n));
  HIPC(h->lane.scratch->vals.reserve(n));
  HIPC(h->ssn_keep.reserve(n));
  HIPC(h->ssn_out_pos.reserve(n));
  HIPC(h->ssn_seg_of.reserve(n));   // voxel head flags
  HIPC(h->flt_ref.reserve(n));      // centroids by sorted position
  hipLaunchKernelGGL(k_voxel_keys, dim3(nblk(n)), dim3(256), 0, h->stream, src, (int)n, inv[0], inv[1], inv[2],
                     minb[0], minb[1], minb[2], divb[0], divb[0] * divb[1], h->lane.scratch->keys.p, h->lane.scratch->vals.p);
  rc = sort_pairs(h, n, 31);  // stable: equal voxels keep input order
  if (rc) return rc;
  hipLaunchKernelGGL(k_voxel_heads, dim3(nblk(n)), dim3(256), 0, h->stream, h->lane.scratch->keys_alt.p, (int)n, h->ssn_seg_of.p);
  hipLaunchKernelGGL(k_voxel_centroids, dim3(nblk(n)), dim3(256), 0, h->stream, src, h->lane.scratch->keys_alt.p, h->lane.scratch->vals_alt.p, (int)n,
                     min_points, h->ssn_seg_of.p, h->flt_ref.p, h->ssn_keep.p);
  OutStage<float4> ox;
  if ((rc = ox.open(h, out_xyz1, h->flt_rd, n))) return rc;
  rc = compact_kept(h, h->flt_ref.p, n, ox.p, n_out);
  if (rc) return rc;
  if ((rc = ox.copy_back(h, *n_out))) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

// VoxelGridDataPointsFilter (include/lsgpu_icp.h, "the input filter chain"): src (m points, device) -> dst (device, room for
// m; none of src and h->vgf_out), one point per occupied voxel in the order of the voxels' first points.  No draw.
static int voxel_grid_filter_device(lsgpu_icp* h, const float4* src, int64_t m, const lsgpu_point_filter& f, float4* dst,
                                    int64_t* m_out) {
  // the cloud's minimum and maximum, and with them the verdict on its finiteness
  float lo[3], hi[3];
  int rc = cloud_bounds(h, src, m, lo, hi);
  if (rc) return rc;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) {
      h->err = "apply_point_filters: VoxelGridDataPointsFilter was handed a NaN or infinite coordinate; put RemoveNaNDataPointsFilter "
               "(and a MaxDist / BoundingBox filter against infinities) in front of it";
      return LSGPU_BAD_ARG;
    }
  }
  voxelf::Geom g;
  if (voxelf::make_geom(lo, hi, f.v, &g) != LSGPU_OK) {
    h->err = "apply_point_filters: VoxelGridDataPointsFilter: too many voxels (more than 2^31 - 1) for this cloud, the voxel sizes are too small";
    return LSGPU_BAD_CONFIG;
  }
  const uint32_t nvox = g.ndiv[0] * g.ndiv[1] * g.ndiv[2];
  int nbits = 1;
  while (nbits < 31 && (nvox - 1u) >> nbits) ++nbits;
  HIPC(h->lane.scratch->keys.reserve(m));
  HIPC(h->lane.scratch->vals.reserve(m));
  HIPC(h->vgf_out.reserve(m));
  hipLaunchKernelGGL(k_vgf_keys, dim3(nblk(m)), dim3(256), 0, h->stream, src, (int)m, g, h->lane.scratch->keys.p, h->lane.scratch->vals.p);
  rc = sort_pairs(h, m, nbits);  // stable: the points of a voxel keep input order
  if (rc) return rc;
  hipLaunchKernelGGL(k_vgf_reduce, dim3(nblk(m)), dim3(256), 0, h->stream, src, h->lane.scratch->keys_alt.p, h->lane.scratch->vals_alt.p, (int)m, g,
                     f.flag ? 1 : 0, h->vgf_out.p, h->ssn_keep.p);
  return compact_kept(h, h->vgf_out.p, m, dst, m_out);
}

// ... the launches of OctreeGridDataPointsFilter behind the root box: path keys, their sort, leaves, ranks, the sort by leaf
// rank from input order, one point per leaf at the front of dst, the number of leaves on its way to the host
static int octree_grid_enqueue(lsgpu_icp* h, const float4* src, int64_t m, const octreef::Root& g, uint32_t max_point, int method,
                               float4* dst) {
  hipLaunchKernelGGL(k_ogf_keys, dim3(nblk(m)), dim3(256), 0, h->stream, src, (int)m, g, h->lane.scratch->keys.p, h->lane.scratch->vals.p);
  int rc = sort_pairs(h, m, 3 * g.depth);  // the nodes of every depth in depth-first order (equal paths keep input order)
  if (rc) return rc;
  hipLaunchKernelGGL(k_ogf_leaves, dim3(nblk(m)), dim3(256), 0, h->stream, h->lane.scratch->keys_alt.p, (int)m, g.depth, max_point, h->ssn_keep.p);
  rc = scan_u32(h, h->ssn_keep.p, h->ssn_out_pos.p, (size_t)m, false, true);   // (the heads' words are not 1: they count as 1)
  if (rc) return rc;
  // (the path sort's result is in keys_alt / vals_alt: the other pair is free, and it is the next sort's input)
  hipLaunchKernelGGL(k_ogf_regroup, dim3(nblk(m)), dim3(256), 0, h->stream, h->lane.scratch->vals_alt.p, h->ssn_keep.p, h->ssn_out_pos.p, (int)m,
                     h->lane.scratch->keys.p, h->lane.scratch->vals.p);
  int rank_bits = 0;   // a leaf's rank is < m
  while (rank_bits < 31 && ((uint64_t)(m - 1) >> rank_bits)) ++rank_bits;
  rc = sort_pairs(h, m, rank_bits);  // stable, from input order: a leaf's points in ascending input index
  if (rc) return rc;
  hipLaunchKernelGGL(k_ogf_sample, dim3(nblk(m)), dim3(256), 0, h->stream, src, h->lane.scratch->keys_alt.p, h->lane.scratch->vals_alt.p, (int)m,
                     h->ssn_keep.p, method, h->ssn_draws.p, dst);
  HIPC(hipGetLastError());
  return scan_totals_enqueue(h, nullptr, nullptr, 0, h->ssn_keep.p, h->ssn_out_pos.p, (size_t)m);
}

// OctreeGridDataPointsFilter (include/lsgpu_icp.h, "the input filter chain"): src (m points, device) -> dst (device, room for
// m, not src), one point per non-empty leaf in depth-first order.  RandomPts: one draw per leaf -- their number is known on
// the device only, so up to m draws are uploaded and the stream is committed with the count once it is on the host (the rule
// of the pass behind MaxDensityDataPointsFilter).
static int octree_grid_filter_device(lsgpu_icp* h, const float4* src, int64_t m, const lsgpu_point_filter& f, float4* dst,
                                     int64_t* m_out) {
  float lo[3], hi[3];
  int rc = cloud_bounds(h, src, m, lo, hi);
  if (rc) return rc;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a])) {
      h->err = "apply_point_filters: OctreeGridDataPointsFilter was handed a NaN or infinite coordinate; put RemoveNaNDataPointsFilter "
               "(and a MaxDist / BoundingBox filter against infinities) in front of it";
      return LSGPU_BAD_ARG;
    }
  }
  octreef::Root g;
  octreef::make_root(lo, hi, f.v[0], &g);
  const bool draws = f.dim == octreef::kRandomPts;
  HIPC(h->lane.scratch->keys.reserve(m));
  HIPC(h->lane.scratch->vals.reserve(m));
  HIPC(h->ssn_draws.reserve((size_t)m + 1));
  if (draws) {
    rc = upload_draws_begin(h, -1, (size_t)m);   // at most one draw per point; the stream stays locked until the commit
    if (rc) return rc;
  }
  rc = octree_grid_enqueue(h, src, m, g, (uint32_t)f.v[1], f.dim, dst);
  uint32_t unused = 0, n_leaves = 0;
  if (!rc) rc = scan_totals_wait(h, &unused, &n_leaves, true);
  if (draws) DrawStream::global().commit(rc ? 0 : (size_t)n_leaves);   // one draw per non-empty leaf
  if (rc) return rc;
  *m_out = n_leaves;
  return LSGPU_OK;
}

// the parameter checks of lsgpu_apply_point_filters (and of lsgpu_cloud_ingest): LSGPU_OK, or LSGPU_BAD_CONFIG with the text
static int point_filters_check(lsgpu_icp* h, const lsgpu_point_filter* filters, int n_filters) {
  for (int k = 0; k < n_filters; ++k) {
    const lsgpu_point_filter& f = filters[k];
    const bool ok = (f.type == LSGPU_FILTER_MAX_DIST || f.type == LSGPU_FILTER_MIN_DIST) ? (f.dim >= -1 && f.dim <= 2)
                    : f.type == LSGPU_FILTER_BOUNDING_BOX ? true
                    : f.type == LSGPU_FILTER_FIX_STEP_SAMPLING ? (f.v[0] >= 1.f && f.v[1] >= 1.f && f.v[2] > 0.f)
                    : f.type == LSGPU_FILTER_RANDOM_SAMPLING ? (f.v[0] >= 0.f && f.v[0] <= 1.f)
                    : f.type == LSGPU_FILTER_REMOVE_NAN ? true
                    : f.type == LSGPU_FILTER_VOXEL_GRID ? true
                    : f.type == LSGPU_FILTER_OCTREE_GRID ? true : false;
    if (ok && f.type == LSGPU_FILTER_OCTREE_GRID) {
      if (const char* why = octreef::why_bad_params(f.v[0], f.v[1], f.dim, f.flag)) { h->err = std::string("apply_point_filters: ") + why; return LSGPU_BAD_CONFIG; }
    }
    if (ok && f.type == LSGPU_FILTER_VOXEL_GRID) {
      if (const char* why = voxelf::why_bad_params(f.v, f.flag, f.dim)) { h->err = std::string("apply_point_filters: ") + why; return LSGPU_BAD_CONFIG; }
    }
    if (!ok) { h->err = "apply_point_filters: unknown filter type or parameter out of range"; return LSGPU_BAD_CONFIG; }
  }
  return LSGPU_OK;
}

// The point modules of a chain on a staged cloud (`src`, n > 0 points on the device): the kept cloud is *out (src itself
// for an empty chain, else one of the handle's two filter buffers), *m_out points, enqueued on the handle's stream.
// Draws and FixStepSampling's `state` move as lsgpu_apply_point_filters documents; both of its callers are this function.
static int point_filters_run(lsgpu_icp* h, lsgpu_point_filter* filters, int n_filters, const float4* src, int64_t n,
                             const float4** out, int64_t* m_out) {
  const float4* cur = src;
  int rc = LSGPU_OK;
  HIPC(h->flt_ref.reserve(n));
  HIPC(h->flt_rd.reserve(n));
  HIPC(h->ssn_keep.reserve(n));
  HIPC(h->ssn_out_pos.reserve(n));
  float4* ping = h->flt_ref.p;
  float4* pong = h->flt_rd.p;
  int64_t m = n;
  for (int k = 0; k < n_filters; ++k) {
    lsgpu_point_filter& f = filters[k];
    if (m == 0) { h->err = "apply_point_filters: no points to filter"; return LSGPU_NO_CONVERGENCE; }
    if (f.type == LSGPU_FILTER_VOXEL_GRID || f.type == LSGPU_FILTER_OCTREE_GRID) {
      rc = f.type == LSGPU_FILTER_VOXEL_GRID ? voxel_grid_filter_device(h, cur, m, f, ping, &m) : octree_grid_filter_device(h, cur, m, f, ping, &m);
      if (rc) return rc;
      cur = ping;
      std::swap(ping, pong);
      continue;
    }
    PointFilterDev d;
    std::memset(&d, 0, sizeof(d));
    d.type = f.type; d.dim = f.dim; d.flag = f.flag;
    for (int i = 0; i < 6; ++i) d.v[i] = f.v[i];
    d.step = 1; d.phase = 0;
    if (f.type == LSGPU_FILTER_FIX_STEP_SAMPLING) {
      double step = f.state > 0.0 ? f.state : (double)f.v[0];
      const int istep = std::max(1, (int)step);
      d.step = (uint32_t)istep;
      d.phase = DrawStream::global().take_raw(-1) % (uint32_t)istep;  // rand() % iStep
      const double delta = (double)f.v[0] * (double)f.v[2] - (double)f.v[0];
      step *= (double)f.v[2];
      if (delta >= 0 && step > (double)f.v[1]) step = (double)f.v[1];
      if (delta < 0 && step < (double)f.v[1]) step = (double)f.v[1];
      f.state = step;
    } else if (f.type == LSGPU_FILTER_RANDOM_SAMPLING) {
      rc = upload_draws_begin(h, -1, (size_t)m);
      if (rc) return rc;
      DrawStream::global().commit((size_t)m);  // one draw per point
    }
    hipLaunchKernelGGL(k_point_filter_select, dim3(nblk(m)), dim3(256), 0, h->stream, cur, (int)m, d, h->ssn_draws.p,
                       h->ssn_keep.p);
    rc = compact_kept(h, cur, m, ping, &m);
    if (rc) return rc;
    cur = ping;
    std::swap(ping, pong);
  }
  *out = cur;
  *m_out = m;
  return LSGPU_OK;
}

int lsgpu_apply_point_filters(lsgpu_icp* h, lsgpu_point_filter* filters, int n_filters, const float* xyz1,
                              int64_t n, int64_t seed, float* out_xyz1, int64_t* n_out) {
  if (!h || !n_out || n_filters < 0 || (n_filters > 0 && !filters) || n < 0 || (n > 0 && (!xyz1 || !out_xyz1))) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  if (n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  int rc = point_filters_check(h, filters, n_filters);
  if (rc) return rc;
  if (seed >= 0) DrawStream::global().take(seed, 0, nullptr);
  // DataPointsFilters::apply: an empty CHAIN is a no-op; otherwise the first filter that is handed an empty cloud throws
  // ConvergenceError("no points to filter") -- also when the cloud came in empty
  if (n == 0) {
    if (n_filters == 0) return LSGPU_OK;
    h->err = "apply_point_filters: no points to filter";
    return LSGPU_NO_CONVERGENCE;
  }
  HIPC(hipSetDevice(h->device));
  const float4* cur = nullptr;
  rc = stage_points(h, xyz1, n, h->flt_in, &cur);
  if (rc) return rc;
  int64_t m = 0;
  rc = point_filters_run(h, filters, n_filters, cur, n, &cur, &m);
  if (rc) return rc;
  *n_out = m;
  if (m) HIPC(hipMemcpyAsync(out_xyz1, cur, (size_t)m * 16, hipMemcpyDefault, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_cloud_from_pointcloud2(lsgpu_icp* h, const unsigned char* data, int64_t n, int point_step, int off_x,
                                 int off_y, int off_z, int is_bigendian, int drop_non_finite, float* out_xyz1,
                                 int64_t* n_out) {
  if (!h || !n_out || n < 0 || (n > 0 && (!data || !out_xyz1))) return LSGPU_BAD_ARG;
  h->err.clear();
  *n_out = 0;
  const int lo = std::min(off_x, std::min(off_y, off_z)), hi = std::max(off_x, std::max(off_y, off_z));
  if (point_step < 12 || lo < 0 || hi + 4 > point_step) { h->err = "from_pointcloud2: x/y/z fields do not fit a record"; return LSGPU_BAD_ARG; }
  if (n == 0) return LSGPU_OK;
  if (n > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  HIPC(hipSetDevice(h->device));
  const unsigned char* src = data;
  if (!is_device_ptr(data)) {  // the message's byte block crosses PCIe once, as it is
    HIPC(h->lane.scratch->sort_tmp.reserve((size_t)n * (size_t)point_step));
    HIPC(hipMemcpyAsync(h->lane.scratch->sort_tmp.p, data, (size_t)n * (size_t)point_step, hipMemcpyHostToDevice, h->stream));
    src = reinterpret_cast<const unsigned char*>(h->lane.scratch->sort_tmp.p);
  }
  HIPC(h->flt_in.reserve(n));
  HIPC(h->ssn_keep.reserve(n));
  HIPC(h->ssn_out_pos.reserve(n));
  hipLaunchKernelGGL(k_pc2_unpack, dim3(nblk(n)), dim3(256), 0, h->stream, src, (int)n, point_step, off_x, off_y, off_z,
                     is_bigendian ? 1 : 0, drop_non_finite ? 1 : 0, h->flt_in.p, h->ssn_keep.p);
  OutStage<float4> ox;   // (the result is unpacked, and compacted, in the handle's buffers whatever the caller's is)
  ox.classify(out_xyz1);
  int64_t m = n;
  const float4* res = h->flt_in.p;
  if (drop_non_finite) {
    HIPC(h->flt_rd.reserve(n));
    const int rc = compact_kept(h, h->flt_in.p, n, h->flt_rd.p, &m);
    if (rc) return rc;
    res = h->flt_rd.p;
  }
  HIPC(hipGetLastError());
  *n_out = m;
  const int rc = ox.send(h, res, (size_t)m);
  if (rc) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

int lsgpu_cloud_to_pointxyz(lsgpu_icp* h, const float* xyz1, int64_t n, unsigned char* out_data) {
  if (!h || n < 0 || (n > 0 && (!xyz1 || !out_data))) return LSGPU_BAD_ARG;
  h->err.clear();
  if (n == 0) return LSGPU_OK;
  HIPC(hipSetDevice(h->device));
  const float4* src = nullptr;
  int rc = stage_points(h, xyz1, n, h->flt_in, &src);
  if (rc) return rc;
  OutStage<float4> dst;
  if ((rc = dst.open(h, out_data, h->flt_rd, n))) return rc;
  hipLaunchKernelGGL(k_pc2_pack, dim3(nblk(n)), dim3(256), 0, h->stream, src, n, dst.p);
  HIPC(hipGetLastError());
  if ((rc = dst.copy_back(h, n))) return rc;
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

// the slot exists, holds nothing and carries no normals (whatever it held is gone from here on: a failed copy must not leave
// a half-written cloud behind)
static void cloud_slot_clear(lsgpu_icp* h, int slot) {
  if ((size_t)slot >= h->clouds.size()) { h->clouds.resize((size_t)slot + 1); h->cloud_n.resize((size_t)slot + 1, -1); }
  if (h->cloud_nrm.size() < h->clouds.size()) { h->cloud_nrm.resize(h->clouds.size()); h->cloud_has_nrm.resize(h->clouds.size(), 0); }
  h->cloud_n[slot] = -1;
  h->cloud_has_nrm[slot] = 0;
}
static bool cloud_has_normals(const lsgpu_icp* h, int slot) {
  return slot >= 0 && (size_t)slot < h->cloud_has_nrm.size() && h->cloud_n[slot] >= 0 && h->cloud_has_nrm[slot] != 0;
}

int lsgpu_cloud_upload_normals(lsgpu_icp* h, int slot, const float* xyz1, const float* normals, int64_t n) {
  if (!h || slot < 0 || slot >= (1 << 20) || n < 0 || n > 0x7FFFFFF0ll || (n > 0 && !xyz1)) return LSGPU_BAD_ARG;
  h->err.clear();
  HIPC(hipSetDevice(h->device));
  cloud_slot_clear(h, slot);
  HIPC(h->clouds[slot].reserve(n ? n : 1));
  if (normals) HIPC(h->cloud_nrm[slot].reserve(n ? (size_t)3 * n : 1));
  if (n) HIPC(hipMemcpyAsync(h->clouds[slot].p, xyz1, (size_t)n * 16, hipMemcpyDefault, h->stream));
  if (n && normals) HIPC(hipMemcpyAsync(h->cloud_nrm[slot].p, normals, (size_t)n * 12, hipMemcpyDefault, h->stream));
  HIPC(hipStreamSynchronize(h->stream));  // the caller's buffers are free again on return
  h->cloud_n[slot] = n;
  h->cloud_has_nrm[slot] = normals ? 1 : 0;
  return LSGPU_OK;
}

int lsgpu_cloud_upload(lsgpu_icp* h, int slot, const float* xyz1, int64_t n) {
  return lsgpu_cloud_upload_normals(h, slot, xyz1, nullptr, n);
}

int lsgpu_cloud_has_normals(lsgpu_icp* h, int slot, int* has) {
  if (!h || !has || slot < 0) return LSGPU_BAD_ARG;
  *has = cloud_has_normals(h, slot) ? 1 : 0;
  return LSGPU_OK;
}

int lsgpu_cloud_release(lsgpu_icp* h, int slot) {
  if (!h || slot < 0) return LSGPU_BAD_ARG;
  if ((size_t)slot >= h->clouds.size() || h->cloud_n[slot] < 0) return LSGPU_OK;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->clouds[slot].release();
  if ((size_t)slot < h->cloud_nrm.size()) { h->cloud_nrm[slot].release(); h->cloud_has_nrm[slot] = 0; }
  h->cloud_n[slot] = -1;
  return LSGPU_OK;
}

int lsgpu_cloud_size(lsgpu_icp* h, int slot, int64_t* n) {
  if (!h || !n || slot < 0) return LSGPU_BAD_ARG;
  *n = (size_t)slot < h->clouds.size() ? h->cloud_n[slot] : -1;
  return LSGPU_OK;
}

// the device half of lsgpu_cloud_ingest; the caller has cleared the slot and confirms it on LSGPU_OK
static int cloud_ingest_run(lsgpu_icp* h, int slot, lsgpu_point_filter* filters, int n_filters, const float* xyz1, int64_t n,
                            int normals_knn, int orient, const float sensor[3], int64_t* kept) {
  const float4* cur = nullptr;
  int64_t m = 0;
  if (n == 0) {
    if (n_filters) { h->err = "apply_point_filters: no points to filter"; return LSGPU_NO_CONVERGENCE; }
  } else {
    int rc = stage_points(h, xyz1, n, h->flt_in, &cur);
    if (!rc) rc = point_filters_run(h, filters, n_filters, cur, n, &cur, &m);
    if (rc) return rc;
  }
  *kept = m;
  HIPC(h->clouds[slot].reserve(m ? m : 1));
  if (!normals_knn) {
    if (m) HIPC(hipMemcpyAsync(h->clouds[slot].p, cur, (size_t)m * 16, hipMemcpyDeviceToDevice, h->stream));
    return LSGPU_OK;
  }
  // lsgpu_icp_reading_normals on the kept cloud where it lies: its texts, the grid on this handle
  const char* why = m < normals_knn ? "filter_reference_normals: the cloud has fewer points than knn"
                    : m > 0x7FFFFFF0ll / normals_knn ? "filter_reference_normals: knn x n exceeds the 32-bit pair count" : nullptr;
  if (why) { h->err = std::string("reading_normals: ") + why; return LSGPU_BAD_ARG; }
  int rc = lsgpu_icp_set_reference(h, reinterpret_cast<const float*>(cur), nullptr, m);
  if (!rc) rc = snf_device(h, normals_knn, nullptr, nullptr);
  if (rc) { h->err = std::string("reading_normals: ") + (h->err.empty() ? lsgpu_strerror(rc) : h->err); return rc; }
  HIPC(h->cloud_nrm[slot].reserve((size_t)3 * m));
  const float s3[3] = {orient ? sensor[0] : 0.f, orient ? sensor[1] : 0.f, orient ? sensor[2] : 0.f};
  hipLaunchKernelGGL(k_ingest_store, dim3(nblk(m)), dim3(256), 0, h->stream, cur, (int)m, (const uint32_t*)h->ref_inv.p,
                     (const float4*)h->nrm.p, s3[0], s3[1], s3[2], orient, h->clouds[slot].p, h->cloud_nrm[slot].p);
  HIPC(hipGetLastError());
  return LSGPU_OK;
}

int lsgpu_cloud_ingest(lsgpu_icp* h, int slot, lsgpu_point_filter* filters, int n_filters, const float* xyz1, int64_t n,
                       int64_t seed, int normals_knn, int orient, const float sensor[3], float* out_xyz1, float* out_normals,
                       int64_t* n_out) {
  if (!h || slot < 0 || slot >= (1 << 20) || n_filters < 0 || (n_filters > 0 && !filters) || n < 0 || n > 0x7FFFFFF0ll ||
      (n > 0 && !xyz1))
    return LSGPU_BAD_ARG;
  h->err.clear();
  if (n_out) *n_out = 0;
  int rc = point_filters_check(h, filters, n_filters);
  if (rc) return rc;
  if (normals_knn != 0 && (normals_knn < kSnfMinKnn || normals_knn > kSnfMaxKnn)) { h->err = "cloud_ingest: normals_knn must be 0 or in [3, 32]"; return LSGPU_BAD_ARG; }
  if (orient < 0 || orient > 2) { h->err = "cloud_ingest: orient must be 0, 1 or 2"; return LSGPU_BAD_ARG; }
  if (orient && !sensor) { h->err = "cloud_ingest: orient needs the sensor position"; return LSGPU_BAD_ARG; }
  if (orient && !normals_knn) { h->err = "cloud_ingest: orient needs normals (normals_knn > 0)"; return LSGPU_BAD_ARG; }
  if (out_normals && !normals_knn) { h->err = "cloud_ingest: out_normals needs normals (normals_knn > 0)"; return LSGPU_BAD_ARG; }
  if (normals_knn && h->comm) {
    h->err = "cloud_ingest: normals are not implemented on a split-scan handle (carried normals are refused there)";
    return LSGPU_BAD_CONFIG;
  }
  if (seed >= 0) DrawStream::global().take(seed, 0, nullptr);
  HIPC(hipSetDevice(h->device));
  cloud_slot_clear(h, slot);
  int64_t m = 0;
  rc = cloud_ingest_run(h, slot, filters, n_filters, xyz1, n, normals_knn, orient, sensor, &m);
  if (rc) { if (n_out) *n_out = m; return rc; }   // (what the point modules kept, where the normals' step refused it)
  if (m && out_xyz1) HIPC(hipMemcpyAsync(out_xyz1, h->clouds[slot].p, (size_t)m * 16, hipMemcpyDefault, h->stream));
  if (m && out_normals) HIPC(hipMemcpyAsync(out_normals, h->cloud_nrm[slot].p, (size_t)m * 12, hipMemcpyDefault, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  h->cloud_n[slot] = m;
  h->cloud_has_nrm[slot] = normals_knn ? 1 : 0;
  if (n_out) *n_out = m;
  return LSGPU_OK;
}

int lsgpu_cloud_download(lsgpu_icp* h, int slot, float* out_xyz1, float* out_normals, int64_t cap_points) {
  if (!h || slot < 0 || !out_xyz1) return LSGPU_BAD_ARG;
  h->err.clear();
  if ((size_t)slot >= h->clouds.size() || h->cloud_n[slot] < 0) { h->err = "cloud_download: empty slot"; return LSGPU_BAD_ARG; }
  const int64_t n = h->cloud_n[slot];
  if (cap_points < n) { h->err = "cloud_download: the buffer is smaller than the cloud"; return LSGPU_BAD_ARG; }
  if (out_normals && !cloud_has_normals(h, slot)) { h->err = "cloud_download: the slot carries no normals"; return LSGPU_BAD_ARG; }
  HIPC(hipSetDevice(h->device));
  if (n) HIPC(hipMemcpyAsync(out_xyz1, h->clouds[slot].p, (size_t)n * 16, hipMemcpyDefault, h->stream));
  if (n && out_normals) HIPC(hipMemcpyAsync(out_normals, h->cloud_nrm[slot].p, (size_t)n * 12, hipMemcpyDefault, h->stream));
  HIPC(hipStreamSynchronize(h->stream));
  return LSGPU_OK;
}

// sub-map assembly (laser_track.cpp:474-486) on the device: submap = concat_i ( T_i * cloud ref_slots[i] ), `total` points
static int assemble_submap(lsgpu_icp* h, const int* ref_slots, const float* ref_T, int n_ref, int64_t total) {
  HIPC(h->submap.reserve(total));
  int64_t off = 0;
  for (int i = 0; i < n_ref; ++i) {
    const int64_t n = h->cloud_n[ref_slots[i]];
    if (!n) continue;
    const float* T = ref_T ? ref_T + 16 * i : nullptr;
    bool identity = !T;
    if (T) {
      identity = true;
      for (int k = 0; k < 16; ++k) identity = identity && T[k] == ((k % 5 == 0) ? 1.f : 0.f);
    }
    if (identity) {
      HIPC(hipMemcpyAsync(h->submap.p + off, h->clouds[ref_slots[i]].p, (size_t)n * 16, hipMemcpyDeviceToDevice, h->stream));
    } else {
      if (!lsgpu_check_rigid(T)) { h->err = "compute_clouds: a sub-map transform is not rigid"; return LSGPU_BAD_ARG; }
      hipLaunchKernelGGL(k_transform, dim3(nblk(n)), dim3(256), 0, h->stream, h->clouds[ref_slots[i]].p, n,
                         to_mat34(T), h->submap.p + off);
    }
    off += n;
  }
  HIPC(hipGetLastError());
  return LSGPU_OK;
}

static bool is_identity16(const float* T) {
  if (!T) return true;
  bool identity = true;
  for (int k = 0; k < 16; ++k) identity = identity && T[k] == ((k % 5 == 0) ? 1.f : 0.f);
  return identity;
}
// ... of members that all carry normals somebody reads: points and normals in one launch (lsgpu_submap.hip.h); more members
// than its table holds: one launch per member
static int assemble_submap_normals(lsgpu_icp* h, const int* ref_slots, const float* ref_T, int n_ref, int64_t total) {
  HIPC(h->submap.reserve(total)); HIPC(h->submap_nrm.reserve((size_t)3 * total));
  SubmapTable tab;
  std::memset(&tab, 0, sizeof(tab));
  const bool one_launch = n_ref <= kSubmapMembers;
  auto launch = [&]() {
    const int64_t count = (int64_t)tab.first[tab.n] - (int64_t)tab.first[0];
    if (count > 0) hipLaunchKernelGGL(k_assemble_submap, dim3(nblk(count)), dim3(256), 0, h->stream, tab, h->submap.p, h->submap_nrm.p);
  };
  int64_t off = 0;
  for (int i = 0; i < n_ref; ++i) {
    const int slot = ref_slots[i];
    const int64_t n = h->cloud_n[slot];
    if (!n && !one_launch) continue;
    const float* T = ref_T ? ref_T + 16 * i : nullptr;
    const bool identity = is_identity16(T);
    if (n && !identity && !lsgpu_check_rigid(T)) { h->err = "compute_clouds: a sub-map transform is not rigid"; return LSGPU_BAD_ARG; }
    if (!one_launch) { std::memset(&tab, 0, sizeof(tab)); }
    const int m = tab.n++;
    tab.first[m] = (uint32_t)off; tab.first[m + 1] = (uint32_t)(off + n);
    tab.pts[m] = h->clouds[slot].p; tab.nrm[m] = h->cloud_nrm[slot].p;
    tab.identity[m] = identity ? 1 : 0;
    if (!identity) tab.T[m] = to_mat34(T);
    off += n;
    if (!one_launch) launch();
  }
  if (one_launch && tab.n > 0) launch();
  HIPC(hipGetLastError());
  return LSGPU_OK;
}
// Which of the two: the sub-map has normals iff every member carries some, and they are assembled iff the chain has no
// reference module (a module overwrites them) and somebody reads the reference's normals.  *with_normals tells; a member
// without normals among members with them, where they would be read, is refused by its slot
static int assemble_reference(lsgpu_icp* h, const int* ref_slots, const float* ref_T, int n_ref, int64_t total,
                              const lsgpu_chain_config* chain, bool* with_normals) {
  *with_normals = false;
  bool all = n_ref > 0, any = false;
  int without = -1;
  for (int i = 0; i < n_ref; ++i) {
    const bool has = cloud_has_normals(h, ref_slots[i]);
    all = all && has; any = any || has;
    if (!has && without < 0) without = ref_slots[i];
  }
  const bool wanted = chain->ssn_knn == 0 && chain->sn_knn == 0 && reference_normals_read(h);
  if (wanted && any && !all) {
    h->err = "compute_clouds: reference slot " + std::to_string(without) + " carries no normals: the sub-map has none (every member must "
             "carry some), and the chain reads the reference's normals without a reference filter (ssn_knn or sn_knn)";
    return LSGPU_BAD_CONFIG;
  }
  if (!(wanted && all)) return assemble_submap(h, ref_slots, ref_T, n_ref, total);
  *with_normals = true;
  return assemble_submap_normals(h, ref_slots, ref_T, n_ref, total);
}

int lsgpu_icp_compute_clouds(lsgpu_icp* h, int reading_slot, const int* ref_slots, const float* ref_T,
                             int n_ref, const float T_init[16], const lsgpu_chain_config* chain,
                             float T_out[16], lsgpu_icp_stats* stats) {
  if (!h || !T_init || !T_out || !chain || n_ref < 0 || (n_ref > 0 && !ref_slots)) return LSGPU_BAD_ARG;
  h->err.clear();
  std::memcpy(T_out, T_init, 16 * sizeof(float));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  auto have = [&](int s) { return s >= 0 && (size_t)s < h->clouds.size() && h->cloud_n[s] >= 0; };
  if (!have(reading_slot)) { h->err = "compute_clouds: empty reading slot"; return LSGPU_BAD_ARG; }
  int64_t total = 0;
  for (int i = 0; i < n_ref; ++i) {
    if (!have(ref_slots[i])) { h->err = "compute_clouds: empty reference slot"; return LSGPU_BAD_ARG; }
    total += h->cloud_n[ref_slots[i]];
  }
  if (total > 0x7FFFFFF0ll) return LSGPU_BAD_ARG;
  if (total <= 0 || h->cloud_n[reading_slot] <= 0) {
    if (chain->seed >= 0) DrawStream::global().take(chain->seed, 0, nullptr);
    h->err = "compute: empty cloud";
    return LSGPU_NO_CONVERGENCE;
  }
  HIPC(hipSetDevice(h->device));
  bool with_normals = false;
  {
    const int rca = assemble_reference(h, ref_slots, ref_T, n_ref, total, chain, &with_normals);
    if (rca) return rca;
  }
  // (the assembly is stream-ordered: its time is part of compute's filter time, stats->t_reserved[0])
  return compute_run(h, reinterpret_cast<const float*>(h->clouds[reading_slot].p), h->cloud_n[reading_slot],
                     reinterpret_cast<const float*>(h->submap.p), total, T_init, chain, T_out, stats, nullptr, nullptr,
                     cloud_has_normals(h, reading_slot) ? h->cloud_nrm[reading_slot].p : nullptr,
                     with_normals ? h->submap_nrm.p : nullptr, /*ref_nrm_owned*/ true);
}

int lsgpu_icp_compute_clouds_upload_normals(lsgpu_icp* h, int reading_slot, const float* reading_xyz1, const float* reading_normals,
                                            int64_t nq, const int* ref_slots, const float* ref_T, int n_ref, const float T_init[16],
                                            const lsgpu_chain_config* chain, float T_out[16], lsgpu_icp_stats* stats) {
  if (!h || !T_init || !T_out || !chain || n_ref < 0 || (n_ref > 0 && !ref_slots)) return LSGPU_BAD_ARG;
  const int rcu = lsgpu_cloud_upload_normals(h, reading_slot, reading_xyz1, reading_normals, nq);
  if (rcu) return rcu;
  return lsgpu_icp_compute_clouds(h, reading_slot, ref_slots, ref_T, n_ref, T_init, chain, T_out, stats);
}

// lsgpu_cloud_upload(reading_slot) + lsgpu_icp_compute_clouds in one call: the new scan crosses PCIe WHILE the sub-map --
// the scans already in HBM -- is assembled and filtered (its own stream and host thread, as the host reading of
// lsgpu_icp_compute).  LaserTrack::localScanToSubMap matches every new scan exactly once, right after it arrived
// (laser_track.cpp:112-119, 466-519): uploaded first and matched afterwards, the 0.3 ms of a 1 M-point scan's copy were
// spent with the device idle, inside the reference's own timed region (scan_matching_times_).  The slot holds the scan on
// return whatever the registration's outcome, like the two calls one after the other.
int lsgpu_icp_compute_clouds_upload(lsgpu_icp* h, int reading_slot, const float* reading_xyz1, int64_t nq,
                                    const int* ref_slots, const float* ref_T, int n_ref, const float T_init[16],
                                    const lsgpu_chain_config* chain, float T_out[16], lsgpu_icp_stats* stats) {
  if (!h || !T_init || !T_out || !chain || n_ref < 0 || (n_ref > 0 && !ref_slots)) return LSGPU_BAD_ARG;
  if (reading_slot < 0 || reading_slot >= (1 << 20) || nq < 0 || nq > 0x7FFFFFF0ll || (nq > 0 && !reading_xyz1)) return LSGPU_BAD_ARG;
  auto have = [&](int s) { return s >= 0 && (size_t)s < h->clouds.size() && h->cloud_n[s] >= 0; };
  bool fused = nq > 0 && !is_device_ptr(reading_xyz1);
  int64_t total = 0;
  for (int i = 0; i < n_ref && fused; ++i) {
    fused = have(ref_slots[i]) && ref_slots[i] != reading_slot;
    if (fused) total += h->cloud_n[ref_slots[i]];
  }
  bool ref_all_nrm = n_ref > 0;
  for (int i = 0; i < n_ref && fused; ++i) ref_all_nrm = ref_all_nrm && cloud_has_normals(h, ref_slots[i]);
  fused = fused && total > 0 && total <= 0x7FFFFFF0ll && chain_ok(h, chain, ref_all_nrm);   // (ssn_knn 0: point-to-point without a reference filter)
  if (!fused) {   // nothing to overlap (or nothing to match against): the two calls, one after the other
    const int rcu = lsgpu_cloud_upload(h, reading_slot, reading_xyz1, nq);
    if (rcu) return rcu;
    return lsgpu_icp_compute_clouds(h, reading_slot, ref_slots, ref_T, n_ref, T_init, chain, T_out, stats);
  }
  h->err.clear();
  std::memcpy(T_out, T_init, 16 * sizeof(float));
  if (stats) std::memset(stats, 0, sizeof(*stats));
  HIPC(hipSetDevice(h->device));
  cloud_slot_clear(h, reading_slot);   // (this entry stores points only: the slot's normals are dropped, as by lsgpu_cloud_upload)
  HIPC(h->clouds[reading_slot].reserve(nq));
  bool with_normals = false;
  {
    const int rca = assemble_reference(h, ref_slots, ref_T, n_ref, total, chain, &with_normals);
    if (rca) {   // (a sub-map transform that is not rigid: the scan is stored all the same)
      const std::string why = h->err;
      const int rcu = lsgpu_cloud_upload(h, reading_slot, reading_xyz1, nq);
      h->err = why;
      return rcu ? rcu : rca;
    }
  }
  bool upload_enqueued = false;
  const int rc = compute_run(h, reading_xyz1, nq, reinterpret_cast<const float*>(h->submap.p), total, T_init, chain, T_out, stats,
                             h->clouds[reading_slot].p, &upload_enqueued, nullptr, with_normals ? h->submap_nrm.p : nullptr, /*ref_nrm_owned*/ true);
  if (!upload_enqueued) {   // the call returned before its upload went out: the plain copy, so that the slot holds the scan
    const std::string why = h->err;
    HIPC(hipMemcpyAsync(h->clouds[reading_slot].p, reading_xyz1, (size_t)nq * 16, hipMemcpyDefault, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    h->err = why;
  }
  h->cloud_n[reading_slot] = nq;
  return rc;
}

}  // extern "C"

// The loop's normal-equation kernel for k matches per reading point (k-match loop, k >= 2), for the chain plan (KDTreeMatcher
// maxDist / outlier-filter chains, any k) and for RobustOutlierFilter's weighted pairs (always the chain plan).
// nullptr: k = 1 without a chain -- the plain k_normal_eq_loop<minimizer> serves that case.
using NeLoopFn = decltype(&k_normal_eq_loop<kPointToPlane>);
using UpdateFn = decltype(&k_icp_update<kPointToPlane>);
template <int MIN, bool CHAIN, bool RB, size_t... I>
static NeLoopFn ne_loop_of_k(int k, std::index_sequence<I...>) {
  static const NeLoopFn tab[] = {k_normal_eq_loop<MIN, (int)I + 1, CHAIN, RB>...};   // k = 1 .. kKnnKMax
  return tab[k - 1];
}
template <bool CHAIN, bool RB>
static NeLoopFn ne_loop_of(bool p2p, int k) {
  using Ks = std::make_index_sequence<kKnnKMax>;
  return p2p ? ne_loop_of_k<kPointToPoint, CHAIN, RB>(k, Ks{}) : ne_loop_of_k<kPointToPlane, CHAIN, RB>(k, Ks{});
}
// force4DOF / force2D (lsgpu_icp_set_motion: knn 1, binary filters): the plain loop and the chain plan's k = 1 instantiation
template <int MIN>
static void constrained_kernels(bool chain, NeLoopFn* ne_loop, NeLoopFn* ne_loop_k, UpdateFn* update) {
  *ne_loop = k_normal_eq_loop<MIN>;
  *ne_loop_k = chain ? k_normal_eq_loop<MIN, 1, true, false> : nullptr;
  *update = k_icp_update<MIN>;
}
static NeLoopFn ne_loop_fn(bool p2p, int k, bool chain, bool robust) {
  if (robust) return ne_loop_of<true, true>(p2p, k);
  if (chain) return ne_loop_of<true, false>(p2p, k);
  return k >= 2 ? ne_loop_of<false, false>(p2p, k) : nullptr;
}

// One call of lsgpu_icp_align: the state its phases share, and the phases in the order they run -- start, init_loop_state,
// configure_policy, feed (which enqueues iterations and fetches the loop state), harvest.  Each returns an LSGPU code.
struct AlignRun {
  lsgpu_icp* const h;
  const float* const reading_xyz1; const int64_t nq; const float* const T_init;   // the call's arguments
  AlignExtras x;   // ... and what a caller inside this file adds to them (build_index_on_side: unless configure_policy calls it off)
  int kk = 1;   // KDTreeMatcher knn: 1, or k >= 2 nearest matches per reading point (k N pairs; the split-scan mode refuses such handles)
  bool kmatch = false, chain = false, robust = false, angle = false;
  ChainArgs ca{};
  double t0 = 0.0;
  float T_rm_in[16];
  int64_t nq_total = 0;
  int max_it = 0, nb = 0;
  IcpState* hst = nullptr;   // the staging block's copy of the loop state
  uint32_t k = 0;            // TrimmedDist rank
  bool p2p = false, timed = false, split_update = false;
  Mat34 Tdummy;
  NeLoopFn ne_loop = nullptr, ne_loop_k = nullptr; UpdateFn update = nullptr;   // this handle's instantiations
  std::vector<size_t> ev_of_launch;  // event index of every enqueued iteration

  // Start checks, the reading's order (step 5) and, in the split-scan mode, the entry handshake.
  int start() {
    h->trace.clear(); h->trace_on_device = 0; h->rb_trace_n = 0; h->na_trace_n = 0;
    // Local reasons not to start.  In the split-scan mode they are NOT returned yet: a rank that left here would
    // leave its peers blocked in the first collective, so every rank first takes part in the entry handshake below.
    int local_rc = LSGPU_OK;
    kk = h->cfg.matcher_knn >= 2 ? h->cfg.matcher_knn : 1;
    kmatch = kk > 1;
    // KDTreeMatcher maxDist / Max-, Min-, MedianDistOutlierFilter: the chain plan (lsgpu_policy.h), whatever k
    chain = chain_on(h);
    ca.lo2 = h->cfg.outlier_min_dist * h->cfg.outlier_min_dist;
    ca.max2 = (h->cfg.outlier_max_dist > 0.f && !std::isinf(h->cfg.outlier_max_dist)) ? h->cfg.outlier_max_dist * h->cfg.outlier_max_dist : INFINITY;
    ca.med_factor = h->cfg.outlier_median_factor; ca.has_median = h->cfg.outlier_median_factor > 0.f ? 1 : 0;
    robust = h->mods.robust_on;
    if (robust) { ca.rb = robust::params(h->mods.robust); ca.has_trim = h->cfg.trim_ratio < 1.f ? 1 : 0; }
    // SurfaceNormalOutlierFilter: inert without reading normals or without reference normals (as upstream)
    angle = chain && h->mods.normals_on && h->mods.normals.max_angle >= 0.f && h->have_normals && reading_xyz1 && x.reading_normals;
    if (robust && ca.rb.plane && !h->have_normals) {
      h->err = "align: RobustOutlierFilter distanceType point2plane needs reference normals";
      return LSGPU_BAD_CONFIG;
    }
    if (h->nr <= 0 || nq <= 0 || !reading_xyz1) {  // empty cloud: ConvergenceError upstream
      h->err = "align: empty reading or no reference";
      local_rc = LSGPU_NO_CONVERGENCE;
    } else if (nq > 0x7FFFFFF0ll) {
      local_rc = LSGPU_BAD_ARG;
    } else if (kmatch && h->nr < kk) {
      h->err = "align: the reference has fewer points than the matcher's knn";
      local_rc = LSGPU_BAD_ARG;
    } else if (kmatch && nq > 0x7FFFFFF0ll / kk) {
      h->err = "align: knn x reading points exceeds the 32-bit pair count";
      local_rc = LSGPU_BAD_ARG;
    } else if (!lsgpu_check_rigid(T_init)) {
      // step 5 moves the reading with RigidTransformation::compute, which throws TransformationError for such a matrix
      // (after both filters have run, as here when the call came through lsgpu_icp_compute)
      h->err = "align: the initial guess is not a rigid transformation (|1 - det R| > 1e-3)";
      local_rc = LSGPU_BAD_ARG;
    }
    if (local_rc && !h->comm) return local_rc;
    HIPC(hipSetDevice(h->device));
    t0 = wall_ms();
    h->knn_events_used = 0;
    h->comm_events_used = 0;
    h->time_comm = h->comm != nullptr && h->cfg.profile_kernels != 0;
    h->tail_pending = false;   // (from here on everything is behind it on h->stream itself)

    // step 5: T_refMean_dataIn = T_refIn_refMean^-1 * T_init (pure translation inverse)
    std::memcpy(T_rm_in, T_init, sizeof(T_rm_in));
    for (int d = 0; d < 3; ++d) T_rm_in[12 + d] = T_init[12 + d] - h->mean[d];
    int rc = local_rc;
    if (!rc && x.queries_prepared && !h->comm) HIPC(hipStreamWaitEvent(h->stream, h->side_done, 0));   // (ordered and moved on the side lane already)
    else if (!rc) rc = prepare_queries(h, reading_xyz1, nq, to_mat34(T_rm_in));
    if (rc && !h->comm) return rc;
    nq_total = nq;
    if (h->comm) {
      // entry handshake: {shard size, cannot-start flag} summed over the ranks.  TrimmedDist ranks over ALL matches, so
      // the rank uses the global count; and either every rank enters the loop or none does.
      long long* hn = h->pin->handshake;
      hn[0] = rc ? 0 : (long long)nq;
      hn[1] = rc ? 1 : 0;
      HIPC(hipMemcpyAsync(h->comm_tmp.p, hn, 2 * sizeof(long long), hipMemcpyHostToDevice, h->stream));
      RCCLC(rccl_api()->AllReduce(h->comm_tmp.p, h->comm_tmp.p + 2, 2, ncclInt64, ncclSum, h->comm, h->stream));
      HIPC(hipMemcpyAsync(hn, h->comm_tmp.p + 2, 2 * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
      const int w = wait_stream(h);
      if (w) return w;
      nq_total = (int64_t)hn[0];
      if (rc) return rc;
      if (hn[1] != 0) {
        h->err = "align (split-scan): another rank could not start; all ranks give up together";
        return LSGPU_NO_CONVERGENCE;
      }
    }
    return LSGPU_OK;
  }

  // step 6: the loop runs on the device.  Every iteration is {kNN, select x3, normal equations,
  // update}; k_icp_update solves, moves T_iter, runs the checkers and raises `done`, after which the
  // remaining enqueued launches exit immediately.  The host only looks at the state every few iterations.
  // Here: the loop's buffers, its initial state (one launch, k_align_init) and the kernels this handle's loop is made of.
  int init_loop_state() {
    max_it = h->cfg.max_iterations;
    HIPC(h->state.reserve(1));
    HIPC(h->chk_hist.reserve((size_t)8 * (max_it + 2)));
    HIPC(h->trace_dev.reserve((size_t)max_it));
    if (robust) {
      HIPC(h->rb_hist.reserve(3 * kHistBins)); HIPC(h->rb_sel.reserve(4)); HIPC(h->rb_state.reserve(1));
      HIPC(h->rb_trace_dev.reserve((size_t)max_it));
      HIPC(hipMemsetAsync(h->rb_state.p, 0, sizeof(RobustState), h->stream));
      ca.rb_hist = h->rb_hist.p; ca.rb_sel = h->rb_sel.p; ca.rb_state = h->rb_state.p; ca.rb_trace = h->rb_trace_dev.p;
    }
    if (angle) {
      // step 5 moves the reading's descriptors with the reading: n0 = R_init n, once per alignment (lsgpu_rotate_descriptors' chain)
      HIPC(h->rd_nrm0.reserve((size_t)3 * nq)); HIPC(h->na_trace_dev.reserve((size_t)max_it));
      hipLaunchKernelGGL(k_rotate3, dim3(nblk(nq)), dim3(256), 0, h->stream, h->rd_nrm.p, nq, to_mat34(T_rm_in), h->rd_nrm0.p);
      HIPC(hipGetLastError());
      ca.na_rn = h->rd_nrm0.p; ca.na_eps = normal_angle::eps_of(h->mods.normals.max_angle); ca.na_trace = h->na_trace_dev.p;
    }
    hst = &h->pin->state;
    std::memset(hst, 0, sizeof(IcpState));
    hostmath::identity4(hst->T_iter);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) hst->T_rows[r * 4 + c] = hst->T_iter[c * 4 + r];
    hst->prev_limit = INFINITY; hst->cap2 = INFINITY;
    hst->cap_enabled = (h->cfg.reserved[0] == 0 && !kmatch && !chain) ? 1 : 0;   // (no radius cap in the k-match loop / the chain plan)
    hst->minimizer = h->cfg.error_minimizer;
    hst->max_iter = max_it; hst->smooth = h->cfg.smooth_length;
    hst->lim_rot = h->cfg.min_diff_rot; hst->lim_trans = h->cfg.min_diff_trans;
    AlignInitArgs ia{};
    {  // checkers.init(T_iter): history starts with the identity
      hostmath::CheckerState cs{0, 0};
      hostmath::checker_push(&cs, ia.chk0, hst->T_iter);
      hst->counter = cs.counter; hst->n_hist = cs.n_hist;
    }
    k = trim_rank((int64_t)kk * nq_total, h->cfg.trim_ratio);   // (TrimmedDist ranks all k N distances)
    HIPC(h->sel_aux.reserve(kSelFailFlag + 4));
    HIPC(h->spread_flag.reserve((size_t)((nq + 63) / 64))); HIPC(h->spread_list.reserve(kFrontMax)); HIPC(h->spread_cnt.reserve(2));
    HIPC(h->sel_win.reserve((size_t)kSelWinRows * 512));
    HIPC(h->amb_key.reserve((size_t)kSelAmbCap)); HIPC(h->amb_val.reserve((size_t)kSelAmbCap * 32));
    hst->sel_wide = (!h->comm && tuning().fused_select && !kmatch && !chain) ? 1 : 0;
    h->n_spread_host = 0; h->n_spread_known = false;
    ia.state = *hst;
    ia.sel0 = SelState{0u, k};   // sel[0] = {0, rank}: constant during an align
    ia.state_dev = h->state.p; ia.chk_hist = h->chk_hist.p; ia.sel = h->sel.p;
    ia.counters3 = h->counters.p + 32;   // stragglers, (unused), heavy-tile ticket
    ia.ne_ticket = h->ne_tickets.p; ia.sel_aux = h->sel_aux.p; ia.spread_flag = h->spread_flag.p;
    ia.spread_cnt = h->spread_cnt.p; ia.sel_win = h->sel_win.p; ia.hist = h->hist.p;
    ia.n_sel_aux = kSelFailFlag + 4; ia.n_spread_flag = (int)((nq + 63) / 64); ia.n_sel_win = kSelWinRows * 512;
    hipLaunchKernelGGL(k_align_init, dim3(64), dim3(256), 0, h->stream, ia);
    HIPC(hipGetLastError());

    nb = std::min(kNeBlocks, nblk((int64_t)kk * nq));
    timed = h->cfg.profile_kernels != 0;
    Tdummy = to_mat34(hst->T_iter);
    split_update = tuning().split_update;  // (profiling: the update as its own launch)
    // the minimizer's instantiations of the accumulation and of the update (point-to-point reads no normals)
    p2p = h->cfg.error_minimizer == LSGPU_MINIMIZER_POINT_TO_POINT;
    ne_loop = p2p ? k_normal_eq_loop<kPointToPoint> : k_normal_eq_loop<kPointToPlane>;
    update = p2p ? k_icp_update<kPointToPoint> : k_icp_update<kPointToPlane>;
    ne_loop_k = ne_loop_fn(p2p, kk, chain, robust);
    if (h->mods.dof() == LSGPU_MOTION_DOF_4) constrained_kernels<kPointToPlane4Dof>(chain, &ne_loop, &ne_loop_k, &update);
    if (h->mods.dof() == LSGPU_MOTION_DOF_3) constrained_kernels<kPointToPlane2D>(chain, &ne_loop, &ne_loop_k, &update);
    if (h->mods.bound()) HIPC(h->h_chk.reserve((size_t)8 * (max_it + 2)));   // the bound's host copy of the checker history
    ca.hist_med = h->hist_med.p; ca.sel_med = h->sel_med.p;
    return LSGPU_OK;
  }

  // The launch policy (lsgpu_policy.h) decides what every iteration is made of and when the host looks at the loop
  // state; feed() executes its decisions.  (tests/cpp/policy_check.cpp drives the same state machine on the CPU.)
  int configure_policy() {
    policy::Config& pc = h->pol_cfg;
    pc = policy::Config();
    pc.cone_from = tuning().cone_from; pc.wide_iters = tuning().wide_iters; pc.group = 6;
    pc.enq_limit = 8 * max_it + 64;   // (only guards against a device that never finishes, see below)
    pc.predict_select = tuning().predict_select; pc.commit_select = tuning().commit_select; pc.comm_commit = tuning().comm_commit;
    pc.lookahead = tuning().lookahead; pc.comm = h->comm != nullptr;
    pc.seed_cap = tuning().seed_cap; pc.cap_enabled = h->cfg.reserved[0] == 0;
    pc.two_pass_select = !h->comm && tuning().fused_select && tuning().two_pass_select;
    pc.cone_probe = tuning().cone_probe; pc.cone_heavy_share = tuning().cone_heavy_share; pc.cone_max_occupancy = tuning().cone_max_occupancy;
    pc.kmatch = kmatch; pc.chain = chain;
    pc.robust_mad = robust && ca.rb.mad; pc.robust_scale_iters = robust ? h->mods.robust.nb_iteration_for_scale : 0;
    const bool index = x.build_index_on_side ? cone_wanted(h) : h->cone_ok;   // (built behind the first iteration, feed(): h->cone_ok is false until then)
    if (x.build_index_on_side) h->cone_decided = false;
    // a handle whose last alignments found the index slower than the voxel grid leaves it alone for a while (and spares
    // itself the build when that is still to come)
    // (a reference of a markedly different size is another scene or another sub-map depth: the judgement starts over)
    if (h->index_rest > 0 && (h->nr > 2 * h->index_rest_nr || 2 * h->nr < h->index_rest_nr)) h->index_rest = 0;
    const bool index_rests = h->index_rest > 0 && index;
    if (index_rests) { --h->index_rest; x.build_index_on_side = false; }
    h->pol.begin_align(index && !index_rests, h->cone_decided, h->cone_dense, h->cone_occupancy);
    h->pay_voxel_timed = h->pay_index_timed = false;
    for (Event& e : h->ev_pay) HIPC(e.ensure(hipEventDefault));
    if (pc.lookahead && !pc.comm) HIPC(h->ev_state.ensure(hipEventDisableTiming));   // (fetch_state's look-ahead)
    return LSGPU_OK;
  }

  // One iteration on the stream.
  // itn.knn == false: only select + normal equations + update on the distances already there (after a missed
  // prediction).  RCCL mode: the per-shard tables of a *committed* iteration are summed over the ranks in ONE grouped
  // all-reduce (the host knows beforehand that no select kernel will run: sel_streak comes from the global limit,
  // so every rank takes the same decision); un-committed iterations there run the plain three-pass select.
  int enqueue_iteration(const policy::Iteration& itn) {
    int r = LSGPU_OK;
    if (kmatch || chain) {   // the k-match / chain plan (lsgpu_policy.h): k-best search, three-pass select on the k N distances, pair-indexed sums
      const int np = (int)(kk * nq);
      r = run_knn_k(h, kk, Tdummy, h->state.p, itn.seed, timed);                                     // 6a+6b
      if (r) return r;
      ev_of_launch.push_back(h->knn_events_used ? h->knn_events_used - 1 : 0);
      // (chain: the rank from the device's count of valid matches, the median beside it if the chain holds that filter)
      // (RobustOutlierFilter's MAD needs the median too; the MAD's own select runs only where the scale is recomputed)
      r = run_select(h, h->kd2.p, np, k, false /* armed by k_align_init / the previous k_normal_eq_loop */, h->state.p, true, false, 3,
                     chain ? h->cfg.trim_ratio : 0.f, chain && (ca.has_median || itn.mad));  // 6c
      if (r) return r;
      if (itn.mad) { r = run_mad(h, h->kd2.p, np, h->state.p); if (r) return r; }
      ChainArgs ca_it = ca;
      ca_it.rb_recompute = itn.mad ? 1 : 0;
      lsgpu_icp::KnnEv* evk = (timed && h->knn_events_used) ? &h->knn_events[h->knn_events_used - 1] : nullptr;
      if (evk) HIPC(hipEventRecord(evk->d, h->stream));
      hipLaunchKernelGGL(ne_loop_k, dim3(nb), dim3(256), 0, h->stream, h->rdq.p, np,
                         h->state.p, h->kmatch.p, h->kd2.p, (p2p && !(robust && ca.rb.plane) && !angle) ? (const float4*)nullptr : h->nrm.p, h->hist.p, h->sel.p + 2,
                         h->counters.p + 32, h->ne_tickets.p, h->ne_partials.p, h->ne_gpartials.p, h->ne_out.p,
                         h->chk_hist.p, h->trace_dev.p, max_it, 0, !split_update ? 1 : (robust || angle) ? 2 /* the serial update, in this launch */ : 0,
                         h->sel_aux.p, (uint32_t*)nullptr, 0, (uint32_t*)nullptr,
                         0, (uint32_t*)nullptr, (uint2*)nullptr, (double*)nullptr, 0, 0, ca_it);   // 6d (+6e)
      if (split_update && !robust && !angle)
        hipLaunchKernelGGL(update, dim3(1), dim3(64), 0, h->stream, h->state.p, h->ne_out.p,
                           h->chk_hist.p, h->trace_dev.p, max_it, 0, h->sel_aux.p);                       // 6d+6e
      if (evk) HIPC(hipEventRecord(evk->e, h->stream));
      return hipGetLastError() == hipSuccess ? LSGPU_OK : LSGPU_HIP_ERROR;
    }
    if (itn.knn) {
      r = run_knn(h, Tdummy, h->state.p, itn, timed, itn.seed && itn.capped ? k : 0xFFFFFFFFu);  // 6a+6b
      if (r) return r;
      ev_of_launch.push_back(h->knn_events_used ? h->knn_events_used - 1 : 0);
    }
    if (itn.committed && h->comm) {  // one exchange for the whole select: {counts below, 11-bit histogram, window table}
      RcclApi* api = rccl_api();
      comm_mark(h, true);
      if (api->GroupStart) RCCLC(api->GroupStart());
      RCCLC(api->AllReduce(h->sel_aux.p, h->sel_aux.p, kSelFailFlag, ncclUint32, ncclSum, h->comm, h->stream));
      RCCLC(api->AllReduce(h->hist.p + kHistBins, h->hist.p + kHistBins, kHistBins, ncclUint32, ncclSum, h->comm, h->stream));
      RCCLC(api->AllReduce(h->sel_win.p, h->sel_win.p, (size_t)kSelWinRows * 512, ncclUint32, ncclSum, h->comm, h->stream));
      if (api->GroupEnd) RCCLC(api->GroupEnd());
      comm_mark(h, false);
    }
    if (!itn.committed) {
      r = run_select(h, h->d2.p, (int)nq, k, false /* armed by k_align_init / k_seed_cap / the previous k_normal_eq_loop */,
                     h->state.p, true, itn.predicted, itn.full_select ? 3 : 2);       // 6c
      if (r) return r;
    }
    lsgpu_icp::KnnEv* ev = (timed && itn.knn && h->knn_events_used) ? &h->knn_events[h->knn_events_used - 1] : nullptr;
    if (ev) HIPC(hipEventRecord(ev->d, h->stream));
    hipLaunchKernelGGL(ne_loop, dim3(nb), dim3(256), 0, h->stream, h->rdq.p, (int)nq,
                       h->state.p, h->prev.p, h->d2.p, p2p ? (const float4*)nullptr : h->nrm.p, h->hist.p, h->sel.p + 2,
                       h->counters.p + 32, h->ne_tickets.p, h->ne_partials.p, h->ne_gpartials.p, h->ne_out.p,
                       h->chk_hist.p, h->trace_dev.p, max_it, itn.capped ? 1 : 0, (h->comm || split_update) ? 0 : 1,
                       h->sel_aux.p, (h->comm || !tuning().fused_select) ? h->sel_win.p : nullptr, itn.committed ? 1 : 0, h->spread_cnt.p,
                       (itn.predicted && itn.knn) ? 1 : 0, h->sel_aux.p + kSelFailFlag + 2, h->amb_key.p, h->amb_val.p, tuning().sel_amb_cap,
                       (!itn.full_select && !itn.committed) ? 1 : 0, ChainArgs{});   // 6d (+6e)
    if (h->comm || split_update) {   // split scan: every rank gets the sums over all shards (the limit, slot 29, is already global)
      if (h->comm) comm_mark(h, true);
      if (h->comm && rccl_api()->AllReduce(h->ne_out.p, h->ne_out.p, kNe, ncclDouble, ncclSum, h->comm, h->stream) != ncclSuccess) {
        h->err = "RCCL all-reduce of the normal equations failed";
        return LSGPU_HIP_ERROR;
      }
      if (h->comm) comm_mark(h, false);
      hipLaunchKernelGGL(update, dim3(1), dim3(64), 0, h->stream, h->state.p, h->ne_out.p,
                         h->chk_hist.p, h->trace_dev.p, max_it, itn.capped ? 1 : 0, h->sel_aux.p);           // 6d+6e
    }
    if (ev) HIPC(hipEventRecord(ev->e, h->stream));
    return hipGetLastError() == hipSuccess ? LSGPU_OK : LSGPU_HIP_ERROR;
  }

  // A look at the loop state.  Look-ahead (not in the split-scan mode): ONE more iteration is enqueued behind the copy
  // before the host waits for it, so the device works through the round trip instead of idling (~25 us + a cold first
  // launch per look); that iteration carries the decisions of the previous look, like the later iterations of any group,
  // and exits at once if the state it finds says `done`.
  int fetch_state(int* enqueued_ahead) {
    *enqueued_ahead = 0;
    if (h->mods.bound())   // BoundTransformationChecker: the history travels with the state (evaluated after the loop, check_bound)
      HIPC(hipMemcpyAsync(h->h_chk.p, h->chk_hist.p, (size_t)8 * (max_it + 2) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPC(hipMemcpyAsync(hst, h->state.p, sizeof(IcpState), hipMemcpyDeviceToHost, h->stream));
    policy::Iteration ahead_it;
    if (h->pol.lookahead_iteration(h->pol_cfg, &ahead_it)) {
      HIPC(hipEventRecord(h->ev_state, h->stream));
      const int r = enqueue_iteration(ahead_it);
      if (r) return r;
      *enqueued_ahead = 1;
      HIPC(hipEventSynchronize(h->ev_state));
      return LSGPU_OK;
    }
    return wait_stream(h);  // (bounded in the split-scan mode: a dead peer must not hang this rank)
  }

  // The feed loop: iteration 0, the deferred build of the direction index, then groups of iterations and looks until `done`.
  int feed() {
    policy::Config& pc = h->pol_cfg;
    policy::State& pol = h->pol;
    // iteration 0: seeded; capped by the trim quantile of the seed distances (a guaranteed bound: no retry can follow)
    int rc = enqueue_iteration(pol.plan(pc, true, pc.seed_cap && pc.cap_enabled, true, true, false));
    if (rc) return rc;
    pol.enq = 1; pol.since_check = 1;
    if (x.build_index_on_side) {
      // lsgpu_icp_compute left the direction index's build to this point: the device is busy with the first search, the
      // ~15 launches of the build go to the side stream (its own sort scratch) while it is
      LaneScope on_side(h, h->side_lane());
      int rb = build_cone_index(h);
      if (!rb && h->cone_ok) {
        if (hipEventRecord(h->cone_done, h->side_stream) != hipSuccess) { (void)hipGetLastError(); rb = LSGPU_HIP_ERROR; h->err = "align: event record"; }
        h->cone_pending = true;
      }
      if (rb) return rb;
    }
    // The device decides when the loop ends (CounterTransformationChecker raises `done` after max_iterations at the
    // latest); the host keeps feeding groups of launches until it sees `done`.  Launches enqueued behind an
    // iteration that had to be repeated exit at once, so the number of enqueues is NOT bounded by max_iterations;
    // the policy's enq_limit only guards against a device that never finishes.
    for (;;) {
      policy::Iteration itn;
      if (pol.next_in_group(pc, &itn)) {
        rc = enqueue_iteration(itn);
        if (rc) return rc;
        continue;
      }
      int ahead = 0;
      const bool repriced = pol.wants_reprice();   // (the last launch in front of this look priced the index again: its counters
      rc = fetch_state(&ahead);                    //  were copied in front of the state, they are on the host when the state is)
      if (rc) return rc;
      h->n_spread_host = hst->n_spread; h->n_spread_known = true;
      policy::LookInput li;
      li.done = hst->done; li.status = hst->status; li.iter = hst->iter; li.sel_streak = hst->sel_streak;
      if (hst->sel_fails >= 2) pc.two_pass_select = false;   // (slices fuller than the normal equations can set aside: the select's third pass is back)
      li.stragglers = hst->stragglers; li.nq = nq; li.status_cap_failed = kStatusCapFailed; li.status_sel_failed = kStatusSelFailed;
      if (tuning().short_last_group) { li.chk_rot = hst->chk_rot; li.chk_trans = hst->chk_trans; li.lim_rot = hst->lim_rot; li.lim_trans = hst->lim_trans; li.chk_rot_prev = hst->chk_rot_prev; li.chk_trans_prev = hst->chk_trans_prev; }
      const policy::LookVerdict verdict = pol.on_look(pc, li, ahead, repriced ? price_share(h) : -1.f);
      if (verdict == policy::LookVerdict::RepeatUncapped || verdict == policy::LookVerdict::RepeatSelect) {
        // RepeatUncapped: the cap prediction failed for iteration hst->iter: repeat it uncapped, then carry on.
        // RepeatSelect: the limit left the predicted 12-bit bin in iteration hst->iter: its distances stand, the full
        // select and everything after it run again.
        const bool select_only = verdict == policy::LookVerdict::RepeatSelect;
        if (select_only) hst->sel_streak = 0;
        hst->done = 0; hst->status = 0;
        HIPC(hipMemcpyAsync(h->state.p, hst, sizeof(IcpState), hipMemcpyHostToDevice, h->stream));
        HIPC(hipStreamSynchronize(h->stream));
        rc = enqueue_iteration(select_only ? pol.repeat_select(pc) : pol.repeat_uncapped(pc));
        if (rc) return rc;
        continue;
      }
      if (verdict == policy::LookVerdict::Done) {
        if (ahead) {   // one launch is still queued behind the look that saw `done`
          HIPC(h->ev_tail.ensure(hipEventDisableTiming));
          HIPC(hipEventRecord(h->ev_tail, h->stream));
          h->tail_pending = true;
        }
        return LSGPU_OK;
      }
      if (verdict == policy::LookVerdict::GiveUp) {
        h->err = "align: the device loop did not finish";
        return LSGPU_HIP_ERROR;
      }
    }
  }

  // BoundTransformationChecker, after the loop: the first entry of the checker history (entry 0: the state the checkers were
  // initialised with) out of bounds.  When the counter ended the loop its last T_iter is in no history: a checker listed in
  // front of the counter has seen it.  true: violated, h->err holds the text.  A loop that failed by itself did so behind
  // every entry of its history, so a violation found here came first.
  bool check_bound() {
    const lsgpu_motion_config& mc = h->mods.mo_cfg;
    int n = std::min(hst->n_hist, max_it + 2);
    float* hist = h->h_chk.p;
    if (mc.bound_before_counter && hst->status == LSGPU_OK && hst->done && !hst->converged && hst->iter > 0 && n <= max_it + 1) {
      hostmath::CheckerState cs{0, n};
      hostmath::checker_push(&cs, hist, hst->T_iter);
      n = cs.n_hist;
    }
    float rot = 0.f, tr = 0.f;
    if (hostmath::bound_first_violation(hist, n, mc.max_rotation_norm, mc.max_translation_norm, &rot, &tr) < 0) return false;
    char buf[192];
    std::snprintf(buf, sizeof(buf), "BoundTransformationChecker: limit out of bounds: rot %g/%g tr %g/%g", (double)rot,
                  (double)mc.max_rotation_norm, (double)tr, (double)mc.max_translation_norm);
    h->err = buf;
    return true;
  }

  // The harvest: the index's pay-off judgement, status text, T_out (step 7), statistics and timings.  Returns the loop's status.
  int harvest(float T_out[16], lsgpu_icp_stats& st) {
    const policy::State& pol = h->pol;
    st.cap_retries = pol.cap_retries;
    if (h->pay_voxel_timed && h->pay_index_timed) {   // (both launches are long over: the loop's end was seen behind them)
      float t_voxel = 0.f, t_index = 0.f;
      if (hipEventElapsedTime(&t_voxel, h->ev_pay[0], h->ev_pay[1]) == hipSuccess && hipEventElapsedTime(&t_index, h->ev_pay[2], h->ev_pay[3]) == hipSuccess) {
        h->pay_voxel_us = t_voxel * 1e3f; h->pay_index_us = t_index * 1e3f;
        if (tuning().index_rest && policy::index_not_paying(t_voxel * 1e3f, t_index * 1e3f)) { h->index_rest = policy::kIndexRestAligns; h->index_rest_nr = h->nr; }
      } else {
        (void)hipGetLastError();
      }
    }
    const int it = hst->iter;
    const int rc = hst->status;
    if (rc == LSGPU_NO_CONVERGENCE)
      h->err = hst->err_code == 1 ? "no point to minimize" : hst->err_code == 2 ? "normal matrix not positive definite"
             : hst->err_code == 4 ? "non-finite point-to-point solution"
             : hst->err_code == 5 ? "RobustOutlierFilter: no valid match or a MAD scale of 0"
             : hst->err_code == 6 ? "RobustOutlierFilter: a weight is not finite" : "NaN in transformation checker";
    st.iterations = it;
    st.converged = hst->converged;
    st.stragglers = (int64_t)hst->stragglers;
    // The per-iteration trace stays in device memory until lsgpu_icp_get_trace asks for it (the synchronous copy cost every
    // alignment 37 us -- 5 % of a 200 k-point pair -- for a record nobody but the tests and the profiler reads); the two
    // statistics that came out of it travel with the loop state.
    h->trace.clear();
    h->trace_on_device = (size_t)std::min(it, max_it);
    h->rb_trace_n = robust ? h->trace_on_device : 0;
    h->na_trace_n = angle ? h->trace_on_device : 0;
    h->trace_knn_us.clear();
    if (it > 0) { st.final_limit = hst->last_limit; st.final_n_used = (int64_t)hst->last_used; }
    if (rc == LSGPU_OK) {  // step 7
      float Tmean[16], tmp[16];
      hostmath::identity4(Tmean);
      for (int d = 0; d < 3; ++d) Tmean[12 + d] = h->mean[d];
      hostmath::mul4(hst->T_iter, T_rm_in, tmp);
      hostmath::mul4(Tmean, tmp, T_out);
    }
    // kNN timing: launches that actually ran are the first `it` (+ retries) enqueued ones
    size_t t = 0;
    for (size_t i = 0; i < h->knn_events_used && i < ev_of_launch.size(); ++i) {
      const auto& e = h->knn_events[ev_of_launch[i]];
      float m1 = 0.f, m2 = 0.f;
      if (hipEventElapsedTime(&m1, e.a, e.b) != hipSuccess || (e.second && hipEventElapsedTime(&m2, e.b, e.c) != hipSuccess)) {
        (void)hipGetLastError();
        continue;
      }
      if (st.knn_launches >= it + st.cap_retries) break;  // the rest exited immediately (enqueued past the end)
      if (m1 < 0.02f) continue;  // exited immediately (enqueued behind an iteration that had to be repeated)
      st.t_knn_main_ms += m1; st.t_knn_fallback_ms += m2; st.t_knn_ms += m1 + m2; st.knn_launches++;
      float m3 = 0.f, m4 = 0.f;
      if (hipEventElapsedTime(&m3, e.second ? e.c : e.b, e.d) == hipSuccess && hipEventElapsedTime(&m4, e.d, e.e) == hipSuccess) { st.t_select_ms += m3; st.t_ne_ms += m4; }
      else (void)hipGetLastError();
      if (t < h->trace_on_device) { h->trace_knn_us.push_back({m1 * 1e3f, m2 * 1e3f}); ++t; }
    }
    if (h->time_comm) {   // time inside the collectives (launches enqueued behind the end exit at once and add next to nothing)
      for (size_t i = 0; i < h->comm_events_used; ++i) {
        float m = 0.f;
        if (hipEventElapsedTime(&m, h->comm_events[i].first, h->comm_events[i].second) == hipSuccess) { st.t_comm_ms += m; st.comm_calls++; }
        else (void)hipGetLastError();
      }
    }
    st.direction_index_launches = pol.cone_launches;   // (enqueued; those behind the end of the loop exited at once)
    st.direction_index_occupancy = h->cone_decided ? h->cone_occupancy : 0.f;
    st.direction_index_heavy_share = pol.cone_heavy;
    st.pad_ = pol.sel_retries;  // (select predictions that missed; informational)
    st.committed_select_iterations = pol.committed_iterations;
    st.spread_tiles = (int)hst->n_spread;
    st.t_total_ms = wall_ms() - t0;
    return rc;
  }
};

// PointToPlaneWithCovErrorMinimizer: the pass after a loop that returned LSGPU_OK.  The covariance a caller can observe is that
// of the last executed iteration: its pairs at the pose it matched at.  That pose is the loop state's T_rows_prev (the update
// keeps the transform it replaces; the identity after one iteration), its step comes from the normal equations of its trace
// record (lsgpu_point_to_plane_solve, as a caller would take it), its limit is the state's last_limit.  The pairs are searched
// once more, exactly, with the search of lsgpu_knn -- the loop's own ids / d2 are exact only inside the radius cap and the
// kept lanes of the direction index -- and brought into the caller's order, so that the sums are those of
// lsgpu_point_to_plane_cov on the same inputs, bit for bit.
static int covariance_pass(AlignRun& run, lsgpu_icp_stats& st) {
  lsgpu_icp* h = run.h;
  const IcpState* hst = run.hst;
  const int64_t nq = run.nq;
  const int it = hst->iter;
  if (it < 1 || it > run.max_it) return LSGPU_OK;   // (no executed iteration: the record stays "none")
  Mat34 Tm;
  for (int i = 0; i < 12; ++i) Tm.m[i] = hst->T_rows_prev[i];
  HIPC(hipMemcpyAsync(&h->pin->cov_trace, h->trace_dev.p + (it - 1), sizeof(lsgpu_iter_trace), hipMemcpyDeviceToHost, h->stream));
  HIPC(h->cov_pts.reserve((size_t)nq)); HIPC(h->ids_io.reserve((size_t)nq)); HIPC(h->d2_io.reserve((size_t)nq));
  int rc = LSGPU_OK;
  if (matcher_max_d2(h) < INFINITY) {   // KDTreeMatcher maxDist: the bounded k-best search with k = 1 (as lsgpu_knn)
    rc = run_knn_k(h, 1, Tm, nullptr, true, false);
    if (rc) return rc;
    hipLaunchKernelGGL(k_knnk_unpermute, dim3(nblk(nq)), dim3(256), 0, h->stream, h->rdq.p, (int)nq, 1, h->kmatch.p,
                       h->kd2.p, h->pts.p, h->ids_io.p, h->d2_io.p);
  } else {
    policy::Iteration probe;   // a seeded, uncapped, wide search outside any loop
    probe.seed = true; probe.capped = false; probe.wide = true;
    h->pol.begin_align(false, false, false, 0.f);
    rc = run_knn(h, Tm, nullptr, probe, false);
    if (rc) return rc;
    hipLaunchKernelGGL(k_knn_unpermute, dim3(nblk(nq)), dim3(256), 0, h->stream, h->rdq.p, (int)nq,
                       h->ids.p, h->d2.p, h->pts.p, h->ids_io.p, h->d2_io.p);
  }
  hipLaunchKernelGGL(k_cov_unpermute_points, dim3(nblk(nq)), dim3(256), 0, h->stream, h->rdq.p, (int)nq, h->cov_pts.p);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(h->stream));
  const lsgpu_iter_trace& tr = h->pin->cov_trace;
  double sums[27];
  {
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int c = a; c < 6; ++c) sums[k++] = tr.A[a * 6 + c];
    for (int a = 0; a < 6; ++a) sums[21 + a] = tr.b[a];
  }
  float dT[16];
  if (lsgpu_point_to_plane_solve(sums, dT) != LSGPU_OK) { h->quality_state = 2; return LSGPU_OK; }   // (the loop solved it: not reached)
  rc = cov_sums(h, h->cov_pts.p, nq, Tm, h->ids_io.p, h->d2_io.p, hst->last_limit, dT);
  if (rc) return rc;
  const double* s = h->pin->cov;
  lsgpu_icp_quality q;
  std::memset(&q, 0, sizeof(q));
  q.residual = s[43];
  q.n_pairs = (int64_t)s[42];
  q.used_ratio = (float)((double)q.n_pairs / (double)nq);
  const int rs = lsgpu_point_to_plane_cov_solve(s, h->mods.cov_cfg.sensor_std_dev, q.covariance);
  h->quality = q;
  h->quality_state = rs == LSGPU_OK ? 1 : 2;
  st.t_total_ms = wall_ms() - run.t0;
  return LSGPU_OK;
}

extern "C" {

static int align_run(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float T_init[16], float T_out[16],
                     lsgpu_icp_stats* stats, AlignExtras extras) {
  if (!h || !T_init || !T_out) return LSGPU_BAD_ARG;
  h->err.clear();
  std::memcpy(T_out, T_init, 16 * sizeof(float));
  lsgpu_icp_stats st;
  std::memset(&st, 0, sizeof(st));
  if (stats) *stats = st;
  h->quality_state = 0;
  AlignRun run{h, reading_xyz1, nq, T_init, extras};
  int rc = run.start();
  if (!rc) rc = run.init_loop_state();
  if (!rc) rc = run.configure_policy();
  if (!rc) rc = run.feed();
  if (rc) return rc;
  rc = run.harvest(T_out, st);
  if ((rc == LSGPU_OK || rc == LSGPU_NO_CONVERGENCE) && h->mods.bound() && run.check_bound()) {
    std::memcpy(T_out, T_init, 16 * sizeof(float));
    rc = LSGPU_NO_CONVERGENCE;
  }
  if (rc == LSGPU_OK && h->mods.cov_on) {
    const int rq = covariance_pass(run, st);
    if (rq) { std::memcpy(T_out, T_init, 16 * sizeof(float)); return rq; }
  }
  if (stats) *stats = st;
  return rc;
}

int lsgpu_icp_align(lsgpu_icp* h, const float* reading_xyz1, int64_t nq, const float T_init[16],
                    float T_out[16], lsgpu_icp_stats* stats) {
  return align_run(h, reading_xyz1, nq, T_init, T_out, stats, {});
}

int lsgpu_icp_align_batch(lsgpu_icp* const* handles, int n_handles, int64_t n_pairs,
                          const float* const* reference_xyz1, const float* const* reference_normals,
                          const int64_t* n_reference, const float* const* reading_xyz1,
                          const int64_t* n_reading, const float* T_init, float* T_out,
                          lsgpu_icp_stats* stats, int* rc) {
  if (!handles || n_handles < 1 || n_pairs < 0) return LSGPU_BAD_ARG;
  if (n_pairs == 0) return LSGPU_OK;
  if (!reference_xyz1 || !reference_normals || !n_reference || !reading_xyz1 || !n_reading || !T_init || !T_out)
    return LSGPU_BAD_ARG;
  for (int k = 0; k < n_handles; ++k)
    if (!handles[k] || handles[k]->device != handles[0]->device || handles[k]->comm) return LSGPU_BAD_ARG;
  std::vector<int> codes((size_t)n_pairs, LSGPU_OK);
  // handle k owns pairs k, k + n_handles, ...: a static assignment, each pair is one independent,
  // deterministic {set_reference, align} on that handle's stream
  auto worker = [&](int k) {
    lsgpu_icp* h = handles[k];
    // Reference reuse (the part that is exact): a pair that names the SAME reference buffers as the
    // previous pair of this handle (same pointers, same size -- many readings against one map, loop-closure candidates
    // against one sub-map) keeps the centred, sorted reference, its chunks and its cell tables: steps 2-3 of ICP::compute
    // depend on the reference alone.  Bit-identical with rebuilding (tests/test_gpu_parity.py::
    // test_align_batch_reuses_a_shared_reference).
    const float* have_ref = nullptr; const float* have_nrm = nullptr; int64_t have_n = -1;
    for (int64_t i = k; i < n_pairs; i += n_handles) {
      float* To = T_out + 16 * i;
      const float* Ti = T_init + 16 * i;
      std::memcpy(To, Ti, 16 * sizeof(float));
      if (stats) std::memset(&stats[i], 0, sizeof(lsgpu_icp_stats));
      int c = LSGPU_OK;
      const bool same = have_n > 0 && reference_xyz1[i] == have_ref && reference_normals[i] == have_nrm && n_reference[i] == have_n;
      if (!same) {
        c = lsgpu_icp_set_reference(h, reference_xyz1[i], reference_normals[i], n_reference[i]);
        have_ref = reference_xyz1[i]; have_nrm = reference_normals[i]; have_n = c == LSGPU_OK ? n_reference[i] : -1;
      }
      if (c == LSGPU_OK) c = lsgpu_icp_align(h, reading_xyz1[i], n_reading[i], Ti, To, stats ? &stats[i] : nullptr);
      if (stats) stats[i].reference_reused = same ? 1 : 0;
      codes[(size_t)i] = c;
    }
  };
  const int nt = (int)std::min<int64_t>(n_handles, n_pairs);
  std::vector<std::thread> pool;
  for (int k = 1; k < nt; ++k) pool.emplace_back(worker, k);
  worker(0);
  for (auto& t : pool) t.join();
  int ret = LSGPU_OK;
  for (int64_t i = 0; i < n_pairs; ++i) {
    const int c = codes[(size_t)i];
    if (rc) rc[i] = c;
    if (c != LSGPU_OK && c != LSGPU_NO_CONVERGENCE) { if (ret == LSGPU_OK || ret == LSGPU_NO_CONVERGENCE) ret = c; }
    else if (c == LSGPU_NO_CONVERGENCE && ret == LSGPU_OK) ret = c;
  }
  return ret;
}

// dev only: device allocations, pinned allocations, events and streams the library holds at the moment (all handles of the process)
long lsgpu_dev_live_resources(void) { return g_live.load(); }
// dev only (LSGPU_KNN_STATS build): per-wave records of the last k_knn_tile launch / global counters
int lsgpu_dev_knn_wave_stats(lsgpu_icp* h, unsigned int* out, int nwaves) {
  if (!h) return LSGPU_BAD_ARG;
  if (!out) { HIPC(h->knn_dbg_wave.reserve((size_t)nwaves)); HIPC(hipMemset(h->knn_dbg_wave.p, 0, (size_t)nwaves * 16)); return LSGPU_OK; }
  HIPC(hipStreamSynchronize(h->stream));
  HIPC(hipMemcpy(out, h->knn_dbg_wave.p, (size_t)nwaves * 16, hipMemcpyDeviceToHost));
  return LSGPU_OK;
}
#ifdef LSGPU_KNN_STATS
int lsgpu_dev_tree_phases(lsgpu_icp* h, unsigned long long out[64]) {  // stats build only (devtools/tree_phases.py)
  if (!h) return LSGPU_BAD_ARG;
  HIPC(hipStreamSynchronize(h->stream));
  HIPC(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tree_dbg), 512));
  return LSGPU_OK;
}
int lsgpu_dev_cone_phases(lsgpu_icp* h, unsigned int* out, int ntiles) {  // stats build only (devtools/cone_phases.py)
  // out == nullptr: (re)arm the record buffer for `ntiles` waves per iteration; otherwise copy the records back
  if (!h || ntiles <= 0) return LSGPU_BAD_ARG;
  static uint32_t* rec = nullptr;
  static size_t rec_words = 0;
  const size_t words = (size_t)kConeRecIters * (size_t)ntiles * 16;
  HIPC(hipStreamSynchronize(h->stream));
  if (!out) {
    if (words > rec_words) { if (rec) HIPC(hipFree(rec)); HIPC(hipMalloc((void**)&rec, words * 4)); rec_words = words; }
    HIPC(hipMemset(rec, 0, words * 4));
    HIPC(hipMemcpyToSymbol(HIP_SYMBOL(g_cone_rec), &rec, sizeof(rec)));
    return LSGPU_OK;
  }
  if (!rec || words > rec_words) return LSGPU_BAD_ARG;
  HIPC(hipMemcpy(out, rec, words * 4, hipMemcpyDeviceToHost));
  return LSGPU_OK;
}
int lsgpu_dev_ne_phases(lsgpu_icp* h, unsigned long long out[24]) {  // stats build only (devtools/ne_phases.py)
  if (!h) return LSGPU_BAD_ARG;
  HIPC(hipStreamSynchronize(h->stream));
  HIPC(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ne_dbg), 192));
  return LSGPU_OK;
}
#endif
int lsgpu_dev_knn_counters(lsgpu_icp* h, unsigned long long out[8]) {
  if (!h) return LSGPU_BAD_ARG;
  if (!h->knn_dbg.p) {
    HIPC(h->knn_dbg.reserve(8));
    HIPC(hipMemset(h->knn_dbg.p, 0, 64));
    std::memset(out, 0, 64);
    return LSGPU_OK;
  }
  HIPC(hipStreamSynchronize(h->stream));
  HIPC(hipMemcpy(out, h->knn_dbg.p, 64, hipMemcpyDeviceToHost));
  HIPC(hipMemset(h->knn_dbg.p, 0, 64));
  return LSGPU_OK;
}

int lsgpu_icp_get_trace(lsgpu_icp* h, lsgpu_iter_trace* out, int cap) {
  if (!h || !out || cap <= 0) return 0;
  if (h->trace_on_device) {   // the last alignment's records are still where the device wrote them
    h->trace.resize(h->trace_on_device);
    if (hipSetDevice(h->device) != hipSuccess ||
        hipMemcpy(h->trace.data(), h->trace_dev.p, h->trace.size() * sizeof(lsgpu_iter_trace), hipMemcpyDeviceToHost) != hipSuccess) {
      (void)hipGetLastError();
      h->trace.clear();
    }
    for (size_t t = 0; t < h->trace.size() && t < h->trace_knn_us.size(); ++t) {
      h->trace[t].knn_main_us = h->trace_knn_us[t].first; h->trace[t].knn_fallback_us = h->trace_knn_us[t].second;
    }
    h->trace_on_device = 0;
  }
  const int n = std::min<int>(cap, (int)h->trace.size());
  std::memcpy(out, h->trace.data(), (size_t)n * sizeof(lsgpu_iter_trace));
  return n;
}

}  // extern "C"
