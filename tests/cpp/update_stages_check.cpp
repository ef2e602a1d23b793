// update_stages_check.cpp -- the staged per-iteration update (icp_update_stage, csrc/lsgpu_solve.hip.h) against the serial
// icp_update_lane, both compiled for the host: "for each stage, for each thread index" must leave the whole loop state, the
// checker history, the trace records and the robust state byte for byte as the serial function leaves them.  The threads of a
// stage are run in three orders (ascending, descending, shuffled): a stage whose pieces depended on one another would show.
//
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -I include update_stages_check.cpp -o check
//   ./check [file with the 6x6 system of tests/golden/icp_pair4k.npz: 36 doubles A, 6 doubles b, double used, double limit]
//
// For every minimizer (point-to-plane, point-to-point, force4DOF, force2D), with and without the robust filter's part:
//   chains of iterations over random symmetric positive definite systems (point-to-point: sums of random point pairs) that
//   end by the counter or by the differential checker, with the select window armed and not armed, in both select modes,
//   with and without a cap, with a trace shorter than the chain;
//   every exit: done already set, select failed, cap failed, no pair, the robust filter's two refusals, a non-positive
//   pivot in every column, a NaN solution, a NaN in the checker, a non-finite point-to-point step.
// Each scenario states the status it must end with, so a path that was not taken fails the check.
#define LSGPU_UPDATE_HOST_CHECK
#include "../../laser_slam_amd/csrc/lsgpu_solve.hip.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace lsgpu;

namespace {

constexpr int kIterCap = 40;    // the largest max_iter a scenario uses
constexpr int kThreads = 256;

struct World {   // everything an update may write
  IcpState st;
  RobustState rs;
  float chk[8 * (kIterCap + 2)];
  lsgpu_iter_trace tr[kIterCap];
  lsgpu_robust_trace rtr[kIterCap];
};

struct Rng {
  std::mt19937_64 g;
  explicit Rng(uint64_t s) : g(s) {}
  double u() { return (double)(g() >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)
  double sym() { return 2.0 * u() - 1.0; }
  int below(int n) { return (int)(g() % (uint64_t)n); }
};

int g_failures = 0;
long g_steps = 0;
int g_order[3][kThreads];

void fail(const char* what, const char* part) {
  if (g_failures++ < 20) std::fprintf(stderr, "MISMATCH %s: %s differs\n", what, part);
}

void init_world(World* w, int max_iter, int smooth, float lim_rot, float lim_trans, int sel_wide, int cap_enabled) {
  std::memset(w, 0, sizeof(*w));
  std::memset(w->tr, 0xA5, sizeof(w->tr));     // (a record the update must not touch stays recognisable)
  std::memset(w->rtr, 0xA5, sizeof(w->rtr));
  IcpState& s = w->st;
  hostmath::identity4(s.T_iter);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) s.T_rows[r * 4 + c] = s.T_iter[c * 4 + r];
  s.prev_limit = INFINITY; s.cap2 = INFINITY;
  s.cap_enabled = cap_enabled; s.max_iter = max_iter; s.smooth = smooth; s.lim_rot = lim_rot; s.lim_trans = lim_trans;
  s.sel_wide = sel_wide;
  hostmath::CheckerState cs{0, 0};
  hostmath::checker_push(&cs, w->chk, s.T_iter);
  s.counter = cs.counter; s.n_hist = cs.n_hist;
}

// the 32 doubles the last block hands the update: the 29 sums, the limit, the stragglers, the heavy tiles
void pack_plane(const double A[36], const double b[6], double used, double limit, double ne[32]) {
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c) ne[k++] = A[a * 6 + c];
  for (int a = 0; a < 6; ++a) ne[21 + a] = b[a];
  ne[27] = used; ne[28] = 0.25 * used; ne[29] = limit; ne[30] = 3.0; ne[31] = 7.0;
}

// A = M M^T + I (x scale), b = A x for a step x of the given size
void random_spd(Rng& r, double scale, double step, double A[36], double b[6]) {
  double M[36], x[6];
  for (double& m : M) m = r.sym();
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double s = i == j ? 1.0 : 0.0;
      for (int k = 0; k < 6; ++k) s += M[i * 6 + k] * M[j * 6 + k];
      A[i * 6 + j] = scale * s;
    }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < i; ++j) A[i * 6 + j] = A[j * 6 + i];
  for (double& v : x) v = step * r.sym();
  for (int i = 0; i < 6; ++i) {
    b[i] = 0.0;
    for (int j = 0; j < 6; ++j) b[i] += A[i * 6 + j] * x[j];
  }
}

// point-to-point sums of n random pairs q = R p + t + noise, R a rotation of `step` radians
void random_p2p(Rng& r, int n, double step, double limit, double ne[32]) {
  for (int i = 0; i < 32; ++i) ne[i] = 0.0;
  double ax[3] = {r.sym(), r.sym(), r.sym()};
  const double an = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-12;
  for (double& a : ax) a /= an;
  const double ang = step * r.sym(), s = std::sin(ang), c = std::cos(ang);
  double R[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (i == j ? c : 0.0) + (1.0 - c) * ax[i] * ax[j];
  R[1] -= s * ax[2]; R[2] += s * ax[1]; R[3] += s * ax[2]; R[5] -= s * ax[0]; R[6] -= s * ax[1]; R[7] += s * ax[0];
  const double t[3] = {step * r.sym(), step * r.sym(), step * r.sym()};
  for (int i = 0; i < n; ++i) {
    const double p[3] = {10.0 * r.sym(), 10.0 * r.sym(), 2.0 * r.sym()};
    double q[3];
    for (int a = 0; a < 3; ++a) q[a] = R[a * 3] * p[0] + R[a * 3 + 1] * p[1] + R[a * 3 + 2] * p[2] + t[a] + 1e-3 * step * r.sym();
    for (int a = 0; a < 3; ++a) { ne[a] += p[a]; ne[3 + a] += q[a]; }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) ne[6 + 3 * a + b] += q[a] * p[b];
  }
  ne[27] = (double)n; ne[28] = 0.5 * n; ne[29] = limit; ne[30] = 1.0; ne[31] = 0.0;
}

struct Step {   // one update: its inputs
  double ne[32];
  int sel_failed = 0, capped = 0, trace_cap = kIterCap;
  RobustIter rb{};   // (state / trace are pointed at the world's)
};

// both forms on copies of *w; *w becomes the serial result.  false: they differ.
template <int MIN, bool RB>
bool run_step(World* w, const Step& in, const char* what) {
  bool same = true;
  static World ser, stg;   // (static: the records are large)
  ser = *w;
  RobustIter ra = in.rb; ra.state = &ser.rs; ra.trace = ser.rtr;
  icp_update_lane<MIN, RB>(&ser.st, in.ne, ser.chk, ser.tr, in.trace_cap, in.capped, nullptr, in.sel_failed, RB ? &ra : nullptr);
  for (int order = 0; order < 3; ++order) {
    stg = *w;
    RobustIter rs = in.rb; rs.state = &stg.rs; rs.trace = stg.rtr;
    UpdateCtx c;
    std::memset(&c, 0xCD, sizeof(c));   // (what an earlier update left in the context must not matter)
    const UpdateArgs ua{&stg.st, in.ne, stg.chk, stg.tr, in.trace_cap, in.capped, in.sel_failed, RB ? &rs : nullptr};
    for (int s = 0; s < kUpdateStages; ++s)
      for (int k = 0; k < kThreads; ++k) icp_update_stage<MIN, RB>(s, g_order[order][k], c, ua);
    if (std::memcmp(&ser.st, &stg.st, sizeof(IcpState))) { fail(what, "IcpState"); same = false; }
    if (std::memcmp(ser.chk, stg.chk, sizeof(ser.chk))) { fail(what, "checker history"); same = false; }
    if (std::memcmp(ser.tr, stg.tr, sizeof(ser.tr))) { fail(what, "trace record"); same = false; }
    if (std::memcmp(ser.rtr, stg.rtr, sizeof(ser.rtr))) { fail(what, "robust trace"); same = false; }
    if (std::memcmp(&ser.rs, &stg.rs, sizeof(ser.rs))) { fail(what, "robust state"); same = false; }
  }
  *w = ser;
  ++g_steps;
  return same;
}

void expect(bool cond, const char* what, const char* why) {
  if (!cond) { ++g_failures; std::fprintf(stderr, "SCENARIO %s: %s\n", what, why); }
}
void expect_end(const World& w, int status, int err, int converged, const char* what) {
  expect(w.st.done == 1 && w.st.status == status && w.st.err_code == err && w.st.converged == converged, what,
         "the serial update did not take the path the scenario is about");
}

template <int MIN>
void make_input(Rng& r, double step, double limit, Step* in) {
  if (MIN == kPointToPoint) { random_p2p(r, 24, step, limit, in->ne); return; }
  double A[36], b[6];
  random_spd(r, std::pow(10.0, 1.0 + 4.0 * r.u()), step, A, b);
  pack_plane(A, b, 3000.0, limit, in->ne);
}

RobustIter robust_proto(Rng& r) {
  RobustIter rb{};
  rb.used = 2500; rb.bad = 0.0; rb.scale = (float)(0.1 + r.u()); rb.median = (float)r.u(); rb.recomputed = r.below(2); rb.mad = 1;
  return rb;
}

struct Counts { long plain = 0, by_counter = 0, by_diff = 0, armed = 0, not_armed = 0, untraced = 0, capped = 0; };

template <int MIN, bool RB>
void chains(Rng& r, int n_chains, Counts* n, const char* what) {
  for (int ch = 0; ch < n_chains; ++ch) {
    World w;
    const int max_iter = 3 + r.below(kIterCap - 2), smooth = 1 + r.below(4), sel_wide = r.below(2), cap_enabled = r.below(2);
    const bool settle = r.below(2) != 0, steady = r.below(2) != 0;   // steps that shrink; limits that move little
    init_world(&w, max_iter, smooth, 1e-5f, 1e-4f, sel_wide, cap_enabled);
    const int trace_cap = r.below(4) == 0 ? 1 + r.below(max_iter) : kIterCap;
    double step = 0.05, limit = 0.01 + r.u();
    for (int it = 0; it < kIterCap + 2 && !w.st.done; ++it) {
      Step in;
      in.trace_cap = trace_cap;
      in.rb = robust_proto(r);
      make_input<MIN>(r, step, limit, &in);
      if (cap_enabled && w.st.cap2 < INFINITY && r.below(2)) { in.capped = 1; ++n->capped; }   // (the limit stays below the cap: x 1.1)
      if (!run_step<MIN, RB>(&w, in, what)) return;
      if (w.st.iter - 1 >= trace_cap) ++n->untraced;
      if (!w.st.done) ++n->plain;
      else if (w.st.status == 0 && w.st.converged) ++n->by_diff;
      else if (w.st.status == 0) ++n->by_counter;
      else expect(false, what, "a chain ended with an error");
      if (w.st.sel_mode) ++n->armed; else ++n->not_armed;
      if (settle) step *= 0.2;
      limit *= steady ? 1.0 + 0.02 * r.sym() : (in.capped || cap_enabled ? 0.6 + 0.45 * r.u() : 0.3 + 2.7 * r.u());
    }
    expect(w.st.done == 1, what, "a chain did not end");
  }
}

// a world two plain iterations into an alignment
template <int MIN, bool RB>
void warm_world(Rng& r, World* w, int sel_wide, const char* what) {
  init_world(w, 30, 3, 1e-5f, 1e-4f, sel_wide, 1);
  for (int it = 0; it < 2; ++it) {
    Step in;
    in.rb = robust_proto(r);
    make_input<MIN>(r, 0.02, 0.5, &in);
    run_step<MIN, RB>(w, in, what);
  }
  expect(!w->st.done && w->st.iter == 2, what, "warm-up iterations ended the alignment");
}

template <int MIN, bool RB>
void exits(Rng& r, const double* golden, const char* what) {
  constexpr int N = MIN == kPointToPlane ? 6 : MIN == kPointToPlane4Dof ? 4 : MIN == kPointToPlane2D ? 3 : 0;   // LLT columns
  constexpr int F = MIN == kPointToPlane ? 0 : 2;
  for (int sel_wide = 0; sel_wide < 2; ++sel_wide) {
    World w0, w;
    warm_world<MIN, RB>(r, &w0, sel_wide, what);
    Step base;
    base.rb = robust_proto(r);
    make_input<MIN>(r, 0.02, 0.5, &base);
    {   // done already set: nothing moves
      w = w0; w.st.done = 1; const World before = w;
      run_step<MIN, RB>(&w, base, what);
      expect(!std::memcmp(&before, &w, sizeof(World)), what, "an update of a finished alignment wrote something");
    }
    {   // select failed
      w = w0; Step in = base; in.sel_failed = 1;
      run_step<MIN, RB>(&w, in, what);
      expect_end(w, kStatusSelFailed, 0, 0, what);
      expect(w.st.sel_fails == 1 && w.st.sel_mode == 0, what, "select failure not recorded");
    }
    {   // cap failed: the limit lies above the cap of a capped launch
      w = w0; Step in = base; in.capped = 1; w.st.cap2 = 0.25f;
      run_step<MIN, RB>(&w, in, what);
      expect_end(w, kStatusCapFailed, 0, 0, what);
    }
    {   // no pair
      w = w0; Step in = base; in.ne[27] = 0.0; in.rb.used = 0;
      run_step<MIN, RB>(&w, in, what);
      expect_end(w, LSGPU_NO_CONVERGENCE, 1, 0, what);
      expect(w.st.stragglers == w0.st.stragglers + (unsigned long long)base.ne[30], what, "stragglers of a refused iteration not counted");
    }
    if (RB) {
      w = w0; Step in = base; in.rb.scale = 0.f;
      run_step<MIN, RB>(&w, in, what);
      expect_end(w, LSGPU_NO_CONVERGENCE, 5, 0, what);
      w = w0; in = base; in.rb.bad = 2.0;
      run_step<MIN, RB>(&w, in, what);
      expect_end(w, LSGPU_NO_CONVERGENCE, 6, 0, what);
    }
    for (int j = 0; j < N; ++j) {   // a non-positive pivot in column j (of the sub-system): slot of the diagonal (F + j, F + j)
      const int a = F + j, slot = a * 6 - a * (a - 1) / 2;
      for (int kind = 0; kind < 2; ++kind) {
        w = w0; Step in = base; in.ne[slot] = kind ? -1.0 : (j == 0 ? 0.0 : in.ne[slot] * 1e-9);
        run_step<MIN, RB>(&w, in, what);
        expect_end(w, LSGPU_NO_CONVERGENCE, 2, 0, what);
      }
    }
    if (N) {   // every pivot positive, a NaN in the solution
      w = w0; Step in = base; in.ne[21 + F + 1] = NAN;
      run_step<MIN, RB>(&w, in, what);
      expect_end(w, LSGPU_NO_CONVERGENCE, 2, 0, what);
      double A[36], b[6]; float x[6];
      hostmath::unpack_normal_eq(base.ne, A, b);
      expect(hostmath::llt_solve6(A, b, x), what, "the NaN scenario's matrix is not positive definite");
    }
    {   // a NaN in the checker: the step is finite, the transform it is applied to is not (history longer than `smooth`)
      w = w0; w.st.T_iter[13] = NAN;
      run_step<MIN, RB>(&w, base, what);
      expect_end(w, LSGPU_NO_CONVERGENCE, 3, 0, what);
    }
    if (MIN == kPointToPoint) {   // a non-finite point-to-point step
      w = w0; Step in = base; in.ne[3] = INFINITY;
      run_step<MIN, RB>(&w, in, what);
      expect_end(w, LSGPU_NO_CONVERGENCE, 4, 0, what);
      if (RB) {   // the weights summed to nothing although pairs were counted
        w = w0; in = base; in.ne[27] = 0.0;
        run_step<MIN, RB>(&w, in, what);
        expect_end(w, LSGPU_NO_CONVERGENCE, 4, 0, what);
      }
    }
    {   // the counter ends it: max_iter 3, the third iteration
      w = w0; w.st.max_iter = 3;
      run_step<MIN, RB>(&w, base, what);
      expect_end(w, 0, 0, 0, what);
    }
    if (golden && N) {   // the first system of the 4 k golden pair: a plain iteration, window not armed (no earlier limit)
      init_world(&w, 40, 3, 1e-5f, 1e-4f, sel_wide, 1);
      Step in; in.rb = robust_proto(r);
      pack_plane(golden, golden + 36, golden[42], golden[43], in.ne);
      run_step<MIN, RB>(&w, in, what);
      expect(!w.st.done && w.st.iter == 1 && w.st.sel_mode == 0, what, "the golden system did not give a plain first iteration");
      in.ne[29] = golden[43] * 0.98;   // ... and a second one whose limit moved by 2 %: armed in the wide mode
      run_step<MIN, RB>(&w, in, what);
      expect(!w.st.done && w.st.iter == 2 && (w.st.sel_mode == 1) == (sel_wide == 1 || (__float_as_uint((float)in.ne[29]) >> 20) == (__float_as_uint((float)golden[43]) >> 20)),
             what, "the golden system's second iteration left the window in the wrong state");
    }
  }
}

template <int MIN, bool RB>
void check_all(uint64_t seed, const double* golden, const char* what) {
  Rng r(seed);
  Counts n;
  chains<MIN, RB>(r, 120, &n, what);
  expect(n.plain > 0 && n.by_counter > 0 && n.by_diff > 0, what, "the chains did not end both ways");
  expect(n.armed > 0 && n.not_armed > 0, what, "the chains did not see the window armed and not armed");
  expect(n.untraced > 0 && n.capped > 0, what, "the chains did not outrun a trace or run capped");
  exits<MIN, RB>(r, golden, what);
  std::printf("%-28s plain %ld, by counter %ld, by differential %ld, armed %ld, not armed %ld, past the trace %ld, capped %ld\n",
              what, n.plain, n.by_counter, n.by_diff, n.armed, n.not_armed, n.untraced, n.capped);
}

}  // namespace

int main(int argc, char** argv) {
  std::vector<double> golden;
  if (argc > 1) {
    golden.resize(44);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(golden.data(), sizeof(double), 44, f) != 44) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
  }
  const double* g = golden.empty() ? nullptr : golden.data();
  Rng perm(99);
  for (int k = 0; k < kThreads; ++k) { g_order[0][k] = k; g_order[1][k] = kThreads - 1 - k; g_order[2][k] = k; }
  for (int k = kThreads - 1; k > 0; --k) std::swap(g_order[2][k], g_order[2][perm.below(k + 1)]);

  check_all<kPointToPlane, false>(1, g, "point-to-plane");
  check_all<kPointToPlane, true>(2, g, "point-to-plane, robust");
  check_all<kPointToPoint, false>(3, g, "point-to-point");
  check_all<kPointToPoint, true>(4, g, "point-to-point, robust");
  check_all<kPointToPlane4Dof, false>(5, g, "force4DOF");
  check_all<kPointToPlane4Dof, true>(6, g, "force4DOF, robust");
  check_all<kPointToPlane2D, false>(7, g, "force2D");
  check_all<kPointToPlane2D, true>(8, g, "force2D, robust");
  if (g_failures) { std::fprintf(stderr, "%d failure(s) in %ld updates\n", g_failures, g_steps); return 1; }
  std::printf("UPDATE_STAGES_OK %ld updates%s\n", g_steps, g ? ", golden system included" : "");
  return 0;
}
