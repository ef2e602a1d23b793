// robust_policy_check.cpp -- CPU driver of the launch policy (laser_slam_amd/csrc/lsgpu_policy.h) for handles with
// RobustOutlierFilter: such a handle takes the chain plan whatever the four chain fields hold, the plan is that of any
// chain, and it marks the iterations that recompute the MAD scale (nbIterationForScale) -- the only ones that launch the
// median's and the MAD's select.  A configuration without the filter is planned as before.
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "../../laser_slam_amd/csrc/lsgpu_policy.h"

using namespace lsgpu::policy;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the `mad` marks of the first n iterations of an alignment (iteration 1 = the seeded one), looks included
static unsigned marks(bool robust_mad, int scale_iters, bool kmatch, int n_want) {
  Config c; c.enq_limit = 400; c.chain = true; c.kmatch = kmatch; c.robust_mad = robust_mad; c.robust_scale_iters = scale_iters;
  State s; s.begin_align(true, true, false, 2.f);
  unsigned m = 0u;
  int n = 0;
  Iteration it = s.plan(c, true, true, true, true, false);
  CHECK(it.seed && it.knn && !it.capped && !it.predicted && !it.committed && it.full_select && !it.cone_iter && !it.price && it.ordinal == 0);
  m |= it.mad ? 1u : 0u; ++n;
  s.enq = 1; s.since_check = 1;
  while (n < n_want) {
    while (n < n_want && s.next_in_group(c, &it)) {
      CHECK(!it.seed && it.knn && !it.capped && !it.predicted && !it.committed && it.full_select && !it.cone_iter && it.ordinal == n);
      CHECK(s.kernel(c, it, true) == KnnKernel::Tile);
      m |= it.mad ? 1u << n : 0u; ++n;
    }
    Iteration ahead; int q = 0;
    if (n < n_want && s.lookahead_iteration(c, &ahead)) { CHECK(ahead.ordinal == n); m |= ahead.mad ? 1u << n : 0u; ++n; q = 1; }
    LookInput li; li.iter = n - q; li.nq = 1000;
    CHECK(s.on_look(c, li, q, -1.f) == LookVerdict::Continue);   // the chain plan never repeats an iteration
  }
  CHECK(s.cap_retries == 0 && s.sel_retries == 0 && s.committed_iterations == 0 && s.cone_launches == 0);
  return m;
}

int main() {
  CHECK(!chain_fields(0.f, 0.f, 0.f, 0.f) && !chain_fields(0.f, 0.f, 0.f, 0.f, false));
  CHECK(chain_fields(0.f, 0.f, 0.f, 0.f, true) && chain_fields(INFINITY, INFINITY, 0.f, 0.f, true) && chain_fields(0.5f, 0.f, 0.f, 0.f, true));
  for (bool kmatch : {false, true}) {
    CHECK(marks(true, 0, kmatch, 20) == (1u << 20) - 1u);     // nbIterationForScale 0: every iteration
    CHECK(marks(true, 3, kmatch, 20) == 0x7u);                // 3: iterations 1..3, frozen from the 4th on
    CHECK(marks(true, 1, kmatch, 20) == 0x1u);
    CHECK(marks(true, 12, kmatch, 20) == 0xFFFu);             // (across two looks)
    CHECK(marks(false, 0, kmatch, 20) == 0u);                 // scaleEstimator none / no filter: never
    CHECK(marks(false, 3, kmatch, 20) == 0u);
  }
  std::printf(fails ? "robust_policy_check: %d failure(s)\n" : "robust_policy_check: ok\n", fails);
  return fails ? 1 : 0;
}
