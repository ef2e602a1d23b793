// normal_outlier_policy_check.cpp -- CPU driver of the launch policy (laser_slam_amd/csrc/lsgpu_policy.h) for handles with
// SurfaceNormalOutlierFilter: such a handle takes the chain plan whatever the other fields hold, and the plan is that of any
// chain (k-best search on the voxel grid, a full select, no repeat, no MAD marks).  A configuration without it is planned as before.
#include <cmath>
#include <cstdio>
#include <initializer_list>

#include "../../laser_slam_amd/csrc/lsgpu_policy.h"

using namespace lsgpu::policy;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
  CHECK(!chain_fields(0.f, 0.f, 0.f, 0.f) && !chain_fields(0.f, 0.f, 0.f, 0.f, false, false));
  CHECK(chain_fields(0.f, 0.f, 0.f, 0.f, false, true) && chain_fields(INFINITY, INFINITY, 0.f, 0.f, false, true) &&
        chain_fields(0.f, 0.f, 0.f, 0.f, true, true) && chain_fields(0.5f, 0.f, 0.f, 0.f, false, true));
  for (bool kmatch : {false, true}) {
    Config c; c.enq_limit = 400; c.chain = true; c.kmatch = kmatch;
    State s; s.begin_align(true, true, false, 2.f);
    Iteration it = s.plan(c, true, true, true, true, false);
    CHECK(it.seed && it.knn && !it.capped && !it.predicted && !it.committed && it.full_select && !it.cone_iter && !it.mad && it.ordinal == 0);
    s.enq = 1; s.since_check = 1;
    int n = 1;
    while (n < 20) {
      while (n < 20 && s.next_in_group(c, &it)) {
        CHECK(!it.seed && it.knn && !it.capped && !it.predicted && !it.committed && it.full_select && !it.cone_iter && !it.mad && it.ordinal == n);
        CHECK(s.kernel(c, it, true) == KnnKernel::Tile);
        ++n;
      }
      Iteration ahead; int q = 0;
      if (n < 20 && s.lookahead_iteration(c, &ahead)) { CHECK(ahead.ordinal == n && !ahead.mad); ++n; q = 1; }
      LookInput li; li.iter = n - q; li.nq = 1000;
      CHECK(s.on_look(c, li, q, -1.f) == LookVerdict::Continue);
    }
    CHECK(s.cap_retries == 0 && s.sel_retries == 0 && s.committed_iterations == 0 && s.cone_launches == 0);
  }
  std::printf(fails ? "normal_outlier_policy_check: %d failure(s)\n" : "normal_outlier_policy_check: ok\n", fails);
  return fails ? 1 : 0;
}
