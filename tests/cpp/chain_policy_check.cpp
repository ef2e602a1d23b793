// chain_policy_check.cpp -- CPU driver of the launch policy (laser_slam_amd/csrc/lsgpu_policy.h) for chains with
// KDTreeMatcher maxDist / Max-, Min-, MedianDistOutlierFilter: which configurations take the chain plan, what that plan
// enqueues, and that a configuration with none of the new fields is planned exactly as before.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../laser_slam_amd/csrc/lsgpu_policy.h"

using namespace lsgpu::policy;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static bool same(const Iteration& a, const Iteration& b) {
  return a.knn == b.knn && a.seed == b.seed && a.capped == b.capped && a.wide == b.wide && a.predicted == b.predicted &&
         a.committed == b.committed && a.full_select == b.full_select && a.cone_iter == b.cone_iter &&
         a.dense_wait == b.dense_wait && a.price == b.price && a.ordinal == b.ordinal;
}

int main() {
  // which fields switch the plan: 0 and (for the two maxDist) +inf mean absent
  CHECK(!chain_fields(0.f, 0.f, 0.f, 0.f));
  CHECK(!chain_fields(INFINITY, INFINITY, 0.f, 0.f));
  CHECK(chain_fields(0.5f, 0.f, 0.f, 0.f) && chain_fields(0.f, 0.5f, 0.f, 0.f) && chain_fields(0.f, 0.f, 0.01f, 0.f) &&
        chain_fields(0.f, 0.f, 0.f, 3.f) && chain_fields(INFINITY, 0.f, 0.f, 2.f));
  // the chain plan, for one neighbour and for k matches: a k-best search every iteration (seeded first), no cap, no
  // predicted / committed / fused select, no direction index, no pricing -- through a whole alignment with looks
  for (bool kmatch : {false, true}) {
    Config c; c.enq_limit = 400; c.chain = true; c.kmatch = kmatch; c.two_pass_select = true;
    State s; s.begin_align(true, true, false, 2.f);
    Iteration it = s.plan(c, true, true, true, true, false);
    CHECK(it.seed && it.knn && !it.capped && !it.wide && !it.predicted && !it.committed && it.full_select && !it.cone_iter && !it.price);
    s.enq = 1; s.since_check = 1;
    int n = 1;
    for (int look = 0; look < 5; ++look) {
      while (s.next_in_group(c, &it)) {
        CHECK(!it.seed && it.knn && !it.capped && !it.predicted && !it.committed && it.full_select && !it.cone_iter && !it.price && it.ordinal == n);
        CHECK(s.kernel(c, it, true) == KnnKernel::Tile && !s.pricing(c, it, true) && !s.wants_occupancy(it, true));
        ++n;
      }
      Iteration ahead; int q = 0;
      if (s.lookahead_iteration(c, &ahead)) { CHECK(!ahead.capped && !ahead.committed && ahead.full_select); ++n; q = 1; }
      LookInput li; li.iter = n - q; li.sel_streak = 5; li.nq = 1000;
      CHECK(s.on_look(c, li, q, -1.f) == LookVerdict::Continue);   // (a confirmed streak commits nothing on this plan)
    }
    CHECK(s.committed_iterations == 0 && s.cone_launches == 0 && s.cap_retries == 0 && s.sel_retries == 0);
    LookInput done; done.done = 1; done.iter = n;
    CHECK(s.on_look(c, done, 0, -1.f) == LookVerdict::Done);
  }
  // a configuration with none of the new fields: chain = false is the default, and the plans of the one-neighbour loop
  // and of the k-match loop are what they are with the field absent
  for (bool kmatch : {false, true}) {
    Config a, b; a.enq_limit = b.enq_limit = 400; a.kmatch = b.kmatch = kmatch;
    b.chain = chain_fields(0.f, INFINITY, 0.f, 0.f);
    CHECK(!b.chain);
    State sa, sb; sa.begin_align(true, true, false, 2.f); sb.begin_align(true, true, false, 2.f);
    CHECK(same(sa.plan(a, true, true, true, true, false), sb.plan(b, true, true, true, true, false)));
    sa.enq = sb.enq = 1; sa.since_check = sb.since_check = 1;
    for (int look = 0; look < 4; ++look) {
      Iteration ia, ib;
      for (;;) {
        const bool ra = sa.next_in_group(a, &ia), rb = sb.next_in_group(b, &ib);
        CHECK(ra == rb);
        if (!ra || !rb) break;
        CHECK(same(ia, ib));
      }
      LookInput li; li.iter = sa.enq; li.sel_streak = 3; li.nq = 1000;
      CHECK(sa.on_look(a, li, 0, -1.f) == sb.on_look(b, li, 0, -1.f));
    }
    if (!kmatch) CHECK(sa.committed_iterations > 0 && sa.committed_iterations == sb.committed_iterations);
  }
  if (fails) return 1;
  std::printf("chain_policy_check: ok\n");
  return 0;
}
