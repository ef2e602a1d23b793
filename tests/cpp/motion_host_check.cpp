// motion_host_check.cpp -- the host-only entries of the force2D / force4DOF steps and BoundTransformationChecker, as a
// stand-alone program: lsgpu_chain_load_motion over a few documents, lsgpu_motion_config_check, lsgpu_point_to_plane_solve_dof
// and lsgpu_bound_first_violation.  Links against csrc/lsgpu_chain_loader.cpp and csrc/lsgpu_host_filters.cpp alone (no HIP,
// no device), so it can be built with -fsanitize=address,undefined and run as it is.  Prints "motion_host_check: ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lsgpu_icp.h"

#ifdef MOTION_HOST_STANDALONE
// The two *_config_default functions the loader calls that live in the library's HIP translation unit: zero-filling stand-ins
// (the loader overwrites what it reads back, and nothing checked here depends on them).  Without the macro the program links
// against the library itself.
extern "C" {
void lsgpu_icp_config_default(lsgpu_icp_config* c) { std::memset(c, 0, sizeof(*c)); c->max_iterations = 40; }
void lsgpu_chain_config_default(lsgpu_chain_config* c) { std::memset(c, 0, sizeof(*c)); c->seed = -1; }
}
#endif

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Mod { const char* section; const char* name; std::vector<lsgpu_yaml_param> params; };

static int load(const std::vector<Mod>& mods, lsgpu_motion_config* out, char* why, int cap) {
  std::vector<lsgpu_yaml_module> arr;
  for (const Mod& m : mods) {
    lsgpu_yaml_module y;
    std::memset(&y, 0, sizeof(y));
    y.section = m.section; y.name = m.name; y.params = m.params.empty() ? nullptr : m.params.data(); y.n_params = (int)m.params.size();
    arr.push_back(y);
  }
  return lsgpu_chain_load_motion(arr.data(), (int)arr.size(), out, why, cap);
}

static std::vector<Mod> chain(std::vector<lsgpu_yaml_param> minimizer, bool bound_first, bool bound, const char* minimizer_name = "PointToPlaneErrorMinimizer") {
  std::vector<Mod> m = {{"referenceDataPointsFilters", "SamplingSurfaceNormalDataPointsFilter", {{"knn", "10"}}},
                        {"matcher", "KDTreeMatcher", {{"knn", "1"}}},
                        {"outlierFilters", "TrimmedDistOutlierFilter", {{"ratio", "0.75"}}},
                        {"errorMinimizer", minimizer_name, minimizer}};
  const Mod b = {"transformationCheckers", "BoundTransformationChecker", {{"maxRotationNorm", "0.5"}, {"maxTranslationNorm", "2"}}};
  if (bound && bound_first) m.push_back(b);
  m.push_back({"transformationCheckers", "CounterTransformationChecker", {{"maxIterationCount", "40"}}});
  if (bound && !bound_first) m.push_back(b);
  return m;
}

int main() {
  char why[256];
  lsgpu_motion_config c;
  // ---- the loader
  CHECK(load(chain({}, false, false), &c, why, sizeof(why)) == LSGPU_OK && c.dof == LSGPU_MOTION_DOF_6 && c.bound == 0);
  CHECK(load(chain({{"force2D", "1"}}, false, false), &c, why, sizeof(why)) == LSGPU_OK && c.dof == LSGPU_MOTION_DOF_3);
  CHECK(load(chain({{"force4DOF", "1"}, {"force2D", "0"}}, true, true), &c, why, sizeof(why)) == LSGPU_OK && c.dof == LSGPU_MOTION_DOF_4 &&
        c.bound == 1 && c.bound_before_counter == 1 && c.max_rotation_norm == 0.5f && c.max_translation_norm == 2.f);
  CHECK(load(chain({}, false, true), &c, why, sizeof(why)) == LSGPU_OK && c.bound == 1 && c.bound_before_counter == 0);
  CHECK(load(chain({{"force2D", "1"}, {"force4DOF", "1"}}, false, false), &c, why, sizeof(why)) == LSGPU_BAD_CONFIG && std::strstr(why, "PointToPlaneErrorMinimizer"));
  CHECK(load(chain({{"force2D", "2"}}, false, false), &c, why, sizeof(why)) == LSGPU_BAD_CONFIG && std::strstr(why, "force2D"));
  CHECK(load(chain({{"force4DOF", "1"}}, false, false, "PointToPointErrorMinimizer"), &c, why, sizeof(why)) == LSGPU_BAD_CONFIG && std::strstr(why, "PointToPointErrorMinimizer"));
  CHECK(load(chain({}, false, false), &c, why, 1) == LSGPU_OK);           // a one-byte reason buffer
  CHECK(load(chain({{"force2D", "x"}}, false, false), &c, why, 4) == LSGPU_BAD_CONFIG && std::strlen(why) == 3);
  CHECK(lsgpu_chain_load_motion(nullptr, 0, nullptr, why, sizeof(why)) == LSGPU_BAD_ARG);
  // ---- the config check
  lsgpu_motion_config_default(&c);
  CHECK(lsgpu_motion_config_check(&c) == LSGPU_OK && c.max_rotation_norm == 1.f && c.max_translation_norm == 1.f);
  c.dof = 5;
  CHECK(lsgpu_motion_config_check(&c) == LSGPU_BAD_CONFIG && std::strstr(lsgpu_motion_config_why(&c), "PointToPlaneErrorMinimizer"));
  c.dof = LSGPU_MOTION_DOF_3; c.bound = 1; c.max_translation_norm = NAN;
  CHECK(lsgpu_motion_config_check(&c) == LSGPU_BAD_CONFIG && std::strstr(lsgpu_motion_config_why(&c), "BoundTransformationChecker"));
  CHECK(lsgpu_motion_config_check(nullptr) == LSGPU_BAD_CONFIG);
  // ---- the solve: A = diag(1..6) + 0.1 (positive definite), b = 0.01 (1..6)
  double sums[27];
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int cc = a; cc < 6; ++cc) sums[k++] = (a == cc ? 1.0 + a : 0.0) + 0.1;
  for (int a = 0; a < 6; ++a) sums[21 + a] = 0.01 * (a + 1);
  float d0[16], d6[16], d4[16], d3[16];
  CHECK(lsgpu_point_to_plane_solve(sums, d0) == LSGPU_OK && lsgpu_point_to_plane_solve_dof(sums, LSGPU_MOTION_DOF_6, d6) == LSGPU_OK &&
        std::memcmp(d0, d6, sizeof(d0)) == 0);
  CHECK(lsgpu_point_to_plane_solve_dof(sums, LSGPU_MOTION_DOF_4, d4) == LSGPU_OK && lsgpu_point_to_plane_solve_dof(sums, LSGPU_MOTION_DOF_3, d3) == LSGPU_OK);
  for (const float* d : {d4, d3}) CHECK(d[2] == 0.f && d[6] == 0.f && d[8] == 0.f && d[9] == 0.f && d[10] == 1.f && d[15] == 1.f);
  CHECK(d3[14] == 0.f && d4[14] != 0.f && d4[1] > 0.f && d4[4] == -d4[1] && d4[0] == d4[5]);
  sums[11] = -1.0;   // A[2][2] < 0: the constrained sub-systems start at that pivot
  CHECK(lsgpu_point_to_plane_solve_dof(sums, LSGPU_MOTION_DOF_4, d4) == LSGPU_NO_CONVERGENCE && d4[0] == 1.f && d4[12] == 0.f);
  CHECK(lsgpu_point_to_plane_solve_dof(sums, 7, d4) == LSGPU_BAD_ARG && lsgpu_point_to_plane_solve_dof(nullptr, 3, d4) == LSGPU_BAD_ARG);
  // ---- the bound: identity, a small step, a step out of bounds, back inside
  float T[4][16];
  for (auto& t : T) { std::memset(t, 0, sizeof(t)); t[0] = t[5] = t[10] = t[15] = 1.f; }
  T[1][12] = 0.05f; T[2][12] = 0.5f; T[3][12] = 0.01f;
  CHECK(lsgpu_bound_first_violation(&T[0][0], 4, 1.f, 0.1f) == 2 && lsgpu_bound_first_violation(&T[0][0], 4, 1.f, 0.5f) == -1);
  CHECK(lsgpu_bound_first_violation(&T[0][0], 1, 0.f, 0.f) == -1 && lsgpu_bound_first_violation(nullptr, 4, 1.f, 1.f) == -1);
  std::printf(fails ? "motion_host_check: %d FAILED\n" : "motion_host_check: ok\n", fails);
  return fails ? 1 : 0;
}
