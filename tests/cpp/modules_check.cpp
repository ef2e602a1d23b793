// modules_check: the verdicts of csrc/lsgpu_modules.h (plain g++, no HIP, no library) on the cases of tests/module_cases.py, printed
// one call per line for tests/test_cpp_mirror.py to compare with what the library's setters and lsgpu_icp_comm_init answered
// before the header existed (tests/golden/module_rules_parent.json).  A setter is modelled as the library runs it: its "all off"
// normalisation, the one value check that depends on the case (normal_angle::check), the state as it would be, refusal(), commit.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../laser_slam_amd/csrc/lsgpu_modules.h"
#include "../../laser_slam_amd/csrc/lsgpu_normal_angle.h"

using namespace lsgpu::modules;

namespace {

const char* const kVariants[] = {"robust", "normals_angle", "normals_knn_only", "normals_angle_knn", "covariance", "cuts", "max_density",
                                 "shadow_reading", "shadow_reference", "cov_sampling_reading", "cov_sampling_reference", "force2d", "force4dof",
                                 "bound_only"};
constexpr int kNumVariants = (int)(sizeof(kVariants) / sizeof(kVariants[0]));
const char* const kConfigs[] = {"plane_knn1", "point", "knn2", "chain_threshold"};

Facts facts(int config, bool comm) {
  Facts f;
  if (config == 1) f.error_minimizer = LSGPU_MINIMIZER_POINT_TO_POINT;
  if (config == 2) f.matcher_knn = 2;
  f.chain = config == 3;
  f.comm = comm;
  return f;
}

lsgpu_normals_config normals(float max_angle, int knn, int given) {
  lsgpu_normals_config c;
  std::memset(&c, 0, sizeof(c));
  c.max_angle = max_angle; c.reading_sn_knn = knn; c.reading_normals_given = given;
  return c;
}

// the setter of variant `v` on `s`: the refusal, the state untouched; or nothing, the state changed
std::string set(State& s, const Facts& f, int v) {
  State next = s;
  Asker who = kSetRobust;
  std::string why;
  const std::string name = kVariants[v];
  if (name == "robust") { next.robust_on = true; }
  else if (name.rfind("normals", 0) == 0) {
    next.normals = name == "normals_angle" ? normals(0.5f, 0, 1) : name == "normals_knn_only" ? normals(-1.f, 5, 0) : normals(0.5f, 5, 0);
    next.normals_on = true;
    why = refusal(next, f, kSetNormalsFirst);
    const char* value = nullptr;
    if (why.empty() && lsgpu::normal_angle::check(&next.normals, f.error_minimizer, 1, &value) != LSGPU_OK) why = value;
    who = kSetNormals;
  }
  else if (name == "covariance") { next.cov_on = true; who = kSetCovariance; }
  else if (name == "cuts") { next.cuts_on = true; next.cuts.n_reading = 1; who = kSetCuts; }
  else if (name == "max_density") { next.md_on = true; who = kSetMaxDensity; }
  else if (name.rfind("shadow", 0) == 0) {
    next.sh_on = true; who = kSetShadow;
    next.sh_cfg.reading_eps = name == "shadow_reading" ? 0.1f : -1.f; next.sh_cfg.reference_eps = name == "shadow_reading" ? -1.f : 0.1f;
  }
  else if (name.rfind("cov_sampling", 0) == 0) {
    next.cs_on = true; who = kSetCovSampling;
    next.cs_cfg.reading_nb_sample = name == "cov_sampling_reading" ? 100 : 0; next.cs_cfg.reference_nb_sample = name == "cov_sampling_reading" ? 0 : 100;
  }
  else {
    next.mo_on = true; who = kSetMotion;
    next.mo_cfg.dof = name == "force2d" ? LSGPU_MOTION_DOF_3 : name == "force4dof" ? LSGPU_MOTION_DOF_4 : LSGPU_MOTION_DOF_6;
    next.mo_cfg.bound = name == "bound_only" ? 1 : 0;
  }
  if (why.empty()) why = refusal(next, f, who);
  if (why.empty()) s = next;
  return why;
}

std::string remove_normals(State& s, const Facts& f) {
  State next = s;
  next.normals_on = false;
  const std::string why = refusal(next, f, kSetNormalsFirst);
  if (why.empty()) s = next;
  return why;
}

}  // namespace

int main() {
  for (int c = 0; c < 4; ++c) {
    const Facts f = facts(c, false);
    for (int a = 0; a < kNumVariants; ++a)
      for (int b = 0; b < kNumVariants; ++b) {
        State s;
        const std::string first = set(s, f, a), second = set(s, f, b);
        std::printf("pairs\t%s\t%d\t%d\t%s\t%s\n", kConfigs[c], a, b, first.c_str(), second.c_str());
      }
    for (int a = 0; a < kNumVariants; ++a) {   // lsgpu_icp_comm_init behind one module ("-": the driver does not ask, see module_cases.drive)
      State s;
      const bool on = set(s, f, a).empty();
      std::printf("comm_init\t%s\t%d\t%s\n", kConfigs[c], a, on || c == 3 ? refusal(s, facts(c, true), kCommInit).c_str() : "-");
    }
    for (int m = 0; m < 2; ++m) {   // the removals that can be refused
      State s;
      const int module = m == 0 ? 7 : 9;
      const std::string r0 = set(s, f, 3), r1 = set(s, f, module), r2 = remove_normals(s, f), r3 = set(s, f, 1);
      std::printf("removals\t%s\t%s\t%s\t%s\t%s\t%s\n", kConfigs[c], kVariants[module], r0.c_str(), r1.c_str(), r2.c_str(), r3.c_str());
    }
    const Facts live = facts(c, true);   // every setter on an empty handle with a communicator
    for (int a = 0; a < kNumVariants; ++a) {
      State s;
      std::printf("with_comm\t%s\t%d\t%s\n", kConfigs[c], a, set(s, live, a).c_str());
    }
  }
  std::printf("modules_check: ok\n");
  return 0;
}
