// section_plan_check.cpp -- CPU driver of the section plan (laser_slam_amd/csrc/lsgpu_section_plan.h): one JSON record per
// input of the whole input space, the refused combinations included, in the terms and the order of
// tests/golden/section_plan_parent.json (the routing of lsgpu_icp_compute before the plan existed).  The test compares the
// two entry by entry.
#include <cstdio>
#include <string>

#include "../../laser_slam_amd/csrc/lsgpu_section_plan.h"

using namespace lsgpu::section;

static const char* tf(bool b) { return b ? "true" : "false"; }

static std::string record(const Inputs& in, bool reaches) {
  char key[16];
  std::snprintf(key, sizeof key, "%d%d%d%d%d%d%d%d%d%d%d", (int)in.module, in.normals_read, in.max_density, in.ref_shadow, in.ref_cov_sampling,
                reaches, in.rd_normals, in.rd_shadow, in.rd_cov_sampling, in.comm, in.side_switch);
  std::string out = std::string("{\"in\": \"") + key + "\", ";
  Plan p = plan(in);
  if (p.refusal) return out + "\"verdict\": \"" + p.refusal + "\"}";
  p = settle(p, 100, reaches ? 100 : 4096);   // (nbSample 100 against the section's count)
  static const char* const sources[] = {"none", "sampling", "final_grid", "whole_cloud", "whole_cloud_densities"};
  static const char* const stages[] = {"max_density", "shadow", "cov_sampling"};
  static const char* const shadow[] = {"null", "\"array\"", "\"gathered\""};
  out += std::string("\"verdict\": \"ok\", \"source\": \"") + sources[(int)p.source] + "\", \"grids_before_final\": " +
         std::to_string((int)p.whole_cloud() + (int)p.rd_normals) + ", \"densities\": " + tf(p.source == Source::WholeCloudDensities) + ", \"stages\": [";
  for (int i = 0; i < p.n_stages; ++i) out += std::string(i ? ", \"" : "\"") + stages[(int)p.stages[i]] + "\"";
  out += std::string("], \"shadow_normals\": ") + shadow[(int)p.shadow_normals] + ", \"emits\": [";
  for (int i = 0; i < p.n_stages; ++i) out += std::string(i ? ", " : "") + tf(p.emits[i]);
  out += "], \"reading_stages\": [";
  if (p.rd_shadow) out += "\"shadow\"";
  if (p.rd_cov_sampling) out += p.rd_shadow ? ", \"cov_sampling\"" : "\"cov_sampling\"";
  out += std::string("], \"normals_to_build\": ") + tf(p.normals_to_build()) + ", \"normals_on_final_grid\": " + tf(p.normals_on_final_grid) +
         ", \"side\": " + tf(p.side) + "}";
  return out;
}

int main() {
  int n = 0;
  for (int m = 0; m < 3; ++m) for (int read = 0; read < 2; ++read) for (int md = 0; md < 2; ++md) for (int sh = 0; sh < 2; ++sh)
  for (int cs = 0; cs < 2; ++cs) for (int reaches = 0; reaches < 2; ++reaches) for (int rd = 0; rd < 8; ++rd)
  for (int comm = 0; comm < 2; ++comm) for (int sw = 0; sw < 2; ++sw, ++n) {
    Inputs in;
    in.module = (Module)m; in.normals_read = read; in.max_density = md; in.ref_shadow = sh; in.ref_cov_sampling = cs;
    in.rd_normals = rd & 1; in.rd_shadow = rd & 2; in.rd_cov_sampling = rd & 4; in.comm = comm; in.side_switch = sw;
    std::printf("%s\n", record(in, reaches).c_str());
  }
  std::printf("section_plan_check: ok %d\n", n);
  return 0;
}
