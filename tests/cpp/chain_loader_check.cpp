// chain_loader_check.cpp -- CPU-only check of ICP::loadFromYaml (laser_slam_amd/cpp/include/laser_slam_amd/icp.hpp) with
// KDTreeMatcher maxDist and the outlier-filter chain: each of Trimmed- / Max- / Min- / MedianDistOutlierFilter alone, all
// four in two orders (same config), module defaults, maxDist: inf = absent; duplicates, unknown parameters and values out
// of range are configuration errors that name the module.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>

#include "laser_slam_amd/icp.hpp"

using namespace laser_slam_amd;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const std::string kHead = "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n";
static const std::string kTail = "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
                                 "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n";
static const std::string kMatcher = "matcher:\n  KDTreeMatcher:\n    knn: 1\n";

static std::string doc(const std::string& matcher, const std::string& outliers) {
  return kHead + matcher + (outliers.empty() ? "" : "outlierFilters:\n" + outliers) + kTail;
}
// "" = loaded, otherwise the error text
static std::string load(ICP& icp, const std::string& y) {
  std::istringstream in(y);
  try { icp.loadFromYaml(in); } catch (const ConfigError& e) { return std::string("E:") + e.what(); }
  return "";
}
static bool refused(ICP& icp, const std::string& y, const char* module) {
  const std::string e = load(icp, y);
  return !e.empty() && e.find(module) != std::string::npos;
}

int main() {
  ICP icp;
  const lsgpu_icp_config& c = icp.config();
  CHECK(c.matcher_max_dist == 0.f && c.outlier_max_dist == 0.f && c.outlier_min_dist == 0.f && c.outlier_median_factor == 0.f);
  const std::string trim = "  - TrimmedDistOutlierFilter:\n      ratio: 0.8\n", maxd = "  - MaxDistOutlierFilter:\n      maxDist: 0.4\n",
                    mind = "  - MinDistOutlierFilter:\n      minDist: 0.02\n", med = "  - MedianDistOutlierFilter:\n      factor: 2.5\n";
  CHECK(load(icp, doc(kMatcher, trim)).empty());
  CHECK(icp.config().trim_ratio == 0.8f && icp.config().outlier_max_dist == 0.f && icp.config().outlier_min_dist == 0.f && icp.config().outlier_median_factor == 0.f);
  CHECK(load(icp, doc(kMatcher, maxd)).empty());
  CHECK(icp.config().trim_ratio == 1.0f && icp.config().outlier_max_dist == 0.4f);
  CHECK(load(icp, doc(kMatcher, mind)).empty());
  CHECK(icp.config().trim_ratio == 1.0f && icp.config().outlier_min_dist == 0.02f && icp.config().outlier_max_dist == 0.f);
  CHECK(load(icp, doc(kMatcher, med)).empty());
  CHECK(icp.config().outlier_median_factor == 2.5f && icp.config().outlier_min_dist == 0.f);
  // all four, two orders: the same config
  CHECK(load(icp, doc(kMatcher, trim + maxd + mind + med)).empty());
  const lsgpu_icp_config a = icp.config();
  CHECK(load(icp, doc(kMatcher, med + mind + trim + maxd)).empty());
  const lsgpu_icp_config b = icp.config();
  CHECK(std::memcmp(&a, &b, sizeof(a)) == 0);
  CHECK(a.trim_ratio == 0.8f && a.outlier_max_dist == 0.4f && a.outlier_min_dist == 0.02f && a.outlier_median_factor == 2.5f);
  // module defaults
  CHECK(load(icp, doc(kMatcher, "  - TrimmedDistOutlierFilter\n  - MaxDistOutlierFilter\n  - MinDistOutlierFilter\n  - MedianDistOutlierFilter\n")).empty());
  CHECK(icp.config().trim_ratio == 0.85f && icp.config().outlier_max_dist == 1.f && icp.config().outlier_min_dist == 1.f && icp.config().outlier_median_factor == 3.f);
  // the matcher's maxDist
  CHECK(load(icp, doc(kMatcher + "    maxDist: 0.5\n", trim)).empty());
  CHECK(icp.config().matcher_max_dist == 0.5f);
  CHECK(load(icp, doc(kMatcher + "    maxDist: inf\n", trim)).empty());
  CHECK(icp.config().matcher_max_dist == 0.f);
  CHECK(load(icp, doc(kMatcher, "")).empty());
  CHECK(icp.config().matcher_max_dist == 0.f && icp.config().trim_ratio == 1.0f);
  // YAML floats with a leading dot are plain floats; .inf / .Inf / .INF are infinity (absent for the two maxDist)
  CHECK(load(icp, doc(kMatcher + "    maxDist: .5\n", "  - TrimmedDistOutlierFilter:\n      ratio: .85\n  - MinDistOutlierFilter:\n      minDist: .05\n"
                                                       "  - MedianDistOutlierFilter:\n      factor: .5\n  - MaxDistOutlierFilter:\n      maxDist: .25\n")).empty());
  CHECK(icp.config().matcher_max_dist == 0.5f && icp.config().trim_ratio == 0.85f && icp.config().outlier_min_dist == 0.05f &&
        icp.config().outlier_median_factor == 0.5f && icp.config().outlier_max_dist == 0.25f);
  for (const char* inf : {".inf", ".Inf", ".INF", "+.inf", "inf"}) {
    CHECK(load(icp, doc(kMatcher + "    maxDist: " + inf + "\n", std::string("  - MaxDistOutlierFilter:\n      maxDist: ") + inf + "\n")).empty());
    CHECK(icp.config().matcher_max_dist == 0.f && icp.config().outlier_max_dist == 0.f);
  }
  CHECK(refused(icp, doc(kMatcher + "    maxDist: -.inf\n", trim), "KDTreeMatcher"));
  CHECK(refused(icp, doc(kMatcher, "  - MaxDistOutlierFilter:\n      maxDist: -.inf\n"), "MaxDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MinDistOutlierFilter:\n      minDist: .inf\n"), "MinDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MedianDistOutlierFilter:\n      factor: .inf\n"), "MedianDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MaxDistOutlierFilter:\n      maxDist: .x5\n"), "MaxDistOutlierFilter"));
  // configuration errors, with the module's name
  CHECK(refused(icp, doc(kMatcher, maxd + maxd), "MaxDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, mind + trim + mind), "MinDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, med + med), "MedianDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, trim + trim), "TrimmedDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MaxDistOutlierFilter:\n      maxDist: 0.4\n      ratio: 0.5\n"), "MaxDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MedianDistOutlierFilter:\n      ratio: 0.5\n"), "MedianDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MinDistOutlierFilter:\n      maxDist: 0.5\n"), "MinDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MaxDistOutlierFilter:\n      maxDist: 0\n"), "MaxDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MedianDistOutlierFilter:\n      factor: -1\n"), "MedianDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher, "  - MinDistOutlierFilter:\n      minDist: -1\n"), "MinDistOutlierFilter"));
  CHECK(refused(icp, doc(kMatcher + "    maxDist: 0\n", trim), "KDTreeMatcher"));
  CHECK(refused(icp, doc(kMatcher + "    maxDist: -2\n", trim), "KDTreeMatcher"));
  // a document with nothing but an outlier filter is refused for the modules it lacks
  CHECK(!load(icp, "outlierFilters:\n  - MaxDistOutlierFilter\n").empty());
  icp.setDefault();
  CHECK(icp.config().matcher_max_dist == 0.f && icp.config().outlier_median_factor == 0.f && icp.config().trim_ratio == 0.85f);
  // lsgpu_icp_create refuses negative / NaN thresholds before it touches a device
  for (int f = 0; f < 4; ++f)
    for (float v : {-1.f, NAN, INFINITY}) {
      lsgpu_icp_config k;
      lsgpu_icp_config_yaml(&k);
      CHECK(k.matcher_max_dist == 0.f && k.outlier_max_dist == 0.f && k.outlier_min_dist == 0.f && k.outlier_median_factor == 0.f);
      float* fld[4] = {&k.matcher_max_dist, &k.outlier_max_dist, &k.outlier_min_dist, &k.outlier_median_factor};
      *fld[f] = v;
      lsgpu_icp* h = nullptr;
      const int rc = lsgpu_icp_create(&k, 0, &h);
      if (std::isinf(v) && f < 2) { CHECK(rc != LSGPU_BAD_CONFIG); if (h) lsgpu_icp_destroy(h); }   // +inf maxDist = absent
      else CHECK(rc == LSGPU_BAD_CONFIG && h == nullptr);
    }
  if (fails) return 1;
  std::printf("chain_loader_check: ok\n");
  return 0;
}
