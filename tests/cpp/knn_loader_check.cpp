// knn_loader_check.cpp -- CPU-only check of ICP::loadFromYaml (laser_slam_amd/cpp/include/laser_slam_amd/icp.hpp) with
// KDTreeMatcher knn = k: knn 1..LSGPU_MATCHER_KNN_MAX with epsilon 0 is accepted with either minimizer and lands in
// lsgpu_icp_config.matcher_knn; knn 0, a knn above the limit and epsilon > 0 stay configuration errors.
#include <cstdio>
#include <sstream>
#include <string>

#include "laser_slam_amd/icp.hpp"

using namespace laser_slam_amd;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const std::string kRef = "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 10\n";
static const std::string kCounter = "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n";
static const std::string kRest = "readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
                                 "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n";

static std::string matcher(const std::string& knn, const std::string& eps = "0") {
  return "matcher:\n  KDTreeMatcher:\n    knn: " + knn + "\n    epsilon: " + eps + "\n";
}

static bool loads(ICP& icp, const std::string& y) {
  std::istringstream in(y);
  try { icp.loadFromYaml(in); } catch (const ConfigError&) { return false; }
  return true;
}

int main() {
  ICP icp;
  CHECK(icp.config().matcher_knn == 0);   // setDefault(): one neighbour
  for (const char* mini : {"errorMinimizer:\n  PointToPlaneErrorMinimizer\n", "errorMinimizer:\n  PointToPointErrorMinimizer\n"}) {
    for (int k : {1, 2, 3, 8}) {
      CHECK(loads(icp, kRest + kRef + matcher(std::to_string(k)) + mini + kCounter));
      CHECK(icp.config().matcher_knn == k);
    }
    CHECK(!loads(icp, kRest + kRef + matcher("0") + mini + kCounter));
    CHECK(!loads(icp, kRest + kRef + matcher("9") + mini + kCounter));
    CHECK(!loads(icp, kRest + kRef + matcher("2.5") + mini + kCounter));
    CHECK(!loads(icp, kRest + kRef + matcher("3", "0.1") + mini + kCounter));
  }
  // a bare matcher is still refused: the minimizer, the counter and the normals are missing
  CHECK(!loads(icp, "matcher:\n  KDTreeMatcher: {knn: 3}\n"));
  icp.setDefault();
  CHECK(icp.config().matcher_knn == 0);
  if (fails) return 1;
  std::printf("knn_loader_check: ok\n");
  return 0;
}
