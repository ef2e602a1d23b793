// p2p_loader_check.cpp -- CPU-only check of ICP::loadFromYaml (laser_slam_amd/cpp/include/laser_slam_amd/icp.hpp) with
// PointToPointErrorMinimizer: accepted with and without referenceDataPointsFilters (no module: ssn knn 0), while
// point-to-plane without the normal filter and any chain without a matcher or a counter stay configuration errors.
#include <cstdio>
#include <sstream>
#include <string>

#include "laser_slam_amd/icp.hpp"

using namespace laser_slam_amd;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const std::string kRef = "referenceDataPointsFilters:\n  - SamplingSurfaceNormalDataPointsFilter:\n      knn: 9\n";
static const std::string kMatcher = "matcher:\n  KDTreeMatcher:\n    knn: 1\n    epsilon: 0\n";
static const std::string kCounter = "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 30\n";
static const std::string kRest = "readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
                                 "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.8\n";

static bool loads(ICP& icp, const std::string& y) {
  std::istringstream in(y);
  try { icp.loadFromYaml(in); } catch (const ConfigError&) { return false; }
  return true;
}

int main() {
  ICP icp;
  const std::string p2p = "errorMinimizer:\n  PointToPointErrorMinimizer\n", p2pl = "errorMinimizer: PointToPlaneErrorMinimizer\n";
  CHECK(icp.config().error_minimizer == LSGPU_MINIMIZER_POINT_TO_PLANE);   // setDefault()
  CHECK(loads(icp, kRest + kRef + kMatcher + p2p + kCounter));
  CHECK(icp.config().error_minimizer == LSGPU_MINIMIZER_POINT_TO_POINT && icp.surfaceNormalKnn() == 9);
  CHECK(icp.config().max_iterations == 30 && icp.readingSamplingProb() == 0.5f);
  CHECK(loads(icp, kRest + kMatcher + p2p + kCounter));                   // no reference filter module
  CHECK(icp.config().error_minimizer == LSGPU_MINIMIZER_POINT_TO_POINT && icp.surfaceNormalKnn() == 0);
  CHECK(loads(icp, kRest + kRef + kMatcher + p2pl + kCounter));
  CHECK(icp.config().error_minimizer == LSGPU_MINIMIZER_POINT_TO_PLANE && icp.surfaceNormalKnn() == 9);
  CHECK(!loads(icp, kRest + kMatcher + p2pl + kCounter));                 // point-to-plane needs the normals
  CHECK(!loads(icp, kRest + kRef + p2p + kCounter));                      // no matcher
  CHECK(!loads(icp, kRest + kRef + kMatcher + p2p));                      // no counter
  CHECK(!loads(icp, kRest + kRef + kMatcher + kCounter));                 // no minimizer
  CHECK(!loads(icp, p2p));
  CHECK(!loads(icp, kRest + kMatcher + "errorMinimizer: PointToPointSimilarityErrorMinimizer\n" + kCounter));
  icp.setDefault();
  CHECK(icp.config().error_minimizer == LSGPU_MINIMIZER_POINT_TO_PLANE);
  if (fails) return 1;
  std::printf("p2p_loader_check: ok\n");
  return 0;
}
