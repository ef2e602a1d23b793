// carried_check.cpp -- CPU-only checks of carried normals (include/lsgpu_icp.h, "carried normals") above the library:
// the section plan's Carried source, the input filter chain's normals tail (DataPointsFilters), ICP::loadFromYaml under a
// declaration, and the shim with the mirror types handing a cloud's normals over.  No device is touched: nothing here
// applies a filter or computes.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "laser_slam_amd/icp.hpp"
#include "../../integration/lsgpu_icp_shim.hpp"
#include "../../laser_slam_amd/csrc/lsgpu_section_plan.h"

using namespace laser_slam_amd;
namespace sec = lsgpu::section;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static const std::string kSN = "- SurfaceNormalDataPointsFilter:\n    knn: 10\n";
static const std::string kPair = "- ObservationDirectionDataPointsFilter:\n    x: 0.5\n    z: -1\n- OrientNormalsDataPointsFilter:\n    towardCenter: 0\n";
static const std::string kRS = "- RandomSamplingDataPointsFilter:\n    prob: 0.5\n";
static const std::string kMax = "- MaxDistDataPointsFilter:\n    maxDist: 80\n";

// "" = parsed, otherwise the error text
static std::string parse(const std::string& y, DataPointsFilters* out = nullptr) {
  std::istringstream in(y);
  try { DataPointsFilters f(in, 0, /*normals_tail*/ true); if (out) *out = std::move(f); } catch (const ConfigError& e) { return std::string("E:") + e.what(); }
  return "";
}
static bool refused(const std::string& y, const char* word) {
  const std::string e = parse(y);
  if (e.empty() || e.find(word) == std::string::npos) std::printf("  got: '%s'\n", e.c_str());
  return !e.empty() && e.find(word) != std::string::npos;
}

static const std::string kIcpFile =
    "readingDataPointsFilters:\n  - RandomSamplingDataPointsFilter:\n      prob: 0.5\n"
    "matcher:\n  KDTreeMatcher:\n    knn: 1\n"
    "outlierFilters:\n  - TrimmedDistOutlierFilter:\n      ratio: 0.75\n  - SurfaceNormalOutlierFilter:\n      maxAngle: 0.5\n"
    "errorMinimizer:\n  PointToPlaneErrorMinimizer\n"
    "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 40\n";

static std::string load(ICP& icp, const std::string& y, unsigned carried) {
  std::istringstream in(y);
  try { icp.loadFromYaml(in, carried); } catch (const ConfigError& e) { return std::string("E:") + e.what(); }
  return "";
}

int main() {
  // ---- the section plan
  {
    sec::Inputs in;
    in.normals_read = true; in.ref_carried = true;
    sec::Plan p = sec::plan(in);
    CHECK(!p.refusal && p.source == sec::Source::Carried && p.n_stages == 0 && p.normals_to_build() && !p.normals_on_final_grid);
    CHECK(!p.draws_per_reference_point() && !p.whole_cloud() && p.side);
    const sec::Plan q = sec::settle(p, 100, 50);
    CHECK(q.source == sec::Source::Carried && q.normals_to_build());
    in.normals_read = false;                                            // nobody reads them: they do not travel
    p = sec::plan(in);
    CHECK(p.source == sec::Source::None && !p.normals_to_build());
    in.normals_read = true;
    for (sec::Module m : {sec::Module::Sampling, sec::Module::SurfaceNormal}) {   // a module wins
      sec::Inputs a = in, b = in;
      a.module = b.module = m; b.ref_carried = false;
      const sec::Plan pa = sec::plan(a), pb = sec::plan(b);
      CHECK(pa.source == pb.source && pa.source != sec::Source::Carried && pa.normals_to_build() == pb.normals_to_build() && pa.side == pb.side);
    }
    in.rd_carried = true;                                               // the reading's, through its section
    p = sec::plan(in);
    CHECK(p.rd_carried && !p.rd_normals && p.side);
    in.rd_normals = true;                                               // ... unless its own module overwrites them
    p = sec::plan(in);
    CHECK(!p.rd_carried && p.rd_normals);
    in.rd_normals = false; in.rd_carried = false;
    // the thinning modules need a module's normals: the standing texts
    sec::Inputs t = in; t.ref_shadow = true;
    CHECK(sec::plan(t).refusal && std::strstr(sec::plan(t).refusal, "ShadowDataPointsFilter on the reference needs the normals of a reference filter"));
    t = in; t.ref_cov_sampling = true;
    CHECK(sec::plan(t).refusal && std::strstr(sec::plan(t).refusal, "CovarianceSamplingDataPointsFilter on the reference needs the normals of a reference filter"));
    t = in; t.max_density = true;
    CHECK(sec::plan(t).refusal && std::strstr(sec::plan(t).refusal, "MaxDensityDataPointsFilter: needs the densities"));
    t = in; t.rd_carried = true; t.rd_shadow = true;
    CHECK(sec::plan(t).refusal && std::strstr(sec::plan(t).refusal, "needs the reading's SurfaceNormalDataPointsFilter"));
  }
  // ---- the input chain's tail
  {
    DataPointsFilters f;
    CHECK(parse(kMax + kRS, &f).empty() && !f.producesNormals() && f.size() == 2 && !f.empty());
    CHECK(parse(kMax + kRS + kSN, &f).empty() && f.producesNormals() && f.normalsKnn() == 10 && f.normalsOrientation() == 0 && f.size() == 2);
    CHECK(parse(kRS + kSN + kPair, &f).empty() && f.producesNormals() && f.normalsOrientation() == 2 && f.size() == 1);
    CHECK(parse(kSN, &f).empty() && f.producesNormals() && f.size() == 0 && !f.empty());
    CHECK(parse("- SurfaceNormalDataPointsFilter\n", &f).empty() && f.normalsKnn() == 5);      // the module's default
    CHECK(parse("", &f).empty() && f.empty() && !f.producesNormals());
    // the loader's rule for the reading's module, by its texts
    CHECK(refused("- SurfaceNormalDataPointsFilter:\n    knn: 2\n", "knn must be an integer in [3, 32]"));
    CHECK(refused("- SurfaceNormalDataPointsFilter:\n    knn: 33\n", "knn must be an integer in [3, 32]"));
    CHECK(refused("- SurfaceNormalDataPointsFilter:\n    keepNormals: 0\n", "keepNormals must be 1"));
    CHECK(refused("- SurfaceNormalDataPointsFilter:\n    epsilon: 0.1\n", "epsilon must be 0"));
    CHECK(refused("- SurfaceNormalDataPointsFilter:\n    keepDensities: 1\n", "keepDensities 1"));
    CHECK(refused("- SurfaceNormalDataPointsFilter:\n    ratio: 1\n", "unknown parameter ratio"));
    // a point module behind the tail, the pair's halves, Shadow
    CHECK(refused(kSN + kRS, "RandomSamplingDataPointsFilter behind SurfaceNormalDataPointsFilter"));
    CHECK(refused(kSN + kPair + kMax, "MaxDistDataPointsFilter behind SurfaceNormalDataPointsFilter"));
    CHECK(refused(kSN + kSN, "given twice"));
    CHECK(refused(kPair + kSN, "ObservationDirectionDataPointsFilter"));
    CHECK(refused(kSN + "- ObservationDirectionDataPointsFilter\n", "only as the pair"));
    CHECK(refused(kSN + "- OrientNormalsDataPointsFilter\n", "only as the pair"));
    CHECK(refused(kSN + kPair + "- OrientNormalsDataPointsFilter\n", "only as the pair"));
    CHECK(refused(kSN + "- ObservationDirectionDataPointsFilter\n- OrientNormalsDataPointsFilter:\n    towardCenter: 2\n", "towardCenter must be 0 or 1"));
    CHECK(refused(kSN + "- ShadowDataPointsFilter\n", "ShadowDataPointsFilter"));
    CHECK(refused("- ShadowDataPointsFilter\n", "is not implemented on the HIP path"));
    // a caller that did not ask for the tail keeps the refusal of the module
    std::istringstream plain(kRS + kSN);
    bool threw = false;
    try { DataPointsFilters f(plain); } catch (const ConfigError& e) { threw = std::strstr(e.what(), "SurfaceNormalDataPointsFilter is not implemented on the HIP path") != nullptr; }
    CHECK(threw);
  }
  // ---- ICP::loadFromYaml under a declaration
  {
    ICP icp;
    CHECK(load(icp, kIcpFile, 0).find("SamplingSurfaceNormalDataPointsFilter or SurfaceNormalDataPointsFilter is required") != std::string::npos);
    CHECK(load(icp, kIcpFile, LSGPU_CARRIED_READING).find("is required") != std::string::npos);
    CHECK(load(icp, kIcpFile, LSGPU_CARRIED_REFERENCE).find("the reading section provides no normals") != std::string::npos);
    CHECK(icp.carried() == 0);
    CHECK(load(icp, kIcpFile, LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE).empty());
    CHECK(icp.carried() == 3 && icp.normalsConfig() && icp.normalsConfig()->reading_normals_given == 1 && icp.normalsConfig()->max_angle == 0.5f);
    CHECK(icp.surfaceNormalKnn() == 0 && icp.referenceNormalKnn() == 0 && icp.readsReferenceNormals());
    icp.setDefault();
    CHECK(icp.carried() == 0);
  }
  // ---- the shim hands a mirror cloud's normals over
  {
    DataPoints d;
    d.features = {1, 2, 3, 1, 4, 5, 6, 1};
    std::vector<float> n;
    CHECK(!LsgpuCloudTraits<LsgpuMirrorPM>::normals(d, &n) && n.empty());
    d.normals = {0, 0, 1, 0, 1, 0};
    CHECK(LsgpuCloudTraits<LsgpuMirrorPM>::normals(d, &n) && n == d.normals);
    LsgpuICP<LsgpuMirrorPM> shim;
    std::istringstream in(kIcpFile);
    bool threw = false;
    try { shim.loadFromYaml(in); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    std::istringstream in3(kIcpFile);
    shim.loadFromYaml(in3, LSGPU_CARRIED_READING | LSGPU_CARRIED_REFERENCE);
    std::istringstream tail(kRS + kSN);
    threw = false;
    try { LsgpuDataPointsFilters<LsgpuMirrorPM> f(tail); } catch (const std::runtime_error& e) { threw = std::strstr(e.what(), "SurfaceNormalDataPointsFilter") != nullptr; }
    CHECK(threw);
  }
  if (fails) { std::printf("carried_check: %d FAILED\n", fails); return 1; }
  std::printf("carried_check: ok\n");
  return 0;
}
