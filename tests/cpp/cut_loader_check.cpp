// cut_loader_check.cpp -- the cut modules (MaxDist-, MinDist-, BoundingBox-, RemoveNaNDataPointsFilter) of an ICP chain document
// through the C++ facade, and lsgpu_chain_load / lsgpu_chain_load_cuts on their own.  Two builds of this one file:
//
//   default (tests/test_chain_cuts.py links it against liblsgpu_icp.so): argv[1] holds documents, each as a line "DOC <bytes>"
//     followed by that many bytes of YAML.  Per document ICP::loadFromYaml, then one line: "OK <hex of lsgpu_loaded_chain> <hex of
//     lsgpu_chain_cuts, or - without cut modules>" or "ERR <the ConfigError's text>".  The test compares the lines with what
//     the Python facade gives for the same documents: the same verdict, the same text, the same bytes.
//
//   -DCUT_LOADER_STANDALONE (links against csrc/lsgpu_chain_loader.cpp ALONE, which is host-only, e.g. both compiled with
//     -fsanitize=address,undefined): no facade, no argument.  Module lists built here go through both entry points -- accepted
//     chains, every refusal of the cut modules' rules, truncated reason buffers -- and the results are checked.  The four
//     *_config_default functions the loader calls live in the library's other translation units; this build defines zero-filling
//     stand-ins (the loader overwrites what it reads back, and what is checked here does not depend on them).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#ifndef CUT_LOADER_STANDALONE

#include <fstream>
#include <sstream>

#include "laser_slam_amd/icp.hpp"

using namespace laser_slam_amd;

static void hex(const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) std::printf("%02x", b[i]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  std::string head;
  int n_docs = 0;
  while (std::getline(in, head)) {
    size_t bytes = 0;
    if (std::sscanf(head.c_str(), "DOC %zu", &bytes) != 1) return 3;
    std::string doc(bytes, '\0');
    in.read(&doc[0], (std::streamsize)bytes);
    if ((size_t)in.gcount() != bytes) return 3;
    ++n_docs;
    ICP icp;
    std::istringstream y(doc);
    try {
      icp.loadFromYaml(y);
    } catch (const ConfigError& e) {
      std::printf("ERR %s\n", e.what());
      continue;
    } catch (const std::exception& e) {
      std::printf("EXC %s\n", e.what());
      continue;
    }
    std::printf("OK ");
    hex(&icp.loadedChain(), sizeof(lsgpu_loaded_chain));
    std::printf(" ");
    if (icp.chainCuts()) hex(icp.chainCuts(), sizeof(lsgpu_chain_cuts)); else std::printf("-");
    std::printf("\n");
  }
  std::printf("cut_loader_check: ok %d\n", n_docs);
  return 0;
}

#else  // CUT_LOADER_STANDALONE

#include "lsgpu_icp.h"

extern "C" {
void lsgpu_icp_config_default(lsgpu_icp_config* c) { std::memset(c, 0, sizeof(*c)); c->max_iterations = 40; }
void lsgpu_chain_config_default(lsgpu_chain_config* c) { std::memset(c, 0, sizeof(*c)); c->seed = -1; }
void lsgpu_robust_config_default(lsgpu_robust_config* c) { std::memset(c, 0, sizeof(*c)); c->tuning = 1.f; }
void lsgpu_normals_config_default(lsgpu_normals_config* c) { std::memset(c, 0, sizeof(*c)); c->max_angle = -1.f; }
}

namespace {

struct Mod { const char* section; const char* name; std::vector<std::pair<const char*, const char*>> params; };

int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); ++g_fail; } } while (0)

// both entry points on one module list: the same verdict and the same text; the chain's counts are the cuts' counts
int load(const std::vector<Mod>& mods, lsgpu_loaded_chain* chain, lsgpu_chain_cuts* cuts, std::string* why) {
  std::vector<std::vector<lsgpu_yaml_param>> params(mods.size());
  std::vector<lsgpu_yaml_module> list(mods.size());
  for (size_t i = 0; i < mods.size(); ++i) {
    for (const auto& kv : mods[i].params) params[i].push_back({kv.first, kv.second});
    list[i] = {mods[i].section, mods[i].name, params[i].empty() ? nullptr : params[i].data(), (int)params[i].size(), 0};
  }
  char a[512], b[512];
  std::memset(chain, 0xAB, sizeof(*chain));
  std::memset(cuts, 0xCD, sizeof(*cuts));
  const int rc_a = lsgpu_chain_load(list.empty() ? nullptr : list.data(), (int)list.size(), chain, a, (int)sizeof(a));
  const int rc_b = lsgpu_chain_load_cuts(list.empty() ? nullptr : list.data(), (int)list.size(), cuts, b, (int)sizeof(b));
  EXPECT(rc_a == rc_b);
  EXPECT(std::strcmp(a, b) == 0);
  if (rc_a == LSGPU_OK) {
    EXPECT(chain->reserved[2] == cuts->n_reading && chain->reserved[3] == cuts->n_reference);
  } else {   // a refusal leaves both outputs as they were
    const unsigned char* p = reinterpret_cast<const unsigned char*>(chain);
    const unsigned char* q = reinterpret_cast<const unsigned char*>(cuts);
    bool same = true;
    for (size_t i = 0; i < sizeof(*chain); ++i) same = same && p[i] == 0xAB;
    for (size_t i = 0; i < sizeof(*cuts); ++i) same = same && q[i] == 0xCD;
    EXPECT(same);
    // a reason buffer too small for the text: cut, NUL-terminated, nothing written behind it
    char small[16];
    std::memset(small, 0x7F, sizeof(small));
    EXPECT(lsgpu_chain_load_cuts(list.empty() ? nullptr : list.data(), (int)list.size(), cuts, small, 8) == rc_a);
    EXPECT(small[7] == '\0' || std::strlen(small) < 7);
    EXPECT(small[8] == 0x7F && small[15] == 0x7F);
    EXPECT(std::strncmp(small, a, std::strlen(small)) == 0);
  }
  *why = a;
  return rc_a;
}

bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

const Mod kMatcher{"matcher", "KDTreeMatcher", {}};
const Mod kPlane{"errorMinimizer", "PointToPlaneErrorMinimizer", {}};
const Mod kPoint{"errorMinimizer", "PointToPointErrorMinimizer", {}};
const Mod kCounter{"transformationCheckers", "CounterTransformationChecker", {}};
const char* const kRd = "readingDataPointsFilters";
const char* const kRf = "referenceDataPointsFilters";

std::vector<Mod> chain_of(std::vector<Mod> filters, bool point_to_point = false) {
  filters.push_back(kMatcher);
  filters.push_back(point_to_point ? kPoint : kPlane);
  filters.push_back(kCounter);
  return filters;
}

}  // namespace

int main() {
  lsgpu_loaded_chain lc;
  lsgpu_chain_cuts cc;
  std::string why;

  // the issue's document: three cut modules around RandomSampling on the reading, four in front of the sampling filter
  EXPECT(load(chain_of({{kRd, "MinDistDataPointsFilter", {{"minDist", "5"}}},
                        {kRd, "RandomSamplingDataPointsFilter", {{"prob", "0.5"}}},
                        {kRd, "MaxDistDataPointsFilter", {{"maxDist", "25"}}},
                        {kRd, "BoundingBoxDataPointsFilter", {{"xMax", "1"}, {"xMin", "-1"}, {"yMax", "8"}, {"yMin", "-8"}, {"zMax", "3"}, {"zMin", "-3"}}},
                        {kRf, "MaxDistDataPointsFilter", {{"maxDist", "30"}}},
                        {kRf, "MinDistDataPointsFilter", {{"dim", "2"}, {"minDist", ".5"}}},
                        {kRf, "BoundingBoxDataPointsFilter", {{"removeInside", "0"}, {"zMax", "inf"}, {"zMin", "-.inf"}}},
                        {kRf, "RemoveNaNDataPointsFilter", {}},
                        {kRf, "SamplingSurfaceNormalDataPointsFilter", {{"knn", "10"}}}}),
              &lc, &cc, &why) == LSGPU_OK);
  EXPECT(cc.n_reading == 3 && cc.n_reference == 4 && cc.reading_sampling_at == 1 && cc.reserved == 0);
  EXPECT(cc.reading[0].type == LSGPU_FILTER_MIN_DIST && cc.reading[0].dim == -1 && cc.reading[0].v[0] == 5.f);
  EXPECT(cc.reading[1].type == LSGPU_FILTER_MAX_DIST && cc.reading[1].v[0] == 25.f);
  EXPECT(cc.reading[2].type == LSGPU_FILTER_BOUNDING_BOX && cc.reading[2].flag == 1 && cc.reading[2].v[2] == -8.f && cc.reading[2].v[5] == 3.f);
  EXPECT(cc.reference[1].dim == 2 && cc.reference[1].v[0] == 0.5f);
  EXPECT(cc.reference[2].flag == 0 && cc.reference[2].v[0] == -1.f && cc.reference[2].v[4] < -1e38f && cc.reference[2].v[5] > 1e38f);
  EXPECT(cc.reference[3].type == LSGPU_FILTER_REMOVE_NAN && cc.reading[3].type == 0 && cc.reference[7].type == 0);
  EXPECT(lc.chain.reading_prob == 0.5f && lc.chain.ssn_knn == 10 && lc.reserved[4] == 0 && lc.reserved[5] == 0);

  // a point-to-point chain: cut modules alone in the reference section, none on the reading, no RandomSampling
  EXPECT(load(chain_of({{kRf, "RemoveNaNDataPointsFilter", {}}, {kRf, "RemoveNaNDataPointsFilter", {}}}, true), &lc, &cc, &why) == LSGPU_OK);
  EXPECT(cc.n_reading == 0 && cc.n_reference == 2 && cc.reading_sampling_at == 0 && lc.chain.ssn_knn == 0);
  // eight are taken, and without RandomSampling all of the reading's count as in front
  {
    std::vector<Mod> f(8, Mod{kRd, "MaxDistDataPointsFilter", {{"dim", "0"}}});
    f.push_back({kRf, "SurfaceNormalDataPointsFilter", {}});
    EXPECT(load(chain_of(f), &lc, &cc, &why) == LSGPU_OK);
    EXPECT(cc.n_reading == 8 && cc.reading_sampling_at == 8 && cc.reading[7].dim == 0 && cc.reading[7].v[0] == 1.f);
    f.insert(f.begin(), Mod{kRd, "RemoveNaNDataPointsFilter", {}});
    EXPECT(load(chain_of(f), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
    EXPECT(has(why, "MaxDistDataPointsFilter") && has(why, "ninth") && has(why, kRd));
  }
  // without cut modules: all slots 0
  EXPECT(load(chain_of({{kRf, "SurfaceNormalDataPointsFilter", {}}}), &lc, &cc, &why) == LSGPU_OK);
  EXPECT(lc.reserved[2] == 0 && lc.reserved[3] == 0 && cc.n_reading == 0 && cc.n_reference == 0);

  // the refusals, each by name
  const Mod ssn{kRf, "SamplingSurfaceNormalDataPointsFilter", {}};
  EXPECT(load(chain_of({ssn, {kRf, "MinDistDataPointsFilter", {}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(has(why, "MinDistDataPointsFilter behind the module that produces the normals is not implemented") && has(why, "gathered through the cut"));
  EXPECT(load(chain_of({ssn, {kRf, "ObservationDirectionDataPointsFilter", {}}, {kRf, "OrientNormalsDataPointsFilter", {}},
                        {kRf, "BoundingBoxDataPointsFilter", {}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(has(why, "BoundingBoxDataPointsFilter behind the module that produces the normals"));
  EXPECT(load(chain_of({ssn, {kRd, "SurfaceNormalDataPointsFilter", {}}, {kRd, "RemoveNaNDataPointsFilter", {}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(has(why, "readingDataPointsFilters: RemoveNaNDataPointsFilter behind the module that produces the normals"));
  EXPECT(load(chain_of({ssn, {kRd, "MaxDistDataPointsFilter", {{"dim", "3"}}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(why == "MaxDistDataPointsFilter: dim must be an integer in [-1, 2]");
  EXPECT(load(chain_of({ssn, {kRd, "MinDistDataPointsFilter", {{"dim", "0.5"}}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(has(why, "MinDistDataPointsFilter: dim"));
  EXPECT(load(chain_of({ssn, {kRd, "BoundingBoxDataPointsFilter", {{"removeInside", "2"}}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(why == "BoundingBoxDataPointsFilter: removeInside must be 0 or 1");
  EXPECT(load(chain_of({ssn, {kRd, "RemoveNaNDataPointsFilter", {{"dim", "0"}}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(why == "RemoveNaNDataPointsFilter: unknown parameter dim");
  EXPECT(load(chain_of({ssn, {kRd, "MaxDistDataPointsFilter", {{"minDist", "1"}}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(why == "MaxDistDataPointsFilter: unknown parameter minDist");
  EXPECT(load(chain_of({ssn, {kRf, "BoundingBoxDataPointsFilter", {{"xMin", "left"}}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(why == "BoundingBoxDataPointsFilter: xMin is not a number");
  EXPECT(load(chain_of({ssn, {kRf, "MaxDistDataPointsFilter", {{"maxDist", "nan"}}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(why == "MaxDistDataPointsFilter: maxDist is not a number");
  // what stays refused as it was
  for (const char* sec : {kRd, kRf})
    for (const char* name : {"FixStepSamplingDataPointsFilter", "VoxelGridDataPointsFilter", "MaxPointCountDataPointsFilter"}) {
      EXPECT(load(chain_of({{sec, name, {}}, ssn}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
      EXPECT(why == std::string(sec) + ": module " + name + " is not implemented on the HIP path");
    }
  EXPECT(load(chain_of({{kRf, "MaxDistDataPointsFilter", {}}, ssn, {kRf, "SurfaceNormalDataPointsFilter", {}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(has(why, "referenceDataPointsFilters: one module at most"));
  EXPECT(load(chain_of({ssn, {kRd, "MinDistDataPointsFilter", {}}, {kRd, "SurfaceNormalDataPointsFilter", {}},
                        {kRd, "RandomSamplingDataPointsFilter", {}}}), &lc, &cc, &why) == LSGPU_BAD_CONFIG);
  EXPECT(has(why, "SurfaceNormalDataPointsFilter before RandomSamplingDataPointsFilter"));
  // bad arguments
  EXPECT(lsgpu_chain_load_cuts(nullptr, 0, nullptr, nullptr, 0) == LSGPU_BAD_ARG);
  EXPECT(lsgpu_chain_load_cuts(nullptr, 1, &cc, nullptr, 0) == LSGPU_BAD_ARG);
  EXPECT(lsgpu_chain_load_cuts(nullptr, 0, &cc, nullptr, 0) == LSGPU_BAD_CONFIG);   // (no matcher; a NULL reason buffer)

  if (g_fail) { std::printf("cut_loader_check (standalone): %d FAILED\n", g_fail); return 1; }
  std::printf("cut_loader_check (standalone): ok\n");
  return 0;
}

#endif
