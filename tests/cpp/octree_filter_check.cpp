// octree_filter_check.cpp -- OctreeGridDataPointsFilter in the C++ facades, without a device: every file named on the command
// line goes through laser_slam_amd::DataPointsFilters (the parser), LsgpuDataPointsFilters (the shim, through that parser)
// and a LaserTrack that names it as icp_input_filters_file; the descriptors -- or each facade's refusal -- are printed for the
// test to compare (tests/test_octree_filter.py).  The descriptor rule of apply() is checked here too: it throws before a
// handle is made.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "laser_slam_amd/laser_track.hpp"
#include "lsgpu_icp_shim.hpp"

using namespace laser_slam_amd;

// does apply() refuse the cloud because of the descriptor rule?  (a chain the rule lets pass goes on to look for a device,
// which this program may not have: any other outcome, that failure included, counts as "passes")
template <class Filters>
static bool rule_fires(const char* yaml, DataPoints cloud) {
  std::istringstream y(yaml);
  Filters flt(y);
  try {
    flt.apply(cloud);
  } catch (const std::exception& e) {
    return std::string(e.what()).find("samplingMethod 2 (Centroid) on a cloud with descriptors") != std::string::npos;
  }
  return false;
}

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::printf("FILE %s\n", argv[a]);
    size_t n = 0;
    bool bad = false;
    try {
      std::ifstream f(argv[a]);
      DataPointsFilters flt(f);
      n = flt.size();
      for (const auto& m : flt.modules())
        std::printf("MODULE %d %d %d %.9g %.9g %.9g %.9g %.9g %.9g\n", m.type, m.dim, m.flag, m.v[0], m.v[1], m.v[2], m.v[3], m.v[4], m.v[5]);
    } catch (const ConfigError& e) {
      std::printf("CONFIG_ERROR %s\n", e.what());
      bad = true;
    }
    try {
      std::ifstream f(argv[a]);
      LsgpuDataPointsFilters<LsgpuMirrorPM> shim(f);
      std::printf("SHIM %zu %s\n", shim.size(), !bad && shim.size() == n ? "same" : "DIFFERENT");
    } catch (const std::runtime_error& e) {
      std::printf("SHIM_ERROR %s\n", e.what());
    }
    try {
      LaserTrackParams p;
      p.use_icp_factors = false;
      p.icp_input_filters_file = argv[a];
      LaserTrack track(p, 0u);
      std::printf("TRACK %zu\n", track.inputFilters().size());
    } catch (const ConfigError& e) {
      std::printf("TRACK_ERROR %s\n", e.what());
    }
  }
  // Centroid on a cloud with normals: refused by apply(), by both facades, before a device is looked for.  The methods that
  // return an input point, and Centroid on a cloud without normals, are not refused by the rule.
  DataPoints with_normals, plain;
  with_normals.features = {0, 0, 0, 1, 1, 1, 1, 1};
  with_normals.normals = {0, 0, 1, 0, 0, 1};
  plain.features = with_normals.features;
  const char* centroid = "- OctreeGridDataPointsFilter: {samplingMethod: 2}\n";
  const char* medoid = "- OctreeGridDataPointsFilter: {samplingMethod: 3}\n";
  const bool threw = rule_fires<DataPointsFilters>(centroid, with_normals);
  const bool shim_threw = rule_fires<LsgpuDataPointsFilters<LsgpuMirrorPM>>(centroid, with_normals);
  const bool picks = !rule_fires<DataPointsFilters>(medoid, with_normals) && !rule_fires<LsgpuDataPointsFilters<LsgpuMirrorPM>>(medoid, with_normals);
  const bool no_normals = !rule_fires<DataPointsFilters>(centroid, plain) && !rule_fires<LsgpuDataPointsFilters<LsgpuMirrorPM>>(centroid, plain);
  std::printf("DESCRIPTOR_RULE %s %s %s %s\n", threw ? "throws" : "SILENT", shim_threw ? "throws" : "SILENT", picks ? "passes" : "REFUSED",
              no_normals ? "passes" : "REFUSED");
  return threw && shim_threw && picks && no_normals ? 0 : 1;
}
