// voxel_filter_check.cpp -- VoxelGridDataPointsFilter in the C++ facades, without a device: every file named on the command
// line goes through laser_slam_amd::DataPointsFilters (the parser), LsgpuDataPointsFilters (the shim, through that parser)
// and a LaserTrack that names it as icp_input_filters_file; the descriptors are printed for the test to compare
// (tests/test_voxel_grid_filter.py).  The descriptor rule of apply() is checked here too: it throws before a handle is made.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "laser_slam_amd/laser_track.hpp"
#include "lsgpu_icp_shim.hpp"

using namespace laser_slam_amd;

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::printf("FILE %s\n", argv[a]);
    size_t n = 0;
    try {
      std::ifstream f(argv[a]);
      DataPointsFilters flt(f);
      n = flt.size();
      for (const auto& m : flt.modules())
        std::printf("MODULE %d %d %d %.9g %.9g %.9g %.9g %.9g %.9g\n", m.type, m.dim, m.flag, m.v[0], m.v[1], m.v[2], m.v[3], m.v[4], m.v[5]);
    } catch (const ConfigError& e) {
      std::printf("CONFIG_ERROR %s\n", e.what());
      continue;
    }
    {
      std::ifstream f(argv[a]);
      LsgpuDataPointsFilters<LsgpuMirrorPM> shim(f);
      std::printf("SHIM %zu %s\n", shim.size(), shim.size() == n ? "same" : "DIFFERENT");
    }
    LaserTrackParams p;
    p.use_icp_factors = false;
    p.icp_input_filters_file = argv[a];
    LaserTrack track(p, 0u);
    std::printf("TRACK %zu\n", track.inputFilters().size());
  }
  // averageExistingDescriptors 1 (the default) on a cloud with normals: ConfigError from apply(), from both facades, before
  // a device is looked for; with 0 the rule does not fire (the call then needs a device, which this program does not use)
  std::istringstream y("- VoxelGridDataPointsFilter: {vSizeX: 0.5}\n");
  DataPointsFilters flt(y);
  DataPoints cloud;
  cloud.features = {0, 0, 0, 1, 1, 1, 1, 1};
  cloud.normals = {0, 0, 1, 0, 0, 1};
  bool threw = false;
  try { flt.apply(cloud); } catch (const ConfigError&) { threw = true; }
  std::istringstream y2("- VoxelGridDataPointsFilter: {vSizeX: 0.5}\n");
  LsgpuDataPointsFilters<LsgpuMirrorPM> shim(y2);
  bool shim_threw = false;
  try { shim.apply(cloud); } catch (const std::runtime_error& e) { shim_threw = std::string(e.what()).find("averageExistingDescriptors") != std::string::npos; }
  std::printf("DESCRIPTOR_RULE %s %s\n", threw ? "throws" : "SILENT", shim_threw ? "throws" : "SILENT");
  return threw && shim_threw ? 0 : 1;
}
