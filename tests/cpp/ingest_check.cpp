// ingest_check.cpp -- CPU-only checks of the ingest path above the library (include/lsgpu_icp.h, lsgpu_cloud_ingest): the
// facade (ICP::ingestCloud, ICP::slotTraffic), LaserTrackParams::ingest_on_device and StageTimes::ingest_ms, and the shim
// with the mirror types.  No device is touched: nothing here ingests.  With -DINGEST_CHECK_OVERLAY (g++ -fsyntax-only
// against tests/cpp/mock/) the same names are resolved through the GTSAM-typed overlay.
#include <cstdio>
#include <sstream>
#include <string>
#include <type_traits>

#ifdef INGEST_CHECK_OVERLAY
#include <laser_slam/laser_track.hpp>
#include <laser_slam/parameters.hpp>
#endif
#include "laser_slam_amd/laser_track.hpp"
#include "../../integration/lsgpu_icp_shim.hpp"

using namespace laser_slam_amd;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the calls a driver makes, resolved and instantiated; never run here (they need a device)
void facade_calls(ICP& icp, DataPoints& cloud, DataPointsFilters& filters) {
  icp.ingestCloud(2, cloud, filters);
  const ICP::SlotTraffic t = icp.slotTraffic();
  (void)t.uploads; (void)t.ingests;
}
void shim_calls(LsgpuICP<LsgpuMirrorPM>& shim, DataPoints& cloud, LsgpuDataPointsFilters<LsgpuMirrorPM>& filters) {
  shim.ingestCloud(1, cloud, filters);
  shim.uploadCloud(0, cloud);
  (void)shim.cloudSize(1);
}
void track_calls(LaserTrack& track, const LaserScan& scan, const Pose& pose) {
  track.processPoseAndLaserScan(pose, scan);
  track.processLaserScan(scan);
  (void)track.lastStageTimes().ingest_ms;
  (void)track.icp().slotTraffic().ingests;
}
#ifdef INGEST_CHECK_OVERLAY
void overlay_calls() {
  laser_slam::LaserTrackParams p;
  p.ingest_on_device = true;
}
#endif

int main() {
  CHECK(!LaserTrackParams().ingest_on_device);
  CHECK(LaserTrackParams().scans_on_device == 16 && LaserTrackParams().overlap_scan_copy);   // (its neighbours are as they were)
  LaserTrack::StageTimes st;
  CHECK(st.ingest_ms == 0 && st.copy_ms == 0 && st.upload_ms == 0 && st.icp_ms == 0);
  ICP icp;
  CHECK(icp.slotTraffic().uploads == 0 && icp.slotTraffic().ingests == 0);
  static_assert(std::is_same<decltype(&ICP::ingestCloud), void (ICP::*)(int, DataPoints&, DataPointsFilters&)>::value, "ICP::ingestCloud(slot, cloud, filters)");
  // the shim's feature write-back with the mirror types
  DataPoints d;
  d.features = {1, 2, 3, 1, 4, 5, 6, 1, 7, 8, 9, 1};
  const float kept[8] = {4, 5, 6, 1, 7, 8, 9, 1};
  LsgpuCloudTraits<LsgpuMirrorPM>::setFeatures(d, kept, 2);
  CHECK(d.getNbPoints() == 2 && d.features[0] == 4.f && d.features[7] == 1.f);
  LsgpuCloudTraits<LsgpuMirrorPM>::setFeatures(d, kept, 0);
  CHECK(d.getNbPoints() == 0);
  LsgpuICP<LsgpuMirrorPM> shim;
  CHECK(shim.cloudSize(0) == -1);   // (no handle yet: nothing is created to answer)
  if (fails) { std::printf("ingest_check: %d FAILED\n", fails); return 1; }
  std::printf("ingest_check: ok\n");
  return 0;
}
