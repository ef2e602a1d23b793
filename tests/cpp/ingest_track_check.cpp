// ingest_track_check.cpp -- LaserTrackParams::ingest_on_device against the path it stands for: one LaserTrack per setting
// over the same scans (one processPoseAndLaserScan per scan, as track_driver.cpp), the library's draw stream reseeded to
// the same state in front of each run.  Equal, byte for byte: every stored scan (features and normals) and every ICP
// transformation.  With ingest on, ICP::slotTraffic() must show one ingest per scan and no upload.
//   usage: ingest_track_check <dir> <n_scans> <scans_on_device> <nscan_in_sub_map>
// <dir>/scan<i>.bin = float32 N x 4, <dir>/poses.txt = "t_ns qw qx qy qz px py pz" per scan, <dir>/input_filters.yaml,
// <dir>/icp.yaml.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "laser_slam_amd/laser_track.hpp"

using namespace laser_slam_amd;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static DataPoints readScan(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
  f.seekg(0, std::ios::end);
  const size_t bytes = (size_t)f.tellg();
  f.seekg(0);
  DataPoints d;
  d.features.resize(bytes / 4);
  f.read(reinterpret_cast<char*>(d.features.data()), (std::streamsize)bytes);
  return d;
}

struct Run {
  std::vector<LaserScan> scans;
  std::vector<RelativePose> icp;
  ICP::SlotTraffic traffic;
  double ingest_ms = 0;
};

static Run run(const std::string& dir, int n, int on_device, int sub_map, bool ingest) {
  LaserTrackParams p;
  p.icp_configuration_file = dir + "/icp.yaml";
  p.icp_input_filters_file = dir + "/input_filters.yaml";
  p.nscan_in_sub_map = sub_map;
  p.scans_on_device = on_device;
  p.ingest_on_device = ingest;
  int64_t none = 0;
  lsgpu_filter_random_sampling(0, 0.5f, 11, &none);   // the draw stream starts here for either run; the track continues it
  LaserTrack track(p, 0u);
  std::ifstream poses(dir + "/poses.txt");
  Run out;
  for (int i = 0; i < n; ++i) {
    Pose pose;
    double q[4], t[3];
    long long tns;
    poses >> tns >> q[0] >> q[1] >> q[2] >> q[3] >> t[0] >> t[1] >> t[2];
    pose.time_ns = tns;
    pose.T_w = SE3({q[0], q[1], q[2], q[3]}, {t[0], t[1], t[2]});
    LaserScan scan;
    scan.time_ns = tns;
    scan.scan = readScan(dir + "/scan" + std::to_string(i) + ".bin");
    track.processPoseAndLaserScan(pose, scan);
    out.ingest_ms += track.lastStageTimes().ingest_ms;
    if (!ingest) CHECK(track.lastStageTimes().ingest_ms == 0);
  }
  out.scans = track.getLaserScans();
  out.icp = track.getIcpTransformations();
  out.traffic = track.icp().slotTraffic();
  return out;
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const std::string dir = argv[1];
  const int n = std::atoi(argv[2]), on_device = std::atoi(argv[3]), sub_map = std::atoi(argv[4]);
  try {
    const Run a = run(dir, n, on_device, sub_map, false), b = run(dir, n, on_device, sub_map, true);
    CHECK((int)a.scans.size() == n && (int)b.scans.size() == n);
    for (size_t i = 0; i < a.scans.size() && i < b.scans.size(); ++i) {
      const DataPoints &x = a.scans[i].scan, &y = b.scans[i].scan;
      CHECK(x.getNbPoints() > 0 && x.normals.size() == (size_t)x.getNbPoints() * 3);
      CHECK(x.features.size() == y.features.size() && std::memcmp(x.features.data(), y.features.data(), x.features.size() * 4) == 0);
      CHECK(x.normals.size() == y.normals.size() && std::memcmp(x.normals.data(), y.normals.data(), x.normals.size() * 4) == 0);
      CHECK(a.scans[i].time_ns == b.scans[i].time_ns && a.scans[i].key == b.scans[i].key);
    }
    CHECK((int)a.icp.size() == n - 1 && a.icp.size() == b.icp.size());
    for (size_t i = 0; i < a.icp.size() && i < b.icp.size(); ++i) {
      const auto qa = a.icp[i].T_a_b.quaternion(), qb = b.icp[i].T_a_b.quaternion();
      const auto pa = a.icp[i].T_a_b.position(), pb = b.icp[i].T_a_b.position();
      CHECK(std::memcmp(qa.data(), qb.data(), sizeof(qa)) == 0 && std::memcmp(pa.data(), pb.data(), sizeof(pa)) == 0);
      CHECK(a.icp[i].time_a_ns == b.icp[i].time_a_ns && a.icp[i].time_b_ns == b.icp[i].time_b_ns && a.icp[i].key_a == b.icp[i].key_a &&
            a.icp[i].key_b == b.icp[i].key_b);
      std::printf("icp %zu q %.9f %.9f %.9f %.9f p %.9f %.9f %.9f\n", i, qa[0], qa[1], qa[2], qa[3], pa[0], pa[1], pa[2]);
    }
    std::printf("traffic off: uploads %llu ingests %llu; on: uploads %llu ingests %llu (ingest %.3f ms in all)\n",
                (unsigned long long)a.traffic.uploads, (unsigned long long)a.traffic.ingests, (unsigned long long)b.traffic.uploads,
                (unsigned long long)b.traffic.ingests, b.ingest_ms);
    CHECK(a.traffic.ingests == 0 && a.traffic.uploads == (uint64_t)n);   // every scan crossed a second time
    CHECK(b.traffic.ingests == (uint64_t)n && b.traffic.uploads == 0);
    CHECK(b.ingest_ms > 0);
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  if (fails) { std::printf("ingest_track_check: %d FAILED\n", fails); return 1; }
  std::printf("ingest_track_check: ok\n");
  return 0;
}
