// motion_loader_check.cpp -- runs ICP::loadFromYaml (laser_slam_amd/cpp/include/laser_slam_amd/icp.hpp) and the shim's
// LsgpuICP::loadFromYaml (integration/lsgpu_icp_shim.hpp) over a list of documents and prints one line per document:
// "OK <dof> <bound> <maxRotationNorm> <maxTranslationNorm> <bound_before_counter> <hex of lsgpu_loaded_chain>" with what
// motionConfig() reports ("0 0 - - 0": neither module) and every byte of the struct the facade holds, or "ERR <text>" with the
// ConfigError's text; then "SHIM OK" or "SHIM ERR <text>" for the shim on the same document.
// tests/test_constrained_step.py compares the lines with what the Python facade gives for the same documents.
//
// argv[1]: the documents, each as a line "DOC <bytes>" followed by that many bytes of YAML.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "laser_slam_amd/icp.hpp"
#include "laser_slam_amd/ros_msgs.hpp"
#include "lsgpu_icp_shim.hpp"

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
    {
      ICP icp;
      std::istringstream y(doc);
      try {
        icp.loadFromYaml(y);
        const lsgpu_motion_config* m = icp.motionConfig();
        if (m && m->bound)
          std::printf("OK %d %d %.9g %.9g %d ", m->dof, m->bound, (double)m->max_rotation_norm, (double)m->max_translation_norm, m->bound_before_counter);
        else
          std::printf("OK %d 0 - - 0 ", m ? m->dof : 0);
        hex(&icp.loadedChain(), sizeof(lsgpu_loaded_chain));
        std::printf("\n");
      } catch (const ConfigError& e) {
        std::printf("ERR %s\n", e.what());
      } catch (const std::exception& e) {
        std::printf("EXC %s\n", e.what());
      }
    }
    {
      LsgpuICP<LsgpuMirrorPM> shim;
      std::istringstream y(doc);
      try {
        shim.loadFromYaml(y);
        std::printf("SHIM OK\n");
      } catch (const std::exception& e) {
        std::printf("SHIM ERR %s\n", e.what());
      }
    }
  }
  // the struct the FFI front ends mirror: its size and field offsets
  std::printf("LAYOUT %zu %zu %zu %zu %zu %zu %zu\n", sizeof(lsgpu_motion_config), offsetof(lsgpu_motion_config, dof),
              offsetof(lsgpu_motion_config, bound), offsetof(lsgpu_motion_config, max_rotation_norm),
              offsetof(lsgpu_motion_config, max_translation_norm), offsetof(lsgpu_motion_config, bound_before_counter),
              offsetof(lsgpu_motion_config, reserved));
  std::printf("motion_loader_check: ok %d\n", n_docs);
  return 0;
}
