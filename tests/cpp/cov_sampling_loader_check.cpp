// cov_sampling_loader_check.cpp -- runs ICP::loadFromYaml (laser_slam_amd/cpp/include/laser_slam_amd/icp.hpp) over a list of
// documents and prints one line per document: "OK <reading nbSample,torqueNorm | -> <reference nbSample,torqueNorm | -> <hex of
// lsgpu_loaded_chain> <hex of lsgpu_chain_cuts>" with what covSamplingConfig() reports ("-": no
// CovarianceSamplingDataPointsFilter in that section) and every byte of the two structs the facade holds (a document without
// cut modules: the zero-filled struct), or "ERR <text>" with the ConfigError's text.  tests/test_covariance_sampling.py
// compares the lines with what the Python facade gives for the same documents.
//
// argv[1]: the documents, each as a line "DOC <bytes>" followed by that many bytes of YAML.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

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
    const lsgpu_cov_sampling_config* s = icp.covSamplingConfig();
    std::printf("OK ");
    if (s && s->reading_nb_sample > 0) std::printf("%d,%d ", s->reading_nb_sample, s->reading_torque_norm); else std::printf("- ");
    if (s && s->reference_nb_sample > 0) std::printf("%d,%d ", s->reference_nb_sample, s->reference_torque_norm); else std::printf("- ");
    hex(&icp.loadedChain(), sizeof(lsgpu_loaded_chain));
    std::printf(" ");
    lsgpu_chain_cuts none;
    std::memset(&none, 0, sizeof(none));
    hex(icp.chainCuts() ? icp.chainCuts() : &none, sizeof(lsgpu_chain_cuts));
    std::printf("\n");
  }
  // the struct the FFI front ends mirror: its size and field offsets
  std::printf("LAYOUT %zu %zu %zu %zu %zu %zu\n", sizeof(lsgpu_cov_sampling_config), offsetof(lsgpu_cov_sampling_config, reading_nb_sample),
              offsetof(lsgpu_cov_sampling_config, reference_nb_sample), offsetof(lsgpu_cov_sampling_config, reading_torque_norm),
              offsetof(lsgpu_cov_sampling_config, reference_torque_norm), offsetof(lsgpu_cov_sampling_config, reserved));
  std::printf("cov_sampling_loader_check: ok %d\n", n_docs);
  return 0;
}
