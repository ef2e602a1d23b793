// max_density_loader_check.cpp -- runs ICP::loadFromYaml (laser_slam_amd/cpp/include/laser_slam_amd/icp.hpp) over a list of
// documents and prints one line per document: "OK <maxDensity | -> <hex>" with what maxDensityConfig() reports ("-": the chain
// does not name MaxDensityDataPointsFilter) and every byte of the lsgpu_loaded_chain the facade holds, reserved slots included
// (tests/cpp/chain_loader_dump.cpp rebuilds the struct from the older accessors and leaves them 0), or "ERR <text>" with the
// ConfigError's text.  tests/test_max_density.py compares the lines with what the Python facade gives for the same documents.
//
// argv[1]: the documents, each as a line "DOC <bytes>" followed by that many bytes of YAML.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "laser_slam_amd/icp.hpp"

using namespace laser_slam_amd;

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
    float md = -1.f;
    if (icp.maxDensityConfig(&md)) std::printf("OK %.9g ", (double)md); else std::printf("OK - ");
    const lsgpu_loaded_chain& c = icp.loadedChain();
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&c);
    for (size_t i = 0; i < sizeof(c); ++i) std::printf("%02x", b[i]);
    std::printf("\n");
  }
  std::printf("max_density_loader_check: ok %d\n", n_docs);
  return 0;
}
