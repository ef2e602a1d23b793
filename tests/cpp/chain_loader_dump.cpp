// chain_loader_dump.cpp -- runs ICP::loadFromYaml (laser_slam_amd/cpp/include/laser_slam_amd/icp.hpp) over a list of documents
// and prints one line per document: "OK <hex>" with the bytes of the lsgpu_loaded_chain the facade's public accessors give
// back, or "ERR <text>" with the ConfigError's text ("EXC <text>" for any other exception, which no document should raise).
// tests/test_chain_loader.py compares the lines with what the Python facade gives for the same documents.
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
    lsgpu_loaded_chain c;
    std::memset(&c, 0, sizeof(c));
    c.icp = icp.config();
    c.chain.reading_prob = icp.readingSamplingProb();
    c.chain.ssn_knn = icp.surfaceNormalKnn();
    c.chain.ssn_ratio = icp.surfaceNormalRatio();
    c.chain.sn_knn = icp.referenceNormalKnn();
    c.chain.seed = icp.seed();
    lsgpu_robust_config_default(&c.robust);
    lsgpu_normals_config_default(&c.normals);
    if (icp.robustFilter()) { c.robust = *icp.robustFilter(); c.has_robust = 1; }
    if (icp.normalsConfig()) { c.normals = *icp.normalsConfig(); c.has_normals = 1; }
    std::printf("OK ");
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&c);
    for (size_t i = 0; i < sizeof(c); ++i) std::printf("%02x", b[i]);
    std::printf("\n");
  }
  std::printf("chain_loader_dump: ok %d\n", n_docs);
  return 0;
}
