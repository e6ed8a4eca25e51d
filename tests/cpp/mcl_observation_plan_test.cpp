// Drives csrc/mcl_observation_plan.hip.h (the cluster order replay and the weights of cbLeGoFeatureCloud) from a plain
// host build.  Reads records from stdin, one per line, and answers each on one line:
//   C <min_size> <n_points> <n_kept> <size>...   ->  C <order>... | <intensity bits of the cluster output q-th>...
//   D <sum_x> <sum_y> <normal_x> <normal_y>      ->  D <branch> <intensity bits>      (hex floats / "nan" accepted)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "mcl_observation_plan.hip.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  std::string line;
  int records = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind == "C") {
      int32_t min_size;
      uint32_t n_points;
      size_t n_kept;
      in >> min_size >> n_points >> n_kept;
      std::vector<uint32_t> sizes(n_kept), order;
      for (size_t c = 0; c < n_kept; ++c) in >> sizes[c];
      if (!in) return 2;
      dddmr::mclobs_order_clusters(sizes.data(), n_kept, order);
      std::printf("C");
      for (uint32_t c : order) std::printf(" %u", c);
      std::printf(" |");
      for (uint32_t c : order) std::printf(" %08x", bits(dddmr::mclobs_cluster_intensity(sizes[c], n_points, min_size)));
      std::printf("\n");
    } else if (kind == "D") {
      std::string t[4];
      in >> t[0] >> t[1] >> t[2] >> t[3];
      if (!in) return 2;
      const double sx = std::strtod(t[0].c_str(), nullptr), sy = std::strtod(t[1].c_str(), nullptr);
      const float nx = std::strtof(t[2].c_str(), nullptr), ny = std::strtof(t[3].c_str(), nullptr);
      const uint32_t br = dddmr::mclobs_branch(sx, sy);
      std::printf("D %u %08x\n", br, br == dddmr::kMclObsClusters ? 0u : bits(dddmr::mclobs_dominant_intensity(br, nx, ny, sx, sy)));
    } else {
      return 3;
    }
    ++records;
  }
  std::fprintf(stderr, "%d records\n", records);
  return 0;
}
