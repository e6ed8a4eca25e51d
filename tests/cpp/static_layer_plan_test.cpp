// Drives csrc/static_layer_plan.hip.h (the adaptive radii, the grid cell choice and the edge-capacity decision of the
// static layer) from a plain host build.  Reads records from stdin, one per line, and answers each on one line:
//   R                                  ->  R <bits of float(r_k * r_k)> for k = 1 .. 101
//   Q <radius>                         ->  Q <bits of float(radius * radius)>
//   C <adaptive> <radius> <inscribed> <inflation>   ->  C <bits of the ground, map and zone cell sizes>
//   E <n_edges> <max_edges>            ->  E <0 | 1>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "static_layer_plan.hip.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  static_assert(dddmr::kSlAdaptiveSteps == 101 && dddmr::kSlMaxAdaptiveNumber == 32, "the reference's loop, the create's limit");
  std::string line;
  int records = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind == "R") {
      std::printf("R");
      for (int k = 1; k <= dddmr::kSlAdaptiveSteps; ++k) std::printf(" %08x", bits(dddmr::sl_radius2(dddmr::sl_adaptive_radius(k))));
      std::printf("\n");
    } else if (kind == "Q") {
      std::string t;
      if (!(in >> t)) return 2;
      std::printf("Q %08x\n", bits(dddmr::sl_radius2(std::strtod(t.c_str(), nullptr))));
    } else if (kind == "C") {
      int adaptive;
      std::string r, ins, infl;
      if (!(in >> adaptive >> r >> ins >> infl)) return 2;
      std::printf("C %08x %08x %08x\n", bits(dddmr::sl_ground_cell(adaptive != 0, std::strtod(r.c_str(), nullptr))),
                  bits(dddmr::sl_map_cell(std::strtod(ins.c_str(), nullptr))), bits(dddmr::sl_zone_cell(std::strtod(infl.c_str(), nullptr))));
    } else if (kind == "E") {
      unsigned long long n, cap;
      if (!(in >> n >> cap)) return 2;
      std::printf("E %d\n", dddmr::sl_edges_fit((uint64_t)n, (uint32_t)cap) ? 1 : 0);
    } else {
      return 3;
    }
    ++records;
  }
  std::fprintf(stderr, "%d records\n", records);
  return 0;
}
