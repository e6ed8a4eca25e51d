// Drives csrc/mcl_submap_plan.hip.h (the keyframe transform and the keyframe radius search of SubMaps) from a plain host
// build.  Reads records from stdin, one per line, and answers each on one line (numbers as %.17g or hex floats):
//   S <radius> <px> <py> <pz> <n> <x y z>...      ->  S <count> <id>...          (keyframe positions as doubles)
//   T <t0 .. t11> <n> <x y z>...                  ->  T <bits of x' y' z'>...    (points as floats)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mcl_submap_plan.hip.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static bool number(std::istringstream& in, double* v) {
  std::string t;
  if (!(in >> t)) return false;
  *v = std::strtod(t.c_str(), nullptr);
  return true;
}

int main() {
  std::string line;
  int records = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    if (kind == "S") {
      double radius, pos[3], nd;
      if (!number(in, &radius) || !number(in, &pos[0]) || !number(in, &pos[1]) || !number(in, &pos[2]) || !number(in, &nd)) return 2;
      const size_t n = (size_t)nd;
      std::vector<float> kf(3 * n);
      for (size_t i = 0; i < 3 * n; ++i) {
        double v;
        if (!number(in, &v)) return 2;
        kf[i] = (float)v;
      }
      std::vector<int32_t> ids(n + 1);
      const size_t cnt = dddmr::submap_select(kf.data(), n, pos, radius, ids.data(), n);
      if (dddmr::submap_select(kf.data(), n, pos, radius, nullptr, 0) != cnt) return 4;      // count only
      std::printf("S %zu", cnt);
      for (size_t i = 0; i < cnt; ++i) std::printf(" %d", ids[i]);
      std::printf("\n");
    } else if (kind == "T") {
      double T[12], nd;
      for (double& t : T)
        if (!number(in, &t)) return 2;
      if (!number(in, &nd)) return 2;
      std::printf("T");
      for (size_t i = 0; i < (size_t)nd; ++i) {
        double p[3];
        if (!number(in, &p[0]) || !number(in, &p[1]) || !number(in, &p[2])) return 2;
        for (int r = 0; r < 3; ++r) std::printf(" %08x", bits(dddmr::submap_transform_row(T, r, (float)p[0], (float)p[1], (float)p[2])));
      }
      std::printf("\n");
    } else {
      return 3;
    }
    ++records;
  }
  std::fprintf(stderr, "%d records\n", records);
  return 0;
}
