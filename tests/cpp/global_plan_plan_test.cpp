// Drives csrc/global_plan_plan.hip.h (the frontier key, the edge filter, the turning angle, the cost of a successor and
// the filing decision of the pre-graph global planner) from a plain host build.  Reads records from stdin, one per line, and
// answers each on one line; floats and doubles travel as hex bit patterns:
//   K <f> <index>                          ->  K <key> <f back> <index back>
//   O <f>:<index> ...                      ->  O <indices in std::set<std::pair<float, unsigned>> order> | <indices in key order>
//   T <px> <py> <cx> <cy> <ex> <ey>        ->  T <cos> <theta (double)>
//   G <g> <w> <factor> <theta> <tw> <i>    ->  G <new_g>            (factor, theta, tw: doubles)
//   E <w> <radius> <d> <inscribed> <rate>  ->  E <skipped> <factor> (all but w: doubles)
//   F <closed> <opened> <g> <f> <new_g> <new_f>  ->  F <0 | 1 | 2>
//   D <ax> <ay> <az> <bx> <by> <bz>        ->  D <distance>
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <set>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "global_plan_plan.hip.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}
static float f32(const std::string& t) {
  const uint32_t u = (uint32_t)std::strtoul(t.c_str(), nullptr, 16);
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static double f64(const std::string& t) {
  const uint64_t u = std::strtoull(t.c_str(), nullptr, 16);
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}

int main() {
  static_assert(dddmr::kGpFound == 0 && dddmr::kGpNoPath == 1 && dddmr::kGpBudget == 2 && dddmr::kGpOpenFull == 3, "DDDMR_GLOBAL_PLAN_* of the header");
  std::string line;
  int records = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind)) continue;
    std::vector<std::string> a;
    for (std::string t; in >> t;) a.push_back(t);
    if (kind == "K" && a.size() == 2) {
      const uint64_t k = dddmr::gp_key(f32(a[0]), (uint32_t)std::strtoul(a[1].c_str(), nullptr, 10));
      std::printf("K %016" PRIx64 " %08x %u\n", k, bits(dddmr::gp_key_f(k)), dddmr::gp_key_index(k));
    } else if (kind == "O") {
      std::set<std::pair<float, unsigned>> s;
      std::vector<uint64_t> keys;
      for (const std::string& t : a) {
        const size_t c = t.find(':');
        if (c == std::string::npos) return 2;
        const float f = f32(t.substr(0, c));
        const unsigned idx = (unsigned)std::strtoul(t.substr(c + 1).c_str(), nullptr, 10);
        if (s.insert({f, idx}).second) keys.push_back(dddmr::gp_key(f, idx));      // (equal pairs collapse)
      }
      std::sort(keys.begin(), keys.end());
      std::printf("O");
      for (const auto& p : s) std::printf(" %u", p.second);
      std::printf(" |");
      for (uint64_t k : keys) std::printf(" %u", dddmr::gp_key_index(k));
      std::printf("\n");
    } else if (kind == "T" && a.size() == 6) {
      const float px = f32(a[0]), py = f32(a[1]), cx = f32(a[2]), cy = f32(a[3]), ex = f32(a[4]), ey = f32(a[5]);
      std::printf("T %08x %016" PRIx64 "\n", bits(dddmr::gp_cos_theta(cx - px, cy - py, ex - cx, ey - cy)), bits(dddmr::gp_theta(px, py, cx, cy, ex, ey)));
    } else if (kind == "G" && a.size() == 6) {
      std::printf("G %08x\n", bits(dddmr::gp_new_g(f32(a[0]), f32(a[1]), f64(a[2]), f64(a[3]), f64(a[4]), f32(a[5]))));
    } else if (kind == "E" && a.size() == 5) {
      std::printf("E %d %016" PRIx64 "\n", dddmr::gp_edge_skipped(f32(a[0]), f64(a[1]), f64(a[2]), f64(a[3])) ? 1 : 0,
                  bits(dddmr::gp_factor(f64(a[4]), f64(a[2]), f64(a[3]))));
    } else if (kind == "F" && a.size() == 6) {
      std::printf("F %d\n", dddmr::gp_file(a[0] == "1", a[1] == "1", f32(a[2]), f32(a[3]), f32(a[4]), f32(a[5])));
    } else if (kind == "D" && a.size() == 6) {
      std::printf("D %08x\n", bits(dddmr::gp_dist(f32(a[0]), f32(a[1]), f32(a[2]), f32(a[3]), f32(a[4]), f32(a[5]))));
    } else {
      return 3;
    }
    ++records;
  }
  std::fprintf(stderr, "%d records\n", records);
  return 0;
}
