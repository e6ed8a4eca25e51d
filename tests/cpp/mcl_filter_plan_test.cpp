// Drives csrc/mcl_filter_plan.hip.h with a plain host compiler (tests/test_particle_filter_cpu.py): one command per input
// line, every float answered as its bit pattern in hex.
//   odoms  <7 prev> <7 cur> <time_diff> <lin_tc> <ang_tc>   -> rt[3] rq[4] rt_norm rel_ang decay_lin decay_ang
//   nl     <sigma>                                          -> a_ sq2_
//   axes   <3 forward> <3 up>                               -> q[4]
//   mean   <10 sums>                                        -> mean[7]
//   bias   <7 state_prev> <var_dist> <var_ang>              -> prev_pos[3] prev_inv[4] a_lin sq2_lin a_ang sq2_ang
// Inputs are float bit patterns in hex.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "mcl_filter_plan.hip.h"

static float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t to_bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    in >> cmd;
    std::vector<float> v;
    while (in >> tok) v.push_back(from_bits((uint32_t)std::stoul(tok, nullptr, 16)));
    std::vector<float> out;
    if (cmd == "odoms" && v.size() == 17) {
      const dddmr::FilterOdom o = dddmr::filter_set_odoms(&v[0], &v[7], v[14], v[15], v[16]);
      out.insert(out.end(), o.rt, o.rt + 3);
      out.insert(out.end(), o.rq, o.rq + 4);
      out.insert(out.end(), {o.rt_norm, o.rel_ang, o.decay_lin, o.decay_ang});
    } else if (cmd == "nl" && v.size() == 1) {
      float a, sq2;
      dddmr::filter_normal_likelihood(v[0], &a, &sq2);
      out = {a, sq2};
    } else if (cmd == "axes" && v.size() == 6) {
      float q[4];
      dddmr::filter_quat_from_axes(&v[0], &v[3], q);
      out.assign(q, q + 4);
    } else if (cmd == "mean" && v.size() == 10) {
      float m[7];
      dddmr::filter_mean_from_sums(v.data(), m);
      out.assign(m, m + 7);
    } else if (cmd == "bias" && v.size() == 9) {
      const dddmr::FilterBias b = dddmr::filter_bias_plan(&v[0], v[7], v[8]);
      if (!b.has_prev || dddmr::filter_bias_plan(nullptr, v[7], v[8]).has_prev) return 3;
      out.insert(out.end(), b.prev_pos, b.prev_pos + 3);
      out.insert(out.end(), b.prev_inv, b.prev_inv + 4);
      out.insert(out.end(), {b.a_lin, b.sq2_lin, b.a_ang, b.sq2_ang});
    } else {
      std::fprintf(stderr, "bad line: %s\n", line.c_str());
      return 2;
    }
    for (size_t i = 0; i < out.size(); ++i) std::printf("%s%08x", i ? " " : "", to_bits(out[i]));
    std::printf("\n");
  }
  return 0;
}
