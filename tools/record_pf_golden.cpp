// record_pf_golden.cpp -- records what mcl_3dl's OWN filter code answers, stage by stage, for tests/golden/REF_MCL_PF_*.npz.
// Built by tools/record_pf_golden.py against the reference checkout's include/mcl_3dl/*.h (pf.h, state_6dof.h, quat.h,
// vec3.h, nd.h, the differential-drive motion model) and the stand-ins of oracle/ref/shim; run by no test.  Nothing here
// restates the filter: every stage below is a call into the reference's headers, and the file written holds the inputs,
// the engine's draws as it made them, and the particle set after each stage.
//
//   record_pf_golden N SEED OUT
//
// OUT is a sequence of records: name length (u32), name, 'f' / 'u' (float32 / uint32), rank (u32), dims (u32 each), data.
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include <mcl_3dl/motion_prediction_models/motion_prediction_model_differential_drive.h>
#include <mcl_3dl/nd.h>
#include <mcl_3dl/pf.h>
#include <mcl_3dl/state_6dof.h>

using mcl_3dl::Quat;
using mcl_3dl::State6DOF;
using mcl_3dl::Vec3;
using Base = mcl_3dl::pf::ParticleFilter<State6DOF, float, mcl_3dl::ParticleWeightedMeanQuat>;

struct PF : Base {
  using Base::Base;
  std::default_random_engine& engine() { return engine_; }
};

static FILE* g_out;

static void put(const std::string& name, char kind, const std::vector<uint32_t>& dims, const void* data) {
  const uint32_t len = (uint32_t)name.size(), rank = (uint32_t)dims.size();
  size_t count = 1;
  for (uint32_t d : dims) count *= d;
  fwrite(&len, 4, 1, g_out);
  fwrite(name.data(), 1, len, g_out);
  fwrite(&kind, 1, 1, g_out);
  fwrite(&rank, 4, 1, g_out);
  fwrite(dims.data(), 4, rank, g_out);
  fwrite(data, 4, count, g_out);
}
static void put_f(const std::string& name, const std::vector<float>& v, std::vector<uint32_t> dims) { put(name, 'f', dims, v.data()); }
static void put_u(const std::string& name, uint32_t v) { put(name, 'u', {1}, &v); }

static std::vector<float> state13(const State6DOF& s) {
  std::vector<float> v(13);
  for (size_t i = 0; i < 13; ++i) v[i] = s[i];
  return v;
}

// the particle set as four arrays: states [n][13], noise4 [n][4], probability [n], bias [n]
static void put_set(const std::string& stage, PF& pf) {
  const uint32_t n = (uint32_t)pf.getParticleSize();
  std::vector<float> st, nz, pr, bs;
  for (auto it = pf.begin(); it != pf.end(); ++it) {
    const std::vector<float> s = state13(it->state_);
    st.insert(st.end(), s.begin(), s.end());
    nz.insert(nz.end(), {it->state_.noise_ll_, it->state_.noise_la_, it->state_.noise_al_, it->state_.noise_aa_});
    pr.push_back(it->probability_);
    bs.push_back(it->probability_bias_);
  }
  put_f(stage + "_states", st, {n, 13});
  put_f(stage + "_noise4", nz, {n, 4});
  put_f(stage + "_probability", pr, {n});
  put_f(stage + "_bias", bs, {n});
}

// the six draws of one DiagonalNoiseGenerator call, as diagonal_noise_generator.h:64-73 makes them
static void draw_row(std::default_random_engine& e, const std::vector<float>& mean, const float sigma[6], std::vector<float>& out) {
  for (int i = 0; i < 6; ++i) {
    std::normal_distribution<float> nd(mean[i], sigma[i]);
    out.push_back(nd(e));
  }
}

static void put_estimate(const std::string& stage, PF& pf) {
  State6DOF e = pf.expectationBiased();
  put_f(stage + "_mean_biased", {e.pos_.x_, e.pos_.y_, e.pos_.z_, e.rot_.x_, e.rot_.y_, e.rot_.z_, e.rot_.w_}, {7});
  put_f(stage + "_max_state", state13(pf.max()), {13});
  State6DOF m = pf.expectation(1.0);
  put_f(stage + "_mean", {m.pos_.x_, m.pos_.y_, m.pos_.z_, m.rot_.x_, m.rot_.y_, m.rot_.z_, m.rot_.w_}, {7});
  auto cov = pf.covariance(1.0, 1.0);
  std::vector<float> c(36);
  for (size_t i = 0; i < 36; ++i) c[i] = cov[i / 6][i % 6];
  put_f(stage + "_cov", c, {6, 6});
}

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: %s N SEED OUT\n", argv[0]); return 2; }
  const size_t n = (size_t)atol(argv[1]);
  const unsigned seed = (unsigned)atol(argv[2]);
  g_out = fopen(argv[3], "wb");
  if (!g_out || n == 0) return 2;

  std::mt19937 in(seed * 7919u + 17u);        // the inputs' generator, apart from the filter's engine
  auto uni = [&in](float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(in); };

  PF pf((int)n, seed);
  // ---- the initial set: poses around (3, -2, 0.5), rotations from small roll / pitch and any yaw, used integrals and noise
  {
    float sum = 0;
    for (auto it = pf.begin(); it != pf.end(); ++it) {
      State6DOF& s = it->state_;
      s = State6DOF(Vec3(3.0f + uni(-1, 1), -2.0f + uni(-1, 1), 0.5f + uni(-0.2f, 0.2f)),
                    Quat(Vec3(uni(-0.1f, 0.1f), uni(-0.1f, 0.1f), uni(-3.1f, 3.1f))));
      s.odom_err_integ_lin_ = Vec3(uni(-0.05f, 0.05f), uni(-0.05f, 0.05f), uni(-0.05f, 0.05f));
      s.odom_err_integ_ang_ = Vec3(uni(-0.05f, 0.05f), uni(-0.05f, 0.05f), uni(-0.05f, 0.05f));
      s.noise_ll_ = uni(-0.6f, 0.6f); s.noise_la_ = uni(-0.3f, 0.3f); s.noise_al_ = uni(-0.3f, 0.3f); s.noise_aa_ = uni(-0.6f, 0.6f);
      it->probability_ = uni(0.2f, 1.0f);
      sum += it->probability_;
    }
    for (auto it = pf.begin(); it != pf.end(); ++it) it->probability_ /= sum;
  }
  put_u("n", (uint32_t)n);
  put_set("in", pf);

  // ---- predict
  const float lin_tc = 5.0, ang_tc = 10.0, dt = 0.1f;
  const State6DOF odom_prev(Vec3(10.0f, 4.0f, 0.1f), Quat(Vec3(0.01f, -0.02f, 0.7f)));
  const State6DOF odom_cur(Vec3(10.12f, 4.09f, 0.11f), Quat(Vec3(0.012f, -0.018f, 0.74f)));
  put_f("odom_prev", {odom_prev.pos_.x_, odom_prev.pos_.y_, odom_prev.pos_.z_, odom_prev.rot_.x_, odom_prev.rot_.y_, odom_prev.rot_.z_, odom_prev.rot_.w_}, {7});
  put_f("odom_cur", {odom_cur.pos_.x_, odom_cur.pos_.y_, odom_cur.pos_.z_, odom_cur.rot_.x_, odom_cur.rot_.y_, odom_cur.rot_.z_, odom_cur.rot_.w_}, {7});
  put_f("predict_params", {dt, lin_tc, ang_tc}, {3});
  mcl_3dl::MotionPredictionModelDifferentialDrive model(lin_tc, ang_tc);
  model.setOdoms(odom_prev, odom_cur, dt);
  pf.predict([&model](State6DOF& s) { model.predict(s); });
  put_set("predict", pf);

  // ---- pf::measure with recorded likelihoods (none small enough to be absorbed by the running sum)
  std::vector<float> lik(n);
  for (float& v : lik) v = uni(0.05f, 1.0f);
  put_f("likelihood", lik, {(uint32_t)n});
  {
    size_t at = 0;
    pf.measure([&lik, &at](const State6DOF&) -> float { return lik[at++]; });
  }
  // ---- the bias (src/mcl_3dl.cpp:518-530)
  const double bias_var_dist = 2.0, bias_var_ang = 1.57;
  const State6DOF state_prev(Vec3(3.1f, -2.05f, 0.52f), Quat(Vec3(0.0f, 0.01f, 0.4f)));
  put_f("state_prev", {state_prev.pos_.x_, state_prev.pos_.y_, state_prev.pos_.z_, state_prev.rot_.x_, state_prev.rot_.y_, state_prev.rot_.z_, state_prev.rot_.w_}, {7});
  put_f("bias_params", {(float)bias_var_dist, (float)bias_var_ang}, {2});
  {
    mcl_3dl::NormalLikelihood<float> nl_lin(bias_var_dist);
    mcl_3dl::NormalLikelihood<float> nl_ang(bias_var_ang);
    pf.bias([&](const State6DOF& s, float& p_bias) {
      const float lin_diff = (s.pos_ - state_prev.pos_).norm();
      Vec3 axis;
      float ang_diff;
      (s.rot_ * state_prev.rot_.inv()).getAxisAng(axis, ang_diff);
      p_bias = nl_lin(lin_diff) * nl_ang(ang_diff) + 1e-6;
    });
  }
  put_set("measure", pf);
  put_estimate("measure", pf);
  // the same estimate with every probability times 1.5, so that expectation(1.0)'s break falls inside the array
  {
    PF scaled = pf;
    for (auto it = scaled.begin(); it != scaled.end(); ++it) it->probability_ *= 1.5f;
    put_set("scaled", scaled);
    put_estimate("scaled", scaled);
  }

  // ---- resample: the canonical draw and the noise draws from a copy of the engine, then the reference's own resample
  const float sigma[6] = {0.2f, 0.2f, 0.2f, 0.2f, 0.2f, 0.1f};
  const mcl_3dl::DiagonalNoiseGenerator<float> gen(State6DOF(), State6DOF(Vec3(sigma[0], sigma[1], sigma[2]), Vec3(sigma[3], sigma[4], sigma[5])));
  {
    float accum = 0;
    size_t ties = 0;
    for (auto it = pf.begin(); it != pf.end(); ++it) {
      const float prev = accum;
      accum += it->probability_;
      if (it != pf.begin() && accum == prev) ++ties;
    }
    if (n > 16 && ties) { fprintf(stderr, "N = %zu: %zu ties in accum_probability_\n", n, ties); return 1; }
    put_u("resample_ties", (uint32_t)ties);
    std::default_random_engine copy = pf.engine();
    const float u = std::generate_canonical<float, std::numeric_limits<float>::digits>(copy);
    put_f("resample_u", {u}, {1});
    std::vector<float> draws;
    for (size_t i = 0; i < n; ++i) draw_row(copy, gen.getMean(), sigma, draws);
    put_f("resample_draws", draws, {(uint32_t)n, 6});
    put_f("noise_mean", gen.getMean(), {6});
  }
  pf.resample(State6DOF(Vec3(sigma[0], sigma[1], sigma[2]), Vec3(sigma[3], sigma[4], sigma[5])));
  put_set("resample", pf);
  {
    // what the engine gives next: tells how many rows the reference consumed
    std::default_random_engine copy = pf.engine();
    put_u("engine_after_resample", (uint32_t)copy());
  }

  // ---- pf::noise
  {
    std::default_random_engine copy = pf.engine();
    std::vector<float> draws;
    for (size_t i = 0; i < n; ++i) draw_row(copy, gen.getMean(), sigma, draws);
    put_f("add_noise_draws", draws, {(uint32_t)n, 6});
  }
  pf.noise(State6DOF(Vec3(sigma[0], sigma[1], sigma[2]), Vec3(sigma[3], sigma[4], sigma[5])));
  put_set("add_noise", pf);
  fclose(g_out);
  return 0;
}
