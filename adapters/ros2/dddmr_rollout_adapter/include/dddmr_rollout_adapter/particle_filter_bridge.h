// particle_filter_bridge.h -- the mcl_3dl side of the resident particle set: what a patched MCL3dlNode calls instead of
// pf_->predict / measure / resample / noise, and the two helpers that make the caller's draws the reference's draws.
//
//   pf_->predict(prediction_func)        (src/mcl_3dl.cpp:200-205)   -> predict()
//   MCL3dlNode::measure up to :601       (src/mcl_3dl.cpp:466-601)   -> measure(), resetInteg()
//   pf_->resample(sigma)                 (src/mcl_3dl.cpp:213-219)   -> resample(engine, ...)
//   pf_->predict(update_noise_func)      (src/mcl_3dl.cpp:221-229)   -> setNoise()
//   pf_->noise(sigma)                    (include/mcl_3dl/pf.h:221-232) -> addNoise(engine, ...)
//
// The library draws no random number.  canonicalDraw() is the u that libstdc++'s
// uniform_real_distribution<float>(0, pstep) multiplies by pstep; drawNoiseRows() makes, per row, the six fresh
// std::normal_distribution<float> draws of DiagonalNoiseGenerator::operator() (diagonal_noise_generator.h:64-73) and
// State6DOF::generateNoise's state from them (state_6dof.h:200-221), Quat::setRPY's float sines and cosines included.
// The reference draws a row only for a duplicate, and how many there are is known only after the device's resample:
// resample() copies the engine after u, draws one row per particle, and afterwards sets the engine to the copy advanced
// by exactly n_duplicates rows -- the state the reference's engine is in after its resample.
//
// This header includes nothing of ROS, PCL or the reference: it is compiled and run in a plain C++ toolchain
// (tests/cpp/particle_filter_bridge_test.cpp).  It sits on the context a LocalizationBridge::create has prepared.
#ifndef DDDMR_ROLLOUT_ADAPTER_PARTICLE_FILTER_BRIDGE_H_
#define DDDMR_ROLLOUT_ADAPTER_PARTICLE_FILTER_BRIDGE_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "dddmr_rollout.h"

namespace dddmr_rollout_adapter
{

class ParticleFilterBridge
{
public:
  int create(
    dddmr_rollout_ctx * ctx, uint32_t max_particles, double odom_err_integ_lin_tc, double odom_err_integ_ang_tc, double bias_var_dist,
    double bias_var_ang)
  {
    ctx_ = nullptr;
    n_ = 0;
    if (!ctx) {return DDDMR_ERR_BAD_ARG;}
    dddmr_mcl_filter_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.max_particles = max_particles;
    cfg.odom_err_integ_lin_tc = odom_err_integ_lin_tc; cfg.odom_err_integ_ang_tc = odom_err_integ_ang_tc;
    cfg.bias_var_dist = bias_var_dist; cfg.bias_var_ang = bias_var_ang;
    const int rc = dddmr_rollout_mcl_filter_create(ctx, &cfg);
    if (rc == DDDMR_OK) {ctx_ = ctx;}
    return rc;
  }
  bool created() const {return ctx_ != nullptr;}
  size_t size() const {return n_;}

  // states [n][13] in State6DOF::operator[] order; probability NULL: 1.0 / n; noise4 NULL: zeros
  int setParticles(const float * states, const float * probability, const float * noise4, size_t n)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    const int rc = dddmr_rollout_mcl_filter_set_particles(ctx_, states, probability, noise4, n);
    if (rc == DDDMR_OK) {n_ = n;}
    return rc;
  }
  int getParticles(std::vector<float> & states, std::vector<float> & probability)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    states.resize(n_ * 13); probability.resize(n_);
    size_t n = 0;
    return dddmr_rollout_mcl_filter_get_particles(ctx_, states.data(), probability.data(), nullptr, nullptr, n_, &n);
  }
  // State: anything with pos_.x_ .. and rot_.x_ .. (State6DOF)
  template<class State>
  int predict(const State & odom_prev, const State & odom_cur, float time_diff)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    float a[7], b[7];
    pose7(odom_prev, a); pose7(odom_cur, b);
    return dddmr_rollout_mcl_filter_predict(ctx_, a, b, (double)time_diff);
  }
  // state_prev NULL: the branch for more particles than num_particles_ (p_bias = 1)
  template<class State>
  int measure(const State * state_prev, dddmr_mcl_filter_estimate * estimate, dddmr_mcl_stats * stats = nullptr)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    float p[7];
    if (state_prev) {pose7(*state_prev, p);}
    return dddmr_rollout_mcl_filter_measure(ctx_, nullptr, nullptr, n_, state_prev ? p : nullptr, estimate, stats);
  }
  int resetInteg() {return ctx_ ? dddmr_rollout_mcl_filter_reset_integ(ctx_) : DDDMR_ERR_STATE;}

  // update_noise_func: four std::normal_distribution<float>(0, 1) draws per particle from ONE distribution object, as
  // the reference keeps it, each times its odom_err_* factor (doubles in Parameters: a double product, stored as float)
  template<class Engine>
  int setNoise(Engine & engine, double lin_lin, double lin_ang, double ang_ang, double ang_lin)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    std::normal_distribution<float> noise(0.0, 1.0);
    noise4_.resize(n_ * 4);
    for (size_t i = 0; i < n_; ++i) {
      float * z = &noise4_[4 * i];            // stored as noise_ll_, noise_la_, noise_al_, noise_aa_; drawn ll, la, aa, al
      z[0] = noise(engine) * lin_lin;
      z[1] = noise(engine) * lin_ang;
      z[3] = noise(engine) * ang_ang;
      z[2] = noise(engine) * ang_lin;
    }
    return dddmr_rollout_mcl_filter_set_noise(ctx_, noise4_.data(), n_);
  }

  // ---- the draws ----------------------------------------------------------------------------------------------------
  template<class Engine>
  static float canonicalDraw(Engine & engine)
  {
    return std::generate_canonical<float, std::numeric_limits<float>::digits>(engine);
  }
  // Quat::setRPY (include/mcl_3dl/quat.h:202-215) into q[4] = x y z w
  static void quatFromRPY(const float rpy[3], float q[4])
  {
    const float t2 = std::cos(rpy[0] / 2), t3 = std::sin(rpy[0] / 2);
    const float t4 = std::cos(rpy[1] / 2), t5 = std::sin(rpy[1] / 2);
    const float t0 = std::cos(rpy[2] / 2), t1 = std::sin(rpy[2] / 2);
    q[0] = t0 * t3 * t4 - t1 * t2 * t5;
    q[1] = t0 * t2 * t5 + t1 * t3 * t4;
    q[2] = t1 * t2 * t4 - t0 * t3 * t5;
    q[3] = t0 * t2 * t4 + t1 * t3 * t5;
  }
  // n rows of 10 floats appended to `rows`; mean / sigma: x y z roll pitch yaw of the DiagonalNoiseGenerator
  template<class Engine>
  static void drawNoiseRows(Engine & engine, const float mean[6], const float sigma[6], size_t n, std::vector<float> & rows)
  {
    for (size_t r = 0; r < n; ++r) {
      float d[6];
      for (int i = 0; i < 6; ++i) {
        std::normal_distribution<float> nd(mean[i], sigma[i]);
        d[i] = nd(engine);
      }
      float row[10] = {d[0], d[1], d[2], 0, 0, 0, 0, d[3] - mean[3], d[4] - mean[4], d[5] - mean[5]};
      quatFromRPY(d + 3, row + 3);
      rows.insert(rows.end(), row, row + 10);
    }
  }

  // pf_->resample(sigma) with the node's engine; mean: the generator's (zeros for State6DOF())
  template<class Engine>
  int resample(Engine & engine, const float mean[6], const float sigma[6], dddmr_mcl_filter_resample_stats * stats = nullptr)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    const float u = canonicalDraw(engine);
    const Engine after_u = engine;
    rows_.clear();
    drawNoiseRows(engine, mean, sigma, n_, rows_);
    dddmr_mcl_filter_resample_stats st;
    std::memset(&st, 0, sizeof(st));
    const int rc = dddmr_rollout_mcl_filter_resample(ctx_, (double)u, rows_.data(), n_, &st);
    if (stats) {*stats = st;}
    engine = after_u;
    if (rc == DDDMR_OK) {
      rows_.clear();
      drawNoiseRows(engine, mean, sigma, st.n_duplicates, rows_);      // exactly 6 * n_duplicates normal draws
    }
    return rc;
  }
  // pf_->noise(sigma): one row per particle
  template<class Engine>
  int addNoise(Engine & engine, const float mean[6], const float sigma[6])
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    rows_.clear();
    drawNoiseRows(engine, mean, sigma, n_, rows_);
    return dddmr_rollout_mcl_filter_add_noise(ctx_, rows_.data(), n_);
  }

private:
  template<class State>
  static void pose7(const State & s, float out[7])
  {
    out[0] = s.pos_.x_; out[1] = s.pos_.y_; out[2] = s.pos_.z_;
    out[3] = s.rot_.x_; out[4] = s.rot_.y_; out[5] = s.rot_.z_; out[6] = s.rot_.w_;
  }
  dddmr_rollout_ctx * ctx_ = nullptr;
  size_t n_ = 0;
  std::vector<float> rows_, noise4_;
};

}  // namespace dddmr_rollout_adapter
#endif
