// mcl_filter_host_step.cpp -- the HOST filter step that tools/mcl_filter_bench.py times the device's against: this tool's
// own C++ restatement of what mcl_3dl's pf.h / state_6dof.h / motion model do per step in serial loops (predict; after
// the measure: normalise, bias, expectationBiased, max, covariance(1.0, 1.0), resample with a std::sort of the copied
// particles, update_noise_func).  It is NOT the reference's code and is not held to it on bits; it exists to give the
// parent's route (likelihoods down, host loops, states up) an honest host cost.  Built by the tool with g++ -O2.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Q { float x, y, z, w; };
inline Q qmul(Q a, Q b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
          a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
inline Q qnorm(Q q) {
  const float s = (float)(1.0 / std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w));
  return {q.x * s, q.y * s, q.z * s, q.w * s};
}
inline Q qinv(Q q) {
  const float s = (float)(1.0 / (q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w));
  return {-q.x * s, -q.y * s, -q.z * s, q.w * s};
}
inline void qrot(Q q, const float v[3], float out[3]) {
  const Q r = qmul(qmul(q, Q{v[0], v[1], v[2], 0.f}), Q{-q.x, -q.y, -q.z, q.w});
  out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
inline float axis_angle(Q q) {
  if (std::fabs(q.w) >= 1.0 - 0.000001) return 0.f;
  float a = std::acos(q.w) * 2.0;
  if (a > M_PI) a -= 2.0 * M_PI;
  return a;
}
struct Particle {
  float s[13], nz[4], p, bias, accum;
  bool operator<(const Particle& o) const { return accum < o.accum; }
};

}  // namespace

extern "C" {

// states [n][13], noise4 [n][4] in place
void host_predict(size_t n, float* states, const float* noise4, const float* odom_prev, const float* odom_cur, float dt, float lin_tc,
                  float ang_tc) {
  const Q inv = qinv(Q{odom_prev[3], odom_prev[4], odom_prev[5], odom_prev[6]});
  const float d[3] = {odom_cur[0] - odom_prev[0], odom_cur[1] - odom_prev[1], odom_cur[2] - odom_prev[2]};
  float rt[3];
  qrot(inv, d, rt);
  const Q rq = qmul(inv, Q{odom_cur[3], odom_cur[4], odom_cur[5], odom_cur[6]});
  const float ang = axis_angle(rq), norm = std::sqrt(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2]);
  const float dl = 1.0 - dt / lin_tc, da = 1.0 - dt / ang_tc;
  for (size_t i = 0; i < n; ++i) {
    float* s = states + 13 * i;
    const float* z = noise4 + 4 * i;
    const float k = 1.0 + z[0];
    const float diff[3] = {rt[0] * k + z[2] * ang, rt[1] * k, rt[2] * k};
    const Q rot{s[3], s[4], s[5], s[6]};
    float mv[3];
    qrot(rot, diff, mv);
    for (int c = 0; c < 3; ++c) { s[7 + c] += diff[c] - rt[c]; s[c] += mv[c]; }
    const float yaw = z[1] * norm + z[3] * ang;
    const Q r = qnorm(qmul(qmul(qnorm(Q{0.f, 0.f, std::sin(yaw / 2), std::cos(yaw / 2)}), rot), rq));
    s[3] = r.x; s[4] = r.y; s[5] = r.z; s[6] = r.w;
    s[12] += yaw;
    for (int c = 0; c < 3; ++c) { s[7 + c] *= dl; s[10 + c] *= da; }
  }
}

// After the measure: everything MCL3dlNode::measure and cbOdom do with the particles.  states / noise4 / prob in place;
// rows [n][10]; est_out: mean_biased [7], cov [36]; returns the number of duplicates.
uint32_t host_update(size_t n, float* states, float* noise4, float* prob, const float* lik, const float* state_prev, float var_dist,
                     float var_ang, float u, const float* rows, const float* noise4_new, float* est_out) {
  std::vector<Particle> ps(n);
  float sum = 0;
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(ps[i].s, states + 13 * i, sizeof(ps[i].s));
    std::memcpy(ps[i].nz, noise4 + 4 * i, sizeof(ps[i].nz));
    ps[i].p = prob[i] * lik[i];
    sum += ps[i].p;
  }
  if (sum > 0) for (auto& p : ps) p.p /= sum;
  else for (size_t i = 0; i < n; ++i) ps[i].p = prob[i];
  // bias
  const float a_l = 1.0 / std::sqrt(2.0 * M_PI * var_dist * var_dist), q_l = var_dist * var_dist * 2.0;
  const float a_a = 1.0 / std::sqrt(2.0 * M_PI * var_ang * var_ang), q_a = var_ang * var_ang * 2.0;
  const Q pinv = qinv(Q{state_prev[3], state_prev[4], state_prev[5], state_prev[6]});
  for (auto& p : ps) {
    const float dx = p.s[0] - state_prev[0], dy = p.s[1] - state_prev[1], dz = p.s[2] - state_prev[2];
    const float lin = std::sqrt(dx * dx + dy * dy + dz * dz);
    const float ang = axis_angle(qmul(Q{p.s[3], p.s[4], p.s[5], p.s[6]}, pinv));
    p.bias = a_l * expf(-lin * lin / q_l) * a_a * expf(-ang * ang / q_a) + 1e-6;
  }
  // the two means
  const float fx[3] = {1, 0, 0}, uz[3] = {0, 0, 1};
  auto mean = [&](bool biased, float limit, float out[7], float* p_sum_out) {
    float ps_ = 0, e[3] = {0, 0, 0}, f[3] = {0, 0, 0}, up[3] = {0, 0, 0};
    for (auto& p : ps) {
      const float w = biased ? p.p * p.bias : p.p;
      ps_ += w;
      float a[3], b[3];
      const Q r{p.s[3], p.s[4], p.s[5], p.s[6]};
      qrot(r, fx, a); qrot(r, uz, b);
      for (int c = 0; c < 3; ++c) { e[c] += p.s[c] * w; f[c] += a[c] * w; up[c] += b[c] * w; }
      if (!biased && ps_ > limit) break;
    }
    auto nrm = [](float v[3]) { const float n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] /= n; v[1] /= n; v[2] /= n; };
    float xv[3] = {f[0], f[1], f[2]};
    nrm(xv);
    float yv[3] = {up[1] * xv[2] - up[2] * xv[1], up[2] * xv[0] - up[0] * xv[2], up[0] * xv[1] - up[1] * xv[0]};
    nrm(yv);
    float zv[3] = {xv[1] * yv[2] - xv[2] * yv[1], xv[2] * yv[0] - xv[0] * yv[2], xv[0] * yv[1] - xv[1] * yv[0]};
    nrm(zv);
    out[0] = e[0] / ps_; out[1] = e[1] / ps_; out[2] = e[2] / ps_;
    out[6] = std::sqrt(std::max(0.0, 1.0 + xv[0] + yv[1] + zv[2])) / 2.0;
    out[3] = std::sqrt(std::max(0.0, 1.0 + xv[0] - yv[1] - zv[2])) / 2.0;
    out[4] = std::sqrt(std::max(0.0, 1.0 - xv[0] + yv[1] - zv[2])) / 2.0;
    out[5] = std::sqrt(std::max(0.0, 1.0 - xv[0] - yv[1] + zv[2])) / 2.0;
    if (zv[1] - yv[2] > 0) out[3] = -out[3];
    if (xv[2] - zv[0] > 0) out[4] = -out[4];
    if (yv[0] - xv[1] > 0) out[5] = -out[5];
    *p_sum_out = ps_;
  };
  float tmp, e[7];
  mean(true, 0, est_out, &tmp);
  const Particle* best = &ps[0];
  for (auto& p : ps) if (best->p < p.p) best = &p;
  est_out[43] = best->s[0];
  mean(false, 1.0f, e, &tmp);
  float p_sum = 0;
  size_t p_num = 0;
  for (auto& p : ps) { ++p_num; p_sum += p.p; if (p_sum > 1.0f) break; }
  float cov[6][6] = {};
  p_sum = 0;
  for (size_t i = 0; i < p_num; ++i) {
    p_sum += ps[i].p;
    for (int j = 0; j < 6; ++j)
      for (int k = j; k < 6; ++k) cov[k][j] = cov[j][k] += (ps[i].s[k] - e[k]) * (ps[i].s[j] - e[j]) * ps[i].p;
  }
  for (int j = 0; j < 6; ++j)
    for (int k = 0; k < 6; ++k) est_out[7 + 6 * j + k] = cov[j][k] / p_sum;
  // resample
  float accum = 0;
  for (auto& p : ps) { accum += p.p; p.accum = accum; }
  std::vector<Particle> dup = ps;
  std::sort(dup.begin(), dup.end());
  const float pstep = accum / n, initial_p = u * pstep, np = 1.0 / n;
  auto it = dup.begin(), it_prev = dup.begin();
  uint32_t n_dup = 0;
  for (size_t i = 0; i < n; ++i) {
    Particle key;
    key.accum = pstep * i + initial_p;
    it = std::lower_bound(it, dup.end(), key);
    float* s = states + 13 * i;
    prob[i] = np;
    if (it == dup.end()) {
      std::memcpy(s, it_prev->s, sizeof(it_prev->s));
      continue;
    }
    if (it == it_prev) {
      const float* z = rows + 10 * (size_t)n_dup++;
      for (int c = 0; c < 3; ++c) { s[c] = it->s[c] + z[c]; s[7 + c] = it->s[7 + c] + z[c]; s[10 + c] = it->s[10 + c] + z[7 + c]; }
      const Q r = qnorm(qmul(Q{z[3], z[4], z[5], z[6]}, Q{it->s[3], it->s[4], it->s[5], it->s[6]}));
      s[3] = r.x; s[4] = r.y; s[5] = r.z; s[6] = r.w;
    } else {
      std::memcpy(s, it->s, sizeof(it->s));
    }
    it_prev = it;
  }
  std::memcpy(noise4, noise4_new, n * 4 * sizeof(float));      // update_noise_func
  return n_dup;
}

}  // extern "C"
