// mcl_filter_plan.hip.h -- the parts of mcl_3dl's filter step that are host arithmetic alone (citations relative to the
// reference's src/dddmr_mcl_3dl/):
//   MotionPredictionModelDifferentialDrive::setOdoms   include/mcl_3dl/motion_prediction_models/..._differential_drive.h:46-54
//   Quat::inv / operator* / getAxisAng                 include/mcl_3dl/quat.h:131-143,187-190,226-239
//   NormalLikelihood's constants                       include/mcl_3dl/nd.h:45-49
//   Quat(forward, up_raw)                              include/mcl_3dl/quat.h:59-75   (also called by k_filter_reduce)
//   ParticleWeightedMeanQuat::getMean                  include/mcl_3dl/state_6dof.h:317-322
// No HIP call and no HIP type, so that tests/cpp/mcl_filter_plan_test.cpp builds it with a plain host compiler;
// mcl_filter.hip.h calls the same functions.  Float where the reference is float, double where it is double.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define DDDMR_FILTER_HD __host__ __device__
#else
#define DDDMR_FILTER_HD
#endif

namespace dddmr {

// what predict() reads of setOdoms' members, and the two decay factors of :65-66
struct FilterOdom {
  float rt[3];                 // relative_translation_
  float rq[4];                 // relative_quat_ (x y z w)
  float rt_norm;               // relative_translation_norm_
  float rel_ang;               // relative_angle_
  float decay_lin, decay_ang;  // float(1.0 - time_diff_ / odom_err_integ_*_tc_): a float quotient, a double difference
};

// what the bias lambda (src/mcl_3dl.cpp:518-530) reads that does not depend on the particle
struct FilterBias {
  uint32_t has_prev;           // 0: p_bias = 1.0 (:510-514)
  float prev_pos[3];
  float prev_inv[4];           // state_prev_.rot_.inv()
  float a_lin, sq2_lin, a_ang, sq2_ang;
};

// Quat::operator*(const Quat&), every sum left to right
DDDMR_FILTER_HD inline void filter_qmul(const float a[4], const float b[4], float out[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const float y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const float z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  const float w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  out[0] = x; out[1] = y; out[2] = z; out[3] = w;
}

// Quat::inv(): conj() / dot(*this), and operator/(s) is operator*(float(1.0 / s))
inline void filter_qinv(const float q[4], float out[4]) {
  const float dot = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const float s = (float)(1.0 / (double)dot);
  out[0] = -q[0] * s; out[1] = -q[1] * s; out[2] = -q[2] * s; out[3] = q[3] * s;
}

// Quat::operator*(const Vec3&): *this * Quat(v, 0) * conj()
inline void filter_qrot(const float q[4], const float v[3], float out[3]) {
  const float p[4] = {v[0], v[1], v[2], 0.0f}, c[4] = {-q[0], -q[1], -q[2], q[3]};
  float a[4], b[4];
  filter_qmul(q, p, a);
  filter_qmul(a, c, b);
  out[0] = b[0]; out[1] = b[1]; out[2] = b[2];
}

// Quat::getAxisAng's angle (the axis is not used by the filter)
inline float filter_axis_angle(const float q[4]) {
  if (fabs((double)q[3]) >= 1.0 - 0.000001) return 0.0f;
  float ang = (float)((double)acosf(q[3]) * 2.0);
  if ((double)ang > M_PI) ang = (float)((double)ang - 2.0 * M_PI);
  return ang;
}

// setOdoms; odom_prev / odom_cur: pos xyz, rot xyzw
inline FilterOdom filter_set_odoms(const float odom_prev[7], const float odom_cur[7], float time_diff, float lin_tc, float ang_tc) {
  FilterOdom o;
  float inv[4];
  filter_qinv(odom_prev + 3, inv);
  const float d[3] = {odom_cur[0] - odom_prev[0], odom_cur[1] - odom_prev[1], odom_cur[2] - odom_prev[2]};
  filter_qrot(inv, d, o.rt);
  filter_qmul(inv, odom_cur + 3, o.rq);
  o.rel_ang = filter_axis_angle(o.rq);
  o.rt_norm = sqrtf(o.rt[0] * o.rt[0] + o.rt[1] * o.rt[1] + o.rt[2] * o.rt[2]);
  o.decay_lin = (float)(1.0 - (double)(time_diff / lin_tc));
  o.decay_ang = (float)(1.0 - (double)(time_diff / ang_tc));
  return o;
}

// NormalLikelihood<float>(sigma): a_ and sq2_
inline void filter_normal_likelihood(float sigma, float* a, float* sq2) {
  *a = (float)(1.0 / sqrt(2.0 * M_PI * (double)sigma * (double)sigma));
  *sq2 = (float)((double)(sigma * sigma) * 2.0);
}

inline FilterBias filter_bias_plan(const float* state_prev /* [7] or null */, float bias_var_dist, float bias_var_ang) {
  FilterBias b{};
  if (!state_prev) return b;
  b.has_prev = 1;
  for (int i = 0; i < 3; ++i) b.prev_pos[i] = state_prev[i];
  filter_qinv(state_prev + 3, b.prev_inv);
  filter_normal_likelihood(bias_var_dist, &b.a_lin, &b.sq2_lin);
  filter_normal_likelihood(bias_var_ang, &b.a_ang, &b.sq2_ang);
  return b;
}

// Vec3::normalized(): every component divided by sqrtf(x*x + y*y + z*z)
DDDMR_FILTER_HD inline void filter_normalized3(const float v[3], float out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  out[0] = v[0] / n; out[1] = v[1] / n; out[2] = v[2] / n;
}
DDDMR_FILTER_HD inline void filter_cross3(const float a[3], const float b[3], float out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  out[0] = x; out[1] = y; out[2] = z;
}
DDDMR_FILTER_HD inline float filter_half_root(double v) { return (float)(sqrt(v > 0.0 ? v : 0.0) / 2.0); }

// Quat(forward, up_raw)
DDDMR_FILTER_HD inline void filter_quat_from_axes(const float forward[3], const float up_raw[3], float q[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float xv[3], yv[3], zv[3], c[3];
  filter_normalized3(forward, xv);
  filter_cross3(up_raw, xv, c);
  filter_normalized3(c, yv);
  filter_cross3(xv, yv, c);
  filter_normalized3(c, zv);
  q[3] = filter_half_root(1.0 + xv[0] + yv[1] + zv[2]);
  q[0] = filter_half_root(1.0 + xv[0] - yv[1] - zv[2]);
  q[1] = filter_half_root(1.0 - xv[0] + yv[1] - zv[2]);
  q[2] = filter_half_root(1.0 - xv[0] - yv[1] + zv[2]);
  if (zv[1] - yv[2] > 0) q[0] = -q[0];
  if (xv[2] - zv[0] > 0) q[1] = -q[1];
  if (yv[0] - xv[1] > 0) q[2] = -q[2];
}

// ParticleWeightedMeanQuat::getMean from its ten sums: p_sum, e_.pos_, front_sum_, up_sum_ -> pos xyz, rot xyzw
DDDMR_FILTER_HD inline void filter_mean_from_sums(const float sums[10], float mean[7]) {
  mean[0] = sums[1] / sums[0]; mean[1] = sums[2] / sums[0]; mean[2] = sums[3] / sums[0];
  filter_quat_from_axes(sums + 4, sums + 7, mean + 3);
}

}  // namespace dddmr
