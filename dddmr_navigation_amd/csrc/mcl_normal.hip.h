// mcl_normal.hip.h -- pcl::NormalEstimation's per-point arithmetic, shared by the localiser's observation
// (mcl_observation.hip.h: 5 neighbours of a less-sharp point, in LDS) and the sub-maps' ground normals
// (mcl_submap.hip.h: normal_k neighbours of a ground point, in device memory).  DESIGN 4e numbers the assumptions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace dddmr {

// pcl::computeRoots2 / computeRoots of a symmetric 3x3 float matrix (m: 00 01 02 11 12 22), roots ascending
__device__ inline void mclobs_roots2(float b, float c, float* r) {
  r[0] = 0.0f;
  float d = b * b - 4.0f * c;
  if (d < 0.0f) d = 0.0f;
  const float sd = sqrtf(d);
  r[2] = 0.5f * (b + sd);
  r[1] = 0.5f * (b - sd);
}
__device__ inline void mclobs_roots(const float* m, float* r) {
  const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[3], m12 = m[4], m22 = m[5];
  const float c0 = m00 * m11 * m22 + 2.0f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
  const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
  const float c2 = m00 + m11 + m22;
  if (fabsf(c0) < 1.1920929e-07f) {                // Eigen::NumTraits<float>::epsilon()
    mclobs_roots2(c2, c1, r);
    return;
  }
  const float s_inv3 = (float)(1.0 / 3.0), s_sqrt3 = sqrtf(3.0f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0f) a_over_3 = 0.0f;
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0f) q = 0.0f;
  const float rho = sqrtf(-a_over_3);
  const float theta = atan2f(sqrtf(-q), half_b) * s_inv3;
  const float cos_theta = cosf(theta), sin_theta = sinf(theta);
  r[0] = c2_over_3 + 2.0f * rho * cos_theta;
  r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  float t;
  if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  if (r[1] >= r[2]) {
    t = r[1]; r[1] = r[2]; r[2] = t;
    if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  }
  if (r[0] <= 0.0f) mclobs_roots2(c2, c1, r);      // (a positive semi-definite matrix has no negative eigenvalue)
}

// NormalEstimation::computePointNormal over the k neighbours nb[0 .. k) of the point p (assumptions N1-N7):
// mean and covariance about the first neighbour, pcl::eigen33's eigenvector of the smallest eigenvalue, flipped toward
// the origin.  NaN for fewer than 3 neighbours and for a zero cross product.
__device__ inline float3 mclobs_normal(const float4* P, const uint32_t* nb, uint32_t k, float4 p) {
  const float nan = __int_as_float(0x7FC00000);
  if (k < 3) return make_float3(nan, nan, nan);
  const float4 K = P[nb[0]];
  float a[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (uint32_t q = 0; q < k; ++q) {
    const float4 g = P[nb[q]];
    const float x = g.x - K.x, y = g.y - K.y, z = g.z - K.z;
    a[0] += x * x; a[1] += x * y; a[2] += x * z; a[3] += y * y; a[4] += y * z; a[5] += z * z;
    a[6] += x; a[7] += y; a[8] += z;
  }
  const float cnt = (float)k;
  for (int q = 0; q < 9; ++q) a[q] /= cnt;
  float m[6] = {a[0] - a[6] * a[6], a[1] - a[6] * a[7], a[2] - a[6] * a[8], a[3] - a[7] * a[7], a[4] - a[7] * a[8], a[5] - a[8] * a[8]};
  float scale = 0.0f;
  for (int q = 0; q < 6; ++q) scale = fmaxf(scale, fabsf(m[q]));     // (a NaN entry: the roots and the normal are NaN anyway)
  if (scale <= 1.17549435e-38f) scale = 1.0f;                          // std::numeric_limits<float>::min()
  for (int q = 0; q < 6; ++q) m[q] = m[q] / scale;
  float r[3];
  mclobs_roots(m, r);
  const float d0 = m[0] - r[0], d1 = m[3] - r[0], d2 = m[5] - r[0];
  const float r0[3] = {d0, m[1], m[2]}, r1[3] = {m[1], d1, m[4]}, r2[3] = {m[2], m[4], d2};
  float c[3][3], len[3];
  const float* ra[3] = {r0, r0, r1};
  const float* rb[3] = {r1, r2, r2};
  for (int q = 0; q < 3; ++q) {
    const float* u = ra[q];
    const float* v = rb[q];
    c[q][0] = u[1] * v[2] - u[2] * v[1];
    c[q][1] = u[2] * v[0] - u[0] * v[2];
    c[q][2] = u[0] * v[1] - u[1] * v[0];
    len[q] = sqrtf(c[q][0] * c[q][0] + c[q][1] * c[q][1] + c[q][2] * c[q][2]);
  }
  int best = 0;                                                         // maxCoeff(&index): the first of equal maxima
  if (len[1] > len[best]) best = 1;
  if (len[2] > len[best]) best = 2;
  float nx = c[best][0] / len[best], ny = c[best][1] / len[best], nz = c[best][2] / len[best];
  const float vx = 0.0f - p.x, vy = 0.0f - p.y, vz = 0.0f - p.z;       // flipNormalTowardsViewpoint, viewpoint (0, 0, 0)
  const float cos_theta = vx * nx + vy * ny + vz * nz;
  if (cos_theta < 0.0f) { nx *= -1.0f; ny *= -1.0f; nz *= -1.0f; }
  return make_float3(nx, ny, nz);
}

}  // namespace dddmr
