// Functional stand-in for the tf2 / tf2_eigen surface of the reference's rollout units.  Written from the libraries'
// documented behaviour; it includes and calls nothing under oracle/.
#ifndef REF_SHIM_TF2_HPP_
#define REF_SHIM_TF2_HPP_
// tf2/LinearMath/Scalar.h includes <math.h>.  With libstdc++ that header also declares the float (and long double)
// overloads of sqrt / fabs / cos / sin / hypot ... in the global namespace, so an unqualified call on a float argument
// in the reference resolves to the float overload (oracle/ASSUMPTIONS.md row 18).  The ref-math-variant build puts
// shim_nomath/ first on the include path, whose math.h withholds those overloads.
#include <math.h>
#include "ref_eigen.hpp"
#include "ref_ros.hpp"

namespace tf2 {
typedef double tf2Scalar;
inline tf2Scalar tf2Asin(tf2Scalar x) {
  if (x < tf2Scalar(-1)) x = tf2Scalar(-1);
  if (x > tf2Scalar(1)) x = tf2Scalar(1);
  return std::asin(x);
}

class Quaternion {
 public:
  Quaternion() = default;
  Quaternion(tf2Scalar x, tf2Scalar y, tf2Scalar z, tf2Scalar w) : q_{x, y, z, w} {}
  tf2Scalar x() const { return q_[0]; }
  tf2Scalar y() const { return q_[1]; }
  tf2Scalar z() const { return q_[2]; }
  tf2Scalar w() const { return q_[3]; }
  // Quaternion::length2 = dot(*this, *this), summed x, y, z, w left to right (row 13)
  tf2Scalar length2() const { return q_[0] * q_[0] + q_[1] * q_[1] + q_[2] * q_[2] + q_[3] * q_[3]; }

 private:
  tf2Scalar q_[4] = {0, 0, 0, 1};
};

class Matrix3x3 {
 public:
  // Matrix3x3(q) -> setRotation(q): s = 2 / |q|^2 (row 13)
  explicit Matrix3x3(const Quaternion& q) {
    const tf2Scalar d = q.length2();
    const tf2Scalar s = tf2Scalar(2.0) / d;
    const tf2Scalar xs = q.x() * s, ys = q.y() * s, zs = q.z() * s;
    const tf2Scalar wx = q.w() * xs, wy = q.w() * ys, wz = q.w() * zs;
    const tf2Scalar xx = q.x() * xs, xy = q.x() * ys, xz = q.x() * zs;
    const tf2Scalar yy = q.y() * ys, yz = q.y() * zs, zz = q.z() * zs;
    const tf2Scalar v[9] = {tf2Scalar(1.0) - (yy + zz), xy - wz, xz + wy,
                            xy + wz, tf2Scalar(1.0) - (xx + zz), yz - wx,
                            xz - wy, yz + wx, tf2Scalar(1.0) - (xx + yy)};
    for (int i = 0; i < 9; ++i) m_[i / 3][i % 3] = v[i];
  }
  // getEulerYPR, solution 1: pitch = -asin(m20), yaw = atan2(m10 / cos pitch, m00 / cos pitch); gimbal lock
  // (|m20| >= 1): yaw = 0, pitch = +-pi/2, roll from atan2(m21, m22) (row 13)
  void getEulerYPR(tf2Scalar& yaw, tf2Scalar& pitch, tf2Scalar& roll, unsigned int = 1) const {
    if (std::fabs(m_[2][0]) >= 1) {
      yaw = 0;
      const tf2Scalar delta = std::atan2(m_[2][1], m_[2][2]);
      if (m_[2][0] < 0) {
        pitch = M_PI / tf2Scalar(2.0);
        roll = pitch + delta;
      } else {
        pitch = -M_PI / tf2Scalar(2.0);
        roll = -pitch + delta;
      }
    } else {
      pitch = -tf2Asin(m_[2][0]);
      roll = std::atan2(m_[2][1] / std::cos(pitch), m_[2][2] / std::cos(pitch));
      yaw = std::atan2(m_[1][0] / std::cos(pitch), m_[0][0] / std::cos(pitch));
    }
  }

 private:
  tf2Scalar m_[3][3];
};

// tf2_geometry_msgs fromMsg: a plain copy of x, y, z, w
inline void convert(const geometry_msgs::msg::Quaternion& in, Quaternion& out) { out = Quaternion(in.x, in.y, in.z, in.w); }

// tf2_eigen (row 16): transformToEigen = Translation3d(t) * Quaterniond(w, x, y, z); eigenToTransform copies the
// translation and Quaterniond(T.linear()) (the upper 3x3 taken as orthonormal)
inline Eigen::Isometry3d transformToEigen(const geometry_msgs::msg::Transform& t) {
  return Eigen::Translation3d(t.translation.x, t.translation.y, t.translation.z) *
         Eigen::Quaterniond(t.rotation.w, t.rotation.x, t.rotation.y, t.rotation.z);
}
inline Eigen::Isometry3d transformToEigen(const geometry_msgs::msg::TransformStamped& t) {
  return transformToEigen(t.transform);
}
inline geometry_msgs::msg::TransformStamped eigenToTransform(const Eigen::Affine3d& T) {
  geometry_msgs::msg::TransformStamped t;
  t.transform.translation.x = T.translation().x();
  t.transform.translation.y = T.translation().y();
  t.transform.translation.z = T.translation().z();
  const Eigen::Quaterniond q(T.linear());
  t.transform.rotation.x = q.x();
  t.transform.rotation.y = q.y();
  t.transform.rotation.z = q.z();
  t.transform.rotation.w = q.w();
  return t;
}
}  // namespace tf2
#endif
