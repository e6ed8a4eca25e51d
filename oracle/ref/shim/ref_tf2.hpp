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

// tf2::Vector3 (row 14): three doubles; dot sums x, y, z left to right, cross is the closed form, length = sqrt(dot),
// normalized() returns *this / length() and leaves *this alone
class Vector3 {
 public:
  Vector3() = default;
  Vector3(const tf2Scalar& x, const tf2Scalar& y, const tf2Scalar& z) : v_{x, y, z} {}
  const tf2Scalar& x() const { return v_[0]; }
  const tf2Scalar& y() const { return v_[1]; }
  const tf2Scalar& z() const { return v_[2]; }
  tf2Scalar dot(const Vector3& o) const { return v_[0] * o.v_[0] + v_[1] * o.v_[1] + v_[2] * o.v_[2]; }
  tf2Scalar length2() const { return dot(*this); }
  tf2Scalar length() const { return std::sqrt(length2()); }
  Vector3 cross(const Vector3& o) const {
    return Vector3(v_[1] * o.v_[2] - v_[2] * o.v_[1], v_[2] * o.v_[0] - v_[0] * o.v_[2], v_[0] * o.v_[1] - v_[1] * o.v_[0]);
  }
  Vector3 normalized() const {
    const tf2Scalar s = tf2Scalar(1.0) / length();
    return Vector3(v_[0] * s, v_[1] * s, v_[2] * s);
  }

 private:
  tf2Scalar v_[3] = {0, 0, 0};
};

class Quaternion {
 public:
  Quaternion() = default;
  Quaternion(tf2Scalar x, tf2Scalar y, tf2Scalar z, tf2Scalar w) : q_{x, y, z, w} {}
  // Quaternion(axis, angle) -> setRotation (row 14): s = sin(angle / 2) / |axis|, a zero axis gives NaN or inf
  Quaternion(const Vector3& axis, const tf2Scalar& angle) {
    const tf2Scalar d = axis.length();
    const tf2Scalar s = std::sin(angle * tf2Scalar(0.5)) / d;
    q_[0] = axis.x() * s;
    q_[1] = axis.y() * s;
    q_[2] = axis.z() * s;
    q_[3] = std::cos(angle * tf2Scalar(0.5));
  }
  tf2Scalar length() const { return std::sqrt(length2()); }
  // normalize = operator/=(length()) = operator*=(1 / length()) (row 14)
  Quaternion& normalize() {
    const tf2Scalar s = tf2Scalar(1.0) / length();
    q_[0] *= s; q_[1] *= s; q_[2] *= s; q_[3] *= s;
    return *this;
  }
  tf2Scalar x() const { return q_[0]; }
  tf2Scalar y() const { return q_[1]; }
  tf2Scalar z() const { return q_[2]; }
  tf2Scalar w() const { return q_[3]; }
  // Quaternion::length2 = dot(*this, *this), summed x, y, z, w left to right (row 13)
  tf2Scalar length2() const { return q_[0] * q_[0] + q_[1] * q_[1] + q_[2] * q_[2] + q_[3] * q_[3]; }

 private:
  tf2Scalar q_[4] = {0, 0, 0, 1};
};

// the Hamilton product, every component's four terms summed left to right (row 14)
inline Quaternion operator*(const Quaternion& a, const Quaternion& b) {
  return Quaternion(a.w() * b.x() + a.x() * b.w() + a.y() * b.z() - a.z() * b.y(),
                    a.w() * b.y() + a.y() * b.w() + a.z() * b.x() - a.x() * b.z(),
                    a.w() * b.z() + a.z() * b.w() + a.x() * b.y() - a.y() * b.x(),
                    a.w() * b.w() - a.x() * b.x() - a.y() * b.y() - a.z() * b.z());
}

class Matrix3x3 {
 public:
  // getRPY = getEulerYPR with the arguments in the other order (row 13)
  void getRPY(tf2Scalar& roll, tf2Scalar& pitch, tf2Scalar& yaw, unsigned int solution_number = 1) const {
    getEulerYPR(yaw, pitch, roll, solution_number);
  }
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
  // (|m20| >= 1): yaw = 0, pitch = +-pi/2, roll = atan2(m21, m22) (row 13: tf2 takes the bare difference angle
  // where Bullet's btMatrix3x3 adds the pitch to it)
  void getEulerYPR(tf2Scalar& yaw, tf2Scalar& pitch, tf2Scalar& roll, unsigned int = 1) const {
    if (std::fabs(m_[2][0]) >= 1) {
      yaw = 0;
      const tf2Scalar delta = std::atan2(m_[2][1], m_[2][2]);
      if (m_[2][0] < 0) {
        pitch = M_PI / tf2Scalar(2.0);
        roll = delta;
      } else {
        pitch = -M_PI / tf2Scalar(2.0);
        roll = delta;
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
