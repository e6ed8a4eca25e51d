// Functional stand-in for the part of Eigen the reference's rollout units use: Vector3f / Vector3d, Matrix3d,
// AngleAxisd, Quaterniond, Translation3d and Affine3d (= Isometry3d here: only rigid transforms occur).
// Written from Eigen's documented closed forms (Eigen/src/Geometry); it includes and calls nothing under oracle/.
// Every 3-term sum is evaluated left to right in double: oracle/ASSUMPTIONS.md row 12.
#ifndef REF_SHIM_EIGEN_HPP_
#define REF_SHIM_EIGEN_HPP_
#include <cmath>

namespace Eigen {
template <class S> struct Vec3 {
  S v[3] = {S(0), S(0), S(0)};  // Eigen leaves a fresh vector uninitialised; zero keeps unread lanes deterministic
  S& operator[](int i) { return v[i]; }
  const S& operator[](int i) const { return v[i]; }
  S& operator()(int i) { return v[i]; }
  const S& operator()(int i) const { return v[i]; }
  S& x() { return v[0]; }
  S& y() { return v[1]; }
  S& z() { return v[2]; }
  const S& x() const { return v[0]; }
  const S& y() const { return v[1]; }
  const S& z() const { return v[2]; }
  static Vec3 Zero() { return Vec3(); }
  static Vec3 UnitZ() { Vec3 r; r.v[2] = S(1); return r; }
};
using Vector3f = Vec3<float>;
using Vector3d = Vec3<double>;

struct Matrix3d {
  double m[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  double& operator()(int r, int c) { return m[r][c]; }
  double operator()(int r, int c) const { return m[r][c]; }
};
// Row 12: (A*B)(i,j) = (A(i,0)*B(0,j) + A(i,1)*B(1,j)) + A(i,2)*B(2,j)
inline Matrix3d operator*(const Matrix3d& a, const Matrix3d& b) {
  Matrix3d r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
  return r;
}
inline Vector3d operator*(const Matrix3d& a, const Vector3d& b) {
  Vector3d r;
  for (int i = 0; i < 3; ++i) r.v[i] = a.m[i][0] * b.v[0] + a.m[i][1] * b.v[1] + a.m[i][2] * b.v[2];
  return r;
}

// Row 12: AngleAxis::toRotationMatrix (Eigen/src/Geometry/AngleAxis.h), evaluated for a general unit axis.
struct AngleAxisd {
  double angle;
  Vector3d axis;
  AngleAxisd(double a, const Vector3d& ax) : angle(a), axis(ax) {}
  Matrix3d toRotationMatrix() const {
    Matrix3d res;
    const double s = std::sin(angle), c = std::cos(angle);
    const Vector3d sin_axis{{s * axis.v[0], s * axis.v[1], s * axis.v[2]}};
    const Vector3d cos1_axis{{(1.0 - c) * axis.v[0], (1.0 - c) * axis.v[1], (1.0 - c) * axis.v[2]}};
    double tmp;
    tmp = cos1_axis.v[0] * axis.v[1];
    res.m[0][1] = tmp - sin_axis.v[2];
    res.m[1][0] = tmp + sin_axis.v[2];
    tmp = cos1_axis.v[0] * axis.v[2];
    res.m[0][2] = tmp + sin_axis.v[1];
    res.m[2][0] = tmp - sin_axis.v[1];
    tmp = cos1_axis.v[1] * axis.v[2];
    res.m[1][2] = tmp - sin_axis.v[0];
    res.m[2][1] = tmp + sin_axis.v[0];
    for (int i = 0; i < 3; ++i) res.m[i][i] = cos1_axis.v[i] * axis.v[i] + c;
    return res;
  }
};

// Row 12: Quaternion(w, x, y, z); toRotationMatrix (no normalisation) and the constructor from a rotation matrix
// (quaternionbase_assign_selector: trace branch, else the largest diagonal element i, j = i+1, k = j+1 mod 3).
struct Quaterniond {
  double qx = 0.0, qy = 0.0, qz = 0.0, qw = 1.0;
  Quaterniond(double w, double x, double y, double z) : qx(x), qy(y), qz(z), qw(w) {}
  explicit Quaterniond(const Matrix3d& mat) {
    double q[3];
    const double t = mat.m[0][0] + mat.m[1][1] + mat.m[2][2];
    if (t > 0.0) {
      double tt = std::sqrt(t + 1.0);
      qw = 0.5 * tt;
      tt = 0.5 / tt;
      qx = (mat.m[2][1] - mat.m[1][2]) * tt;
      qy = (mat.m[0][2] - mat.m[2][0]) * tt;
      qz = (mat.m[1][0] - mat.m[0][1]) * tt;
    } else {
      int i = 0;
      if (mat.m[1][1] > mat.m[0][0]) i = 1;
      if (mat.m[2][2] > mat.m[i][i]) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      double tt = std::sqrt(mat.m[i][i] - mat.m[j][j] - mat.m[k][k] + 1.0);
      q[i] = 0.5 * tt;
      tt = 0.5 / tt;
      qw = (mat.m[k][j] - mat.m[j][k]) * tt;
      q[j] = (mat.m[j][i] + mat.m[i][j]) * tt;
      q[k] = (mat.m[k][i] + mat.m[i][k]) * tt;
      qx = q[0]; qy = q[1]; qz = q[2];
    }
  }
  double x() const { return qx; }
  double y() const { return qy; }
  double z() const { return qz; }
  double w() const { return qw; }
  Matrix3d toRotationMatrix() const {
    Matrix3d r;
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
    const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
    const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    r.m[0][0] = 1.0 - (tyy + tzz); r.m[0][1] = txy - twz; r.m[0][2] = txz + twy;
    r.m[1][0] = txy + twz; r.m[1][1] = 1.0 - (txx + tzz); r.m[1][2] = tyz - twx;
    r.m[2][0] = txz - twy; r.m[2][1] = tyz + twx; r.m[2][2] = 1.0 - (txx + tyy);
    return r;
  }
};

struct Translation3d {
  double t[3];
  Translation3d(double x, double y, double z) : t{x, y, z} {}
};

class Affine3d {
 public:
  Affine3d() { for (int i = 0; i < 3; ++i) L_.m[i][i] = 1.0; }  // Eigen leaves it uninitialised; never read so
  // Transform(const RotationBase&): linear = R, translation = 0
  explicit Affine3d(const AngleAxisd& r) : L_(r.toRotationMatrix()) {}
  Matrix3d& linear() { return L_; }
  const Matrix3d& linear() const { return L_; }
  Vector3d& translation() { return T_; }
  const Vector3d& translation() const { return T_; }
  double operator()(int r, int c) const { return c < 3 ? L_.m[r][c] : T_.v[r]; }
  // transform_transform_product_impl (Affine * Affine): linear = A.L * B.L, translation = A.L * B.t + A.t
  Affine3d operator*(const Affine3d& b) const {
    Affine3d r;
    r.L_ = L_ * b.L_;
    const Vector3d lt = L_ * b.T_;
    for (int i = 0; i < 3; ++i) r.T_.v[i] = lt.v[i] + T_.v[i];
    return r;
  }
  // Transform::inverse(Affine): linear = L^-1 by cofactors (compute_inverse_size3_helper: inv(r,c) = cof(c,r) / det,
  // det = cof(0,0) m00 + cof(1,0) m10 + cof(2,0) m20), translation = -(L^-1 t)
  Affine3d inverse() const {
    auto cof = [this](int i, int j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      return L_.m[i1][j1] * L_.m[i2][j2] - L_.m[i1][j2] * L_.m[i2][j1];
    };
    const double c00 = cof(0, 0), c10 = cof(1, 0), c20 = cof(2, 0);
    const double det = c00 * L_.m[0][0] + c10 * L_.m[1][0] + c20 * L_.m[2][0];
    const double invdet = 1.0 / det;
    Affine3d r;
    for (int row = 0; row < 3; ++row)
      for (int col = 0; col < 3; ++col) r.L_.m[row][col] = cof(col, row) * invdet;
    const Vector3d lt = r.L_ * T_;
    for (int i = 0; i < 3; ++i) r.T_.v[i] = -lt.v[i];
    return r;
  }
  // Translation3d * Quaterniond -> Isometry: linear = q.toRotationMatrix(), translation = 0 + t (pretranslate)
  static Affine3d from(const Translation3d& t, const Quaterniond& q) {
    Affine3d r;
    r.L_ = q.toRotationMatrix();
    for (int i = 0; i < 3; ++i) r.T_.v[i] = 0.0 + t.t[i];
    return r;
  }

 private:
  Matrix3d L_;
  Vector3d T_;
};
using Isometry3d = Affine3d;
inline Affine3d operator*(const Translation3d& t, const Quaterniond& q) { return Affine3d::from(t, q); }
}  // namespace Eigen
#endif
