// Runs pure_pursuit_last_pose() (csrc/rollout_kernels.hip.h) on the CPU for tests/test_pure_pursuit_cpu.py: the one
// function through which the rollout files PurePursuitModel's (distance, folded yaw) of a trajectory's last pose, on
// poses worked out by hand and, when a file is given, on recorded world poses against the oracle's own values.
// usage: pure_pursuit_test [poses.txt]      (prints "pure pursuit OK: <n> checks", exit status 0)
// poses.txt: one line per pose, 16 numbers: trajectory pose x y z qx qy qz qw, plan pose x y z qx qy qz qw, the oracle's
// distance and folded yaw.  The program makes no HIP call.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rollout_kernels.hip.h"

using namespace dddmr;

static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    ++n_checks;                                                                         \
    if (!(cond)) { ++n_failed; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
  } while (0)

static const double kFold = 3.1416;      // pure_pursuit_model.cpp:110
static const double kPi = 3.14159265358979323846;

static void set_identity(double R[9]) {
  for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
}
static void rot_z(double a, double R[9]) {
  set_identity(R);
  R[0] = std::cos(a); R[1] = -std::sin(a); R[3] = std::sin(a); R[4] = std::cos(a);
}
static void rot_y(double a, double R[9]) {
  set_identity(R);
  R[0] = std::cos(a); R[2] = std::sin(a); R[6] = -std::sin(a); R[8] = std::cos(a);
}
static void mul(const double A[9], const double B[9], double C[9]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
static void quat_rot(const double q[4], double R[9]) {      // (x, y, z, w), Eigen's toRotationMatrix
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// robot at the origin, plan pose = identity, unless told otherwise
static DevTick plain_tick() {
  DevTick k;
  std::memset(&k, 0, sizeof(k));
  set_identity(k.R);
  set_identity(k.planR);
  k.m = 80;
  return k;
}

static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }
// the fold is a saw-tooth: a yaw of +-1e-16 lands on either side of its jump
static bool near_folded(double a, double b, double tol) {
  const double d = std::fabs(a - b);
  return d <= tol || std::fabs(d - kFold) <= tol;
}
static double folded(double yaw) { return std::fmod(yaw + kFold, kFold); }

static void hand_cases() {
  // identity: nothing to go, nothing to turn; fmod(3.1416, 3.1416) is an exact zero
  {
    const DevTick k = plain_tick();
    const double2 r = pure_pursuit_last_pose(k, make_float2(0.f, 0.f), make_double2(1.0, 0.0));
    CHECK(r.x == 0.0);
    CHECK(r.y == 0.0);
  }
  // the trajectory ends heading theta, the plan pose heads 0: the difference's yaw is -theta
  {
    const DevTick k = plain_tick();
    double2 r = pure_pursuit_last_pose(k, make_float2(0.f, 0.f), make_double2(0.0, 1.0));      // theta = +pi/2
    CHECK(r.x == 0.0);
    CHECK(near(r.y, kFold - kPi / 2, 1e-15));
    r = pure_pursuit_last_pose(k, make_float2(0.f, 0.f), make_double2(0.0, -1.0));             // theta = -pi/2
    CHECK(near(r.y, kPi / 2, 1e-15));
  }
  // the plan pose heads phi, the trajectory 0: yaw phi.  phi = +pi folds to pi (fmod(pi + 3.1416, 3.1416)), phi = -pi
  // (sin = -0 after the products: atan2(-0, -1)) to 3.1416 - pi
  {
    DevTick k = plain_tick();
    k.planR[0] = -1.0; k.planR[4] = -1.0; k.planR[3] = 0.0; k.planR[1] = 0.0;
    double2 r = pure_pursuit_last_pose(k, make_float2(0.f, 0.f), make_double2(1.0, 0.0));
    CHECK(near(r.y, folded(kPi), 1e-15));
    k.planR[3] = -0.0;
    r = pure_pursuit_last_pose(k, make_float2(0.f, 0.f), make_double2(1.0, 0.0));
    // (0 * -1) + (1 * -0) + 0 = (-0 + -0) + 0 = +0 under round-to-nearest: atan2(+0, -1) = +pi all the same
    CHECK(near(r.y, folded(kPi), 1e-15));
    for (const double phi : {kPi / 2, -kPi / 2, 0.4, -2.5}) {
      rot_z(phi, k.planR);
      r = pure_pursuit_last_pose(k, make_float2(0.f, 0.f), make_double2(1.0, 0.0));
      CHECK(near(r.y, folded(phi), 1e-15));
    }
  }
  // translation: the plan pose 3 ahead and 4 to the left of a trajectory that ends at (1, 2) heading 0
  {
    DevTick k = plain_tick();
    k.planT[0] = 4.0; k.planT[1] = 6.0; k.planT[2] = 0.0;
    const double2 r = pure_pursuit_last_pose(k, make_float2(1.f, 2.f), make_double2(1.0, 0.0));
    CHECK(r.x == 5.0);
    CHECK(r.y == 0.0);
  }
  // |D20| >= 1 (getEulerYPR's gimbal branch): the plan pose pitched by a quarter turn, D20 = planR[6] = -1 -> yaw 0
  {
    DevTick k = plain_tick();
    const double ry[9] = {0, 0, 1, 0, 1, 0, -1, 0, 0};
    std::memcpy(k.planR, ry, sizeof(ry));
    k.planT[2] = 2.0;
    const double2 r = pure_pursuit_last_pose(k, make_float2(0.f, 0.f), make_double2(std::cos(0.3), std::sin(0.3)));
    CHECK(r.x == 2.0);
    CHECK(r.y == 0.0);
  }
  // the plan pose IS the trajectory's last pose: distance exactly 0, yaw 0 up to the rounding of L^T L
  {
    DevTick k = plain_tick();
    rot_z(0.3, k.R);
    k.t[0] = 1.0; k.t[1] = 2.0; k.t[2] = 0.5;
    const float2 bxy = make_float2(0.5f, 0.25f);
    const double c = std::cos(0.7), s = std::sin(0.7);
    for (int i = 0; i < 3; ++i) {          // L and T by the helper's own operations
      k.planR[3 * i + 0] = k.R[3 * i] * c + k.R[3 * i + 1] * s;
      k.planR[3 * i + 1] = k.R[3 * i + 1] * c - k.R[3 * i] * s;
      k.planR[3 * i + 2] = k.R[3 * i + 2];
    }
    pose_translation(k, bxy, k.planT);
    const double2 r = pure_pursuit_last_pose(k, bxy, make_double2(c, s));
    CHECK(r.x == 0.0);
    CHECK(near_folded(r.y, 0.0, 1e-15));
  }
  // a pitched robot (a 10 degree ramp): the plan pose sits (0.3, -0.4, 0) away in the trajectory's own frame and is
  // turned by 0.4 about its z -> distance 0.5, yaw 0.4
  {
    DevTick k = plain_tick();
    rot_y(10.0 * kPi / 180.0, k.R);
    k.t[0] = -2.0; k.t[1] = 1.0; k.t[2] = 0.25;
    const float2 bxy = make_float2(1.0f, 0.5f);
    const double th = 0.25, c = std::cos(th), s = std::sin(th);
    double rz[9], L[9], T[3], rz4[9];
    rot_z(th, rz);
    mul(k.R, rz, L);
    pose_translation(k, bxy, T);
    rot_z(0.4, rz4);
    mul(L, rz4, k.planR);
    for (int i = 0; i < 3; ++i) k.planT[i] = T[i] + L[3 * i] * 0.3 + L[3 * i + 1] * -0.4;
    const double2 r = pure_pursuit_last_pose(k, bxy, make_double2(c, s));
    CHECK(near(r.x, 0.5, 1e-14));
    CHECK(near(r.y, folded(0.4), 1e-14));
  }
}

// recorded world poses: robot pose := the trajectory's last pose, body-frame state := the origin heading 0, so that the
// helper's L and T are that pose exactly
static int file_cases(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
  double v[16];
  int n = 0;
  for (;;) {
    int got = 0;
    for (; got < 16; ++got)
      if (std::fscanf(f, "%lf", &v[got]) != 1) break;
    if (got == 0) break;
    if (got != 16) { std::fprintf(stderr, "%s: short line\n", path); std::fclose(f); return 1; }
    DevTick k = plain_tick();
    quat_rot(v + 3, k.R);
    for (int i = 0; i < 3; ++i) k.t[i] = v[i];
    quat_rot(v + 10, k.planR);
    for (int i = 0; i < 3; ++i) k.planT[i] = v[7 + i];
    const double2 r = pure_pursuit_last_pose(k, make_float2(0.f, 0.f), make_double2(1.0, 0.0));
    const bool ok_d = near(r.x, v[14], 1e-12 * std::fmax(std::fabs(v[14]), 1e-300));
    const bool ok_y = near_folded(r.y, v[15], 1e-12 * std::fmax(std::fabs(v[15]), 1.0));
    if (!ok_d || !ok_y) std::fprintf(stderr, "pose %d: got (%.17g, %.17g), the oracle has (%.17g, %.17g)\n", n, r.x, r.y, v[14], v[15]);
    CHECK(ok_d);
    CHECK(ok_y);
    ++n;
  }
  std::fclose(f);
  std::printf("pure pursuit: %d recorded poses\n", n);
  return 0;
}

int main(int argc, char** argv) {
  hand_cases();
  if (argc > 1 && file_cases(argv[1]) != 0) return 2;
  if (n_failed) {
    std::fprintf(stderr, "pure pursuit: %d of %d checks FAILED\n", n_failed, n_checks);
    return 1;
  }
  std::printf("pure pursuit OK: %d checks\n", n_checks);
  return 0;
}
