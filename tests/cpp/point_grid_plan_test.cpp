// Drives csrc/point_grid_plan.hip.h -- a grid's shape, the host cell functions, staging a caller's cloud and the limits a
// cloud has to keep -- from a stand-alone host program: every expectation is written out here, next to the call.  It makes
// no HIP runtime call (float4 is the only thing it takes from HIP), so it runs without a GPU.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mcl_submap_plan.hip.h"   // submap_transform_row: the one transform the library stages with
#include "point_grid_plan.hip.h"

using namespace dddmr;

namespace {

int failures = 0, checks = 0;
#define CHECK(cond, ...)                                                                                      \
  do {                                                                                                        \
    ++checks;                                                                                                 \
    if (!(cond)) {                                                                                            \
      if (++failures <= 20) { std::printf("FAIL %s (line %d): ", #cond, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                                                         \
  } while (0)

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
bool same(const float4& a, float x, float y, float z) { return bits(a.x) == bits(x) && bits(a.y) == bits(y) && bits(a.z) == bits(z) && bits(a.w) == 0u; }

constexpr float kInf = std::numeric_limits<float>::infinity();
constexpr float kNan = std::numeric_limits<float>::quiet_NaN();

// n records `stride_bytes` apart: x y z, then filler the staging must not look at
std::vector<float> records(size_t n, size_t stride_bytes) {
  const size_t sf = stride_bytes / 4;
  std::vector<float> v(n * sf + 1, kNan);
  for (size_t i = 0; i < n; ++i) {
    v[i * sf + 0] = 4000.0f + 0.37f * (float)i - (i == 3 ? 7.0f : 0.0f);
    v[i * sf + 1] = -3.0f + 1.5f * (float)((i * 7) % 5);
    v[i * sf + 2] = 0.25f * (float)i * (i & 1 ? -1.0f : 1.0f);
  }
  return v;
}

void test_stage_cloud() {
  const size_t strides[3] = {12, 16, 32}, counts[3] = {0, 1, 5};
  for (size_t stride : strides)
    for (size_t n : counts) {
      const std::vector<float> src = records(n, stride);
      const size_t sf = stride / 4;
      std::vector<float4> out(n + 1, make_float4(9.f, 9.f, 9.f, 9.f));
      float lo[3] = {7, 7, 7}, hi[3] = {7, 7, 7};
      CHECK(stage_cloud(src.data(), n, stride, out.data(), lo, hi), "n %zu stride %zu: finite input refused", n, stride);
      float elo[3] = {0, 0, 0}, ehi[3] = {0, 0, 0};
      for (size_t i = 0; i < n; ++i) {
        const float* p = &src[i * sf];
        CHECK(same(out[i], p[0], p[1], p[2]), "n %zu stride %zu: record %zu", n, stride, i);
        for (int a = 0; a < 3; ++a) {
          if (i == 0 || p[a] < elo[a]) elo[a] = p[a];
          if (i == 0 || p[a] > ehi[a]) ehi[a] = p[a];
        }
      }
      CHECK(bits(out[n].x) == bits(9.f), "n %zu stride %zu: wrote past the last record", n, stride);
      for (int a = 0; a < 3; ++a)
        CHECK(bits(lo[a]) == bits(elo[a]) && bits(hi[a]) == bits(ehi[a]), "n %zu stride %zu axis %d: box %g .. %g, expected %g .. %g", n, stride, a, lo[a], hi[a],
              elo[a], ehi[a]);
      // HostCloud is the same staging owning its records: one zero element without a point
      const HostCloud h(src.data(), n, stride);
      CHECK(h.pts.size() == (n ? n : 1), "HostCloud size");
      if (!n) CHECK(same(h.pts[0], 0.f, 0.f, 0.f), "HostCloud's element without a point");
      for (size_t i = 0; i < n; ++i) CHECK(std::memcmp(&h.pts[i], &out[i], sizeof(float4)) == 0, "HostCloud record %zu", i);
      for (int a = 0; a < 3; ++a) CHECK(bits(h.lo[a]) == bits(elo[a]) && bits(h.hi[a]) == bits(ehi[a]), "HostCloud box");
      CHECK(h.finite && cloud_coords_ok(h), "a finite cloud of %zu points inside the limits refused", n);
    }

  // a coordinate that is not finite is reported wherever it stands
  const float bad[3] = {kNan, kInf, -kInf};
  const size_t at[3] = {0, 2, 4};
  for (size_t stride : strides)
    for (float b : bad)
      for (size_t rec : at)
        for (int axis = 0; axis < 3; ++axis) {
          std::vector<float> src = records(5, stride);
          src[rec * (stride / 4) + axis] = b;
          std::vector<float4> out(5);
          float lo[3], hi[3];
          CHECK(!stage_cloud(src.data(), 5, stride, out.data(), lo, hi), "stride %zu: %g at record %zu axis %d passed", stride, b, rec, axis);
          const HostCloud h(src.data(), 5, stride);          // ... HostCloud keeps it, and cloud_coords_ok refuses the cloud
          CHECK(bits(((const float*)&h.pts[rec])[axis]) == bits(b) && !h.finite && !cloud_coords_ok(h), "HostCloud with %g at record %zu axis %d", b, rec, axis);
        }

  // a finite input that the transform turns infinite
  {
    const std::vector<float> src = records(5, 16);
    std::vector<float4> out(5);
    float lo[3], hi[3];
    int calls = 0;
    CHECK(stage_cloud(src.data(), 5, 16, out.data(), lo, hi, [&](float* v) { ++calls; v[1] *= 2.0f; }), "a finite transform refused");
    CHECK(calls == 5 && same(out[2], src[8], 2.0f * src[9], src[10]), "the transform's result is what is staged");
    for (size_t rec : at)
      CHECK(!stage_cloud(src.data(), 5, 16, out.data(), lo, hi, [&](float* v) { if (v[0] == src[rec * 4]) v[2] = v[0] * 3e38f; }),   // x is unlike in every record
            "an overflow in the transform at record %zu passed", rec);
  }

  // the sub-maps' transform: pcl::transformPointCloud's double expression with one rounding, per point
  {
    const double T[12] = {0.36, -0.48, 0.8, 1234.5678, 0.8, 0.6, 0.0, -987.654321, -0.48, 0.64, 0.6, 12.000001};
    const auto to_map = [&](float* v) {
      const float x = v[0], y = v[1], z = v[2];
      for (int a = 0; a < 3; ++a) v[a] = submap_transform_row(T, a, x, y, z);
    };
    for (size_t stride : strides) {
      const std::vector<float> src = records(5, stride);
      std::vector<float4> out(5);
      float lo[3], hi[3];
      CHECK(stage_cloud(src.data(), 5, stride, out.data(), lo, hi, to_map), "the transformed cloud refused");
      for (size_t i = 0; i < 5; ++i) {
        const float* p = &src[i * (stride / 4)];
        CHECK(same(out[i], submap_transform_row(T, 0, p[0], p[1], p[2]), submap_transform_row(T, 1, p[0], p[1], p[2]), submap_transform_row(T, 2, p[0], p[1], p[2])),
              "stride %zu: transformed record %zu", stride, i);
        for (int a = 0; a < 3; ++a) {
          const float v = submap_transform_row(T, a, p[0], p[1], p[2]);
          CHECK(lo[a] <= v && v <= hi[a], "the box is the transformed points'");
        }
      }
    }
  }

  CHECK(cloud_arg_ok(nullptr, 0, 0) && !cloud_arg_ok(nullptr, 1, 12), "cloud_arg_ok: a count of 0 asks nothing, a null cloud is refused");
  const float one[3] = {0, 0, 0};
  CHECK(cloud_arg_ok(one, 1, 12) && cloud_arg_ok(one, 1, 32) && !cloud_arg_ok(one, 1, 8) && !cloud_arg_ok(one, 1, 14), "cloud_arg_ok: strides");
}

void test_grid_shape() {
  const float lo[3] = {1.0f, 2.0f, 3.0f}, hi[3] = {4.0f, 4.0f, 4.0f};   // 3 x 2 x 1 m
  PointGrid g;
  grid_shape(g, lo, hi, 0.5f, 0.5f, 1000);
  CHECK(g.nx == 7 && g.ny == 5 && g.nz == 3, "a box that fits: %d x %d x %d", g.nx, g.ny, g.nz);           // ceil(extent / cell) + 1
  CHECK(bits(g.inv_xy) == bits(2.0f) && bits(g.inv_z) == bits(2.0f), "a box that fits keeps the asked cell");
  CHECK(bits(g.ox) == bits(lo[0]) && bits(g.oy) == bits(lo[1]) && bits(g.oz) == bits(lo[2]), "the origin is lo");

  // cap 50: 0.5 -> 0.65 (6 x 5 x 3 = 90) -> 0.845 (5 x 4 x 3 = 60) -> 1.0985 (4 x 3 x 2 = 24)
  grid_shape(g, lo, hi, 0.5f, 0.5f, 50);
  float cell = 0.5f;
  int steps = 0;
  for (;; ++steps) {
    const long cells = ((long)std::ceil(3.0f / cell) + 1) * ((long)std::ceil(2.0f / cell) + 1) * ((long)std::ceil(1.0f / cell) + 1);
    if (cells <= 50) break;
    cell *= 1.3f;
  }
  CHECK(steps == 3, "powers of 1.3: %d", steps);
  CHECK(g.nx == 4 && g.ny == 3 && g.nz == 2, "coarsened: %d x %d x %d", g.nx, g.ny, g.nz);
  CHECK(bits(g.inv_xy) == bits(1.0f / cell) && bits(g.inv_z) == bits(1.0f / cell), "coarsened by powers of 1.3: 1 / %g, expected 1 / %g", 1.0f / g.inv_xy, cell);
  CHECK(bits(g.ox) == bits(lo[0]) && bits(g.oy) == bits(lo[1]) && bits(g.oz) == bits(lo[2]), "the origin is lo");
  // the two cell sizes coarsen together
  grid_shape(g, lo, hi, 0.5f, 0.25f, 50);
  CHECK((long)g.nx * g.ny * g.nz <= 50 && bits(g.inv_z / g.inv_xy) == bits(2.0f), "xy and z cells keep their ratio");

  grid_shape(g, lo, lo, 0.5f, 0.5f, 1000);
  CHECK(g.nx == 1 && g.ny == 1 && g.nz == 1, "a degenerate box: %d x %d x %d", g.nx, g.ny, g.nz);
}

void test_host_cells() {
  const float lo[3] = {4000.0f, 4000.0f, 4000.0f}, hi[3] = {4003.0f, 4002.0f, 4001.0f};
  PointGrid g;
  grid_shape(g, lo, hi, 0.5f, 0.25f, 1000);
  CHECK(g.nx == 7 && g.ny == 5 && g.nz == 5, "the grid at 4 km: %d x %d x %d", g.nx, g.ny, g.nz);
  const float below_edge = std::nextafterf(4000.5f, 0.0f), below_z = std::nextafterf(4000.25f, 0.0f);
  CHECK(host_cx(g, 3999.0f) == 0 && host_cx(g, -1e6f) == 0 && host_cx(g, 4000.0f) == 0, "x clamps below");
  CHECK(host_cx(g, 4100.0f) == 6 && host_cx(g, 1e6f) == 6 && host_cx(g, 4003.0f) == 6, "x clamps above");
  CHECK(host_cx(g, 4000.5f) == 1 && host_cx(g, below_edge) == 0 && host_cx(g, 4002.5f) == 5, "x at the cell edges");
  CHECK(host_cy(g, 3999.0f) == 0 && host_cy(g, 4100.0f) == 4, "y clamps");
  CHECK(host_cy(g, 4000.5f) == 1 && host_cy(g, below_edge) == 0 && host_cy(g, 4002.0f) == 4, "y at the cell edges");
  CHECK(host_cz(g, 3000.0f) == 0 && host_cz(g, 5000.0f) == 4, "z clamps");
  CHECK(host_cz(g, 4000.25f) == 1 && host_cz(g, below_z) == 0 && host_cz(g, 4001.0f) == 4, "z at the cell edges (its own cell size)");
}

void test_cloud_limits() {
  const float big = 1e6f, over = std::nextafterf(1e6f, kInf);
  const float a[3] = {big, -big, big}, z[3] = {0, 0, 0};
  CHECK(cloud_box_ok(a, a), "1e6 m passes");
  for (int axis = 0; axis < 3; ++axis) {
    float lo[3] = {big, big, big}, hi[3] = {big, big, big};
    hi[axis] = over;
    CHECK(!cloud_box_ok(lo, hi), "the next float above 1e6 passed (hi, axis %d)", axis);
    lo[axis] = hi[axis] = -over;
    CHECK(!cloud_box_ok(lo, hi), "the next float below -1e6 passed (axis %d)", axis);
    float wide[3] = {0, 0, 0};
    wide[axis] = kCloudMaxExtent;
    CHECK(cloud_box_ok(z, wide), "an extent of exactly the limit refused (axis %d)", axis);
    wide[axis] = std::nextafterf(kCloudMaxExtent, kInf);
    CHECK(!cloud_box_ok(z, wide), "an extent above the limit passed (axis %d)", axis);
    float nan_lo[3] = {0, 0, 0}, nan_hi[3] = {0, 0, 0};
    nan_lo[axis] = kNan;
    CHECK(!cloud_box_ok(nan_lo, z), "a NaN lower bound passed (axis %d)", axis);
    nan_hi[axis] = kNan;
    CHECK(!cloud_box_ok(z, nan_hi), "a NaN upper bound passed (axis %d)", axis);
  }
  static_assert(kCloudMaxExtent == 4096.0f, "half of the 8192 m below which 1.5 ulp stay under the 1e-3 m pads");
}

}  // namespace

int main() {
  test_stage_cloud();
  test_grid_shape();
  test_host_cells();
  test_cloud_limits();
  if (failures) {
    std::printf("point grid plan: %d of %d checks FAILED\n", failures, checks);
    return 1;
  }
  std::printf("point grid plan OK: %d checks\n", checks);
  return 0;
}
