// SubmapBridge (submap_bridge.h) WITHOUT ROS, PCL, Eigen or a GPU: stand-in cloud, transform and pose types against a
// fake C-ABI that records the calls.  Checked: the capacities and normal_k reach the config; nothing is sent before a
// create; a keyframe's first-point addresses, counts and record sizes, the row-major 3 x 4 transform and the position;
// empty clouds pass no pointer; warmUp selects first and hands the selected ids on in the order they came back, does
// nothing when none is selected, reports a refusal and keeps an earlier warm-up on a refusal of the arguments but not
// on a device failure; swapIfReady swaps once per warm-up and is a no-op otherwise; a new create forgets everything.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/submap_bridge.h"

struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };          // 32 bytes, as PCL lays it out
struct Cloud { std::vector<PointXYZI> points; };
struct Position { double x, y, z; };
struct Affine {                                                        // column-major 4 x 4, like Eigen::Affine3d
  double m[16];
  double operator()(int r, int c) const { return m[4 * c + r]; }
};

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int create_rc = DDDMR_OK, add_rc = DDDMR_OK, select_rc = DDDMR_OK, warm_rc = DDDMR_OK, swap_rc = DDDMR_OK;
  int creates = 0, adds = 0, selects = 0, warms = 0, swaps = 0;
  dddmr_submap_config cfg;
  const float *corner = nullptr, *ground = nullptr;
  size_t n_corner = 0, n_ground = 0, corner_stride = 0, ground_stride = 0;
  double T[12], pos[3], radius = 0;
  bool null_T = false;
  std::vector<int32_t> selected, warmed;
  size_t select_capacity = 0;
} F;
extern "C" {
int dddmr_rollout_submap_create(dddmr_rollout_ctx*, const dddmr_submap_config* cfg) {
  ++F.creates; F.cfg = *cfg;
  return F.create_rc; }
int dddmr_rollout_submap_add_keyframe(dddmr_rollout_ctx*, const float* corner, size_t n_corner, size_t corner_stride, const float* ground,
                                      size_t n_ground, size_t ground_stride, const double T[12], const double position[3], int32_t* id_out) {
  F.corner = corner; F.n_corner = n_corner; F.corner_stride = corner_stride; F.ground = ground; F.n_ground = n_ground; F.ground_stride = ground_stride;
  F.null_T = T == nullptr;
  if (T) std::memcpy(F.T, T, sizeof(F.T));
  std::memcpy(F.pos, position, sizeof(F.pos));
  if (F.add_rc != DDDMR_OK) return F.add_rc;
  if (id_out) *id_out = F.adds;
  ++F.adds;
  return DDDMR_OK; }
int dddmr_rollout_submap_select(dddmr_rollout_ctx*, const double position[3], double radius, int32_t* ids_out, size_t capacity, size_t* n) {
  ++F.selects; F.radius = radius; F.select_capacity = capacity;
  std::memcpy(F.pos, position, sizeof(F.pos));
  if (F.select_rc != DDDMR_OK) return F.select_rc;
  *n = F.selected.size();
  if (F.selected.size() > capacity) return DDDMR_ERR_CAPACITY;
  for (size_t i = 0; i < F.selected.size(); ++i) ids_out[i] = F.selected[i];
  return DDDMR_OK; }
int dddmr_rollout_submap_warm_up(dddmr_rollout_ctx*, const int32_t* ids, size_t n_ids, dddmr_submap_stats* stats) {
  ++F.warms;
  F.warmed.assign(ids, ids + n_ids);
  if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->n_keyframes = (uint32_t)n_ids; }
  return F.warm_rc; }
int dddmr_rollout_submap_swap(dddmr_rollout_ctx*) {
  ++F.swaps;
  return F.swap_rc; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  SubmapBridge b;
  Cloud corner, ground, none;
  corner.points.resize(5);
  ground.points.resize(9);
  Affine T{};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T.m[4 * c + r] = 10.0 * r + c;
  T.m[15] = 1.0;
  const Position at{1.5, -2.5, 0.25};

  // nothing before a create
  assert(b.addKeyframe(corner, ground, T, at) == DDDMR_ERR_STATE && b.warmUp(at, 50.0) == DDDMR_ERR_STATE && b.swapIfReady() == DDDMR_ERR_STATE);
  assert(F.adds == 0 && F.selects == 0 && F.swaps == 0 && !b.created() && !b.warmed());
  assert(b.create(nullptr, 8, 100, 100) == DDDMR_ERR_BAD_ARG && F.creates == 0);
  F.create_rc = DDDMR_ERR_STATE;
  assert(b.create(&ctx, 8, 100, 100) == DDDMR_ERR_STATE && !b.created());
  F.create_rc = DDDMR_OK;
  assert(b.create(&ctx, 8, 1000, 500) == DDDMR_OK && b.created() && F.creates == 2);
  assert(F.cfg.max_keyframes == 8 && F.cfg.max_store_map_points == 1000 && F.cfg.max_store_ground_points == 500 && F.cfg.normal_k == 20);
  assert(F.cfg.reserved[0] == 0 && F.cfg.reserved[1] == 0);

  // a keyframe: addresses, counts, record sizes, the transform row-major, the position, the id
  int32_t id = -7;
  assert(b.addKeyframe(corner, ground, T, at, &id) == DDDMR_OK && id == 0 && b.keyframes() == 1);
  assert(F.corner == &corner.points[0].x && F.n_corner == 5 && F.corner_stride == 32);
  assert(F.ground == &ground.points[0].x && F.n_ground == 9 && F.ground_stride == 32 && !F.null_T);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) assert(F.T[4 * r + c] == 10.0 * r + c);
  assert(F.pos[0] == 1.5 && F.pos[1] == -2.5 && F.pos[2] == 0.25);
  assert(b.addKeyframe(none, ground, T, at, &id) == DDDMR_OK && id == 1 && F.corner == nullptr && F.n_corner == 0 && F.corner_stride == 12);
  assert(b.addKeyframe(corner, none, T, at) == DDDMR_OK && F.ground == nullptr && F.n_ground == 0 && F.ground_stride == 12);
  F.add_rc = DDDMR_ERR_CAPACITY;
  id = -7;
  assert(b.addKeyframe(corner, ground, T, at, &id) == DDDMR_ERR_CAPACITY && id == -7 && b.keyframes() == 3);
  F.add_rc = DDDMR_OK;

  // warmUp: select, then the selected ids in their order
  dddmr_submap_stats st;
  F.selected = {};
  assert(b.warmUp(at, 50.0, &st) == DDDMR_OK && F.selects == 1 && F.warms == 0 && !b.warmed() && st.n_keyframes == 0);
  assert(F.radius == 50.0 && F.select_capacity == 8 && F.pos[1] == -2.5);
  bool swapped = true;
  assert(b.swapIfReady(&swapped) == DDDMR_OK && !swapped && F.swaps == 0);
  F.selected = {0, 2};
  assert(b.warmUp(at, 50.0, &st) == DDDMR_OK && F.warms == 1 && b.warmed() && st.n_keyframes == 2);
  assert(F.warmed == std::vector<int32_t>({0, 2}));
  // a refusal of the arguments keeps the earlier warm-up; a refused select sends no warm-up
  F.warm_rc = DDDMR_ERR_CAPACITY;
  assert(b.warmUp(at, 50.0) == DDDMR_ERR_CAPACITY && F.warms == 2 && b.warmed());
  F.warm_rc = DDDMR_OK;
  F.select_rc = DDDMR_ERR_BAD_ARG;
  assert(b.warmUp(at, -1.0) == DDDMR_ERR_BAD_ARG && F.warms == 2 && b.warmed());
  F.select_rc = DDDMR_OK;
  assert(b.swapIfReady(&swapped) == DDDMR_OK && swapped && F.swaps == 1 && !b.warmed());
  assert(b.swapIfReady(&swapped) == DDDMR_OK && !swapped && F.swaps == 1);
  // a device failure loses the earlier warm-up; a refused swap leaves nothing waiting
  assert(b.warmUp(at, 50.0) == DDDMR_OK && b.warmed());
  F.warm_rc = DDDMR_ERR_HIP;
  assert(b.warmUp(at, 50.0) == DDDMR_ERR_HIP && !b.warmed());
  F.warm_rc = DDDMR_OK;
  assert(b.warmUp(at, 50.0) == DDDMR_OK && b.warmed());
  F.swap_rc = DDDMR_ERR_STATE;
  assert(b.swapIfReady(&swapped) == DDDMR_ERR_STATE && !swapped && F.swaps == 2 && !b.warmed());
  F.swap_rc = DDDMR_OK;

  // a new create forgets the keyframes and the warm-up
  assert(b.warmUp(at, 50.0) == DDDMR_OK && b.warmed());
  assert(b.create(&ctx, 4, 10, 10, 12) == DDDMR_OK && !b.warmed() && b.keyframes() == 0 && F.cfg.normal_k == 12);
  assert(b.swapIfReady(&swapped) == DDDMR_OK && !swapped && F.swaps == 2);
  std::printf("submap bridge OK\n");
  return 0;
}
