// LocalizationBridge of localization_bridge.h WITHOUT ROS, PCL or a GPU: instantiated with stand-in cloud, normal and
// state types against a fake C-ABI that records the calls.  Checked: the parameters and capacities reach the config;
// the context is set only after a successful create; ready() needs a create and a setMap that both succeeded and
// drops on a failure of either; the clouds' first-point addresses and record sizes, the packed normals, flat points,
// less-sharp points with their intensity and the states in pos xyz, rot xyzw order; likelihoods and qualities come
// back in particle order with the minimum and maximum; a failing measure is reported and leaves the outputs alone;
// empty clouds and no particles pass no pointer.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/localization_bridge.h"

struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };          // 32 bytes, as PCL lays it out
struct Normal { float normal_x, normal_y, normal_z, pad, curvature, pad2[3]; };
struct Cloud { std::vector<PointXYZI> points; };
struct Normals { std::vector<Normal> points; };
struct Vec3 { float x_, y_, z_; };
struct Quat { float x_, y_, z_, w_; };
struct State6DOF { Vec3 pos_; Quat rot_; int other = 0; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int create_rc = DDDMR_OK, map_rc = DDDMR_OK, measure_rc = DDDMR_OK;
  int creates = 0, maps = 0, measures = 0;
  dddmr_mcl_config cfg;
  const float *map = nullptr, *ground = nullptr;
  size_t n_map = 0, n_ground = 0, map_stride = 0, ground_stride = 0, normal_stride = 0;
  std::vector<float> normals, flat, ls, states;
  bool null_inputs = false;
} F;
extern "C" {
int dddmr_rollout_mcl_create(dddmr_rollout_ctx*, const dddmr_mcl_config* cfg) {
  ++F.creates; F.cfg = *cfg;
  return F.create_rc; }
int dddmr_rollout_mcl_set_map(dddmr_rollout_ctx*, const float* map_xyz, size_t n_map, size_t map_stride, const float* ground_xyz,
                              const float* normals, size_t n_ground, size_t ground_stride, size_t normal_stride) {
  ++F.maps; F.map = map_xyz; F.n_map = n_map; F.map_stride = map_stride; F.ground = ground_xyz; F.n_ground = n_ground;
  F.ground_stride = ground_stride; F.normal_stride = normal_stride;
  F.normals.clear();
  if (normals) F.normals.assign(normals, normals + 3 * n_ground);
  return F.map_rc; }
int dddmr_rollout_mcl_measure(dddmr_rollout_ctx*, const float* flat, size_t n_flat, const float* ls, size_t n_ls, const float* states,
                              size_t n, float* like, float* qual, dddmr_mcl_stats* stats) {
  ++F.measures;
  F.null_inputs = !flat && !ls && !states && !like && !qual;
  F.flat.clear(); F.ls.clear(); F.states.clear();
  if (flat) F.flat.assign(flat, flat + 3 * n_flat);
  if (ls) F.ls.assign(ls, ls + 4 * n_ls);
  if (states) F.states.assign(states, states + 7 * n);
  if (F.measure_rc != DDDMR_OK) return F.measure_rc;
  for (size_t i = 0; i < n; ++i) { like[i] = 10.f + (float)i; qual[i] = 0.1f * (float)(i + 1); }
  std::memset(stats, 0, sizeof(*stats));
  stats->quality_min = 0.1f; stats->quality_max = 0.1f * (float)n;
  return DDDMR_OK; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  Cloud map, ground, flat, ls, none;
  Normals normals, no_normals;
  map.points.resize(5); ground.points.resize(3); normals.points.resize(3);
  for (int i = 0; i < 3; ++i) normals.points[i] = Normal{0.1f * i, 0.2f * i, 1.f - 0.1f * i, 0, 0, {0, 0, 0}};
  flat.points.resize(2); ls.points.resize(2);
  flat.points[1] = PointXYZI{1, 2, 3, 0, 9, {0, 0, 0}};
  ls.points[0] = PointXYZI{4, 5, 6, 0, 1.5f, {0, 0, 0}};
  ls.points[1] = PointXYZI{7, 8, 9, 0, 2.5f, {0, 0, 0}};
  std::vector<State6DOF> particles(3);
  for (int i = 0; i < 3; ++i) particles[i] = State6DOF{{1.f + i, 2.f + i, 3.f + i}, {0.1f, 0.2f, 0.3f, 2.f + i}, i};
  std::vector<float> like{-1.f}, qual{-2.f};
  float qmin = -1, qmax = -1;

  LocalizationBridge b;
  assert(!b.ready());
  assert(b.setMap(map, ground, normals) == DDDMR_ERR_STATE && F.maps == 0);                       // before create: no call
  assert(b.measure(flat, ls, particles, like, qual) == DDDMR_ERR_STATE && F.measures == 0);
  // a failing create leaves no context behind: nothing is ever sent to it
  F.create_rc = DDDMR_ERR_CAPACITY;
  assert(b.create(&ctx, 0.3, 0.05, 1.0, 6, 1000, 500, 60) == DDDMR_ERR_CAPACITY && !b.ready());
  assert(b.setMap(map, ground, normals) == DDDMR_ERR_STATE && F.maps == 0);
  assert(b.create(nullptr, 0.3, 0.05, 1.0, 6, 1000, 500, 60) == DDDMR_ERR_BAD_ARG && F.creates == 1);
  F.create_rc = DDDMR_OK;
  assert(b.create(&ctx, 0.3, 0.05, 1.0, 6, 1000, 500, 60) == DDDMR_OK && F.creates == 2);
  assert(F.cfg.match_dist_min == 0.3 && F.cfg.match_dist_flat == 0.05 && F.cfg.radius_of_ground_search == 1.0 &&
         F.cfg.threshold_for_trusted_ground == 6 && F.cfg.max_map_points == 1000 && F.cfg.max_ground_points == 500 &&
         F.cfg.max_particles == 60 && F.cfg.max_observation_points == 2000 && F.cfg.max_ground_neighbours == 1024 && F.cfg.reserved == 0);
  assert(!b.ready());                                                                           // no map yet
  assert(b.measure(flat, ls, particles, like, qual) == DDDMR_ERR_STATE && F.measures == 0);
  // normals: one per ground point
  assert(b.setMap(map, ground, no_normals) == DDDMR_ERR_BAD_ARG && F.maps == 0 && !b.ready());
  assert(b.setMap(map, ground, normals) == DDDMR_OK && b.ready());
  assert(F.map == &map.points[0].x && F.n_map == 5 && F.map_stride == sizeof(PointXYZI) && F.ground == &ground.points[0].x &&
         F.n_ground == 3 && F.ground_stride == sizeof(PointXYZI) && F.normal_stride == 12);
  assert(F.normals.size() == 9 && F.normals[3] == 0.1f && F.normals[4] == 0.2f && F.normals[5] == 0.9f);

  assert(b.measure(flat, ls, particles, like, qual, &qmin, &qmax) == DDDMR_OK && F.measures == 1);
  assert(F.flat.size() == 6 && F.flat[3] == 1 && F.flat[4] == 2 && F.flat[5] == 3);
  assert(F.ls.size() == 8 && F.ls[0] == 4 && F.ls[3] == 1.5f && F.ls[4] == 7 && F.ls[7] == 2.5f);
  const float want1[7] = {2, 3, 4, 0.1f, 0.2f, 0.3f, 3};
  assert(F.states.size() == 21 && std::memcmp(&F.states[7], want1, sizeof(want1)) == 0);
  assert(like.size() == 3 && like[0] == 10.f && like[2] == 12.f && qual.size() == 3 && qual[1] == 0.2f);       // particle order
  assert(qmin == 0.1f && qmax == 0.1f * 3.f);
  // a failing measure: the code comes back, the outputs stay, the bridge stays ready (the map is still the filter's)
  for (int code : {DDDMR_ERR_CAPACITY, DDDMR_ERR_STATE, DDDMR_ERR_HIP}) {
    F.measure_rc = code;
    like[0] = 77.f; qmin = 5.f;
    assert(b.measure(flat, ls, particles, like, qual, &qmin, &qmax) == code && like[0] == 77.f && like.size() == 3 && qmin == 5.f && b.ready());
  }
  F.measure_rc = DDDMR_OK;
  // nothing to pack: no pointers
  std::vector<State6DOF> nobody;
  assert(b.measure(none, none, nobody, like, qual) == DDDMR_OK && F.null_inputs && like.empty() && qual.empty());
  // a refused setMap: the device answers from the old map, which is no longer the filter's
  F.map_rc = DDDMR_ERR_CAPACITY;
  assert(b.setMap(map, ground, normals) == DDDMR_ERR_CAPACITY && !b.ready());
  const int measures = F.measures;
  assert(b.measure(flat, ls, particles, like, qual) == DDDMR_ERR_STATE && F.measures == measures);
  F.map_rc = DDDMR_OK;
  assert(b.setMap(none, none, no_normals) == DDDMR_OK && b.ready() && F.map == nullptr && F.ground == nullptr && F.n_map == 0);
  // a second create forgets the map
  assert(b.create(&ctx, 0.3, 0.05, 1.0, 6, 1000, 500, 60, 100, 50) == DDDMR_OK && !b.ready());
  assert(F.cfg.max_observation_points == 100 && F.cfg.max_ground_neighbours == 50);
  std::printf("localization bridge OK\n");
  return 0;
}
