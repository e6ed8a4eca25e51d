// The observation calls of LocalizationBridge (localization_bridge.h) WITHOUT ROS, PCL, Eigen or a GPU: stand-in cloud,
// transform and state types against a fake C-ABI that records the calls.  Checked: the two parameters and the
// capacities reach the config; nothing is sent before a create or before a configuration; the clouds' first-point
// addresses, counts and record sizes and the row-major 3 x 4 transform; the sweep source id; prepared() needs a
// successful prepare and drops on a failing one, on a new configuration and on a new create; measurePrepared packs the
// states in pos xyz, rot xyzw order, returns likelihoods and qualities in particle order with the minimum and maximum,
// reports a failing call and leaves the outputs alone; empty clouds and no particles pass no pointer.
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
struct Affine {                                                        // column-major 4 x 4, like Eigen::Affine3d
  double m[16];
  double operator()(int r, int c) const { return m[4 * c + r]; }
};

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int config_rc = DDDMR_OK, prepare_rc = DDDMR_OK, sweep_rc = DDDMR_OK, measure_rc = DDDMR_OK;
  int configs = 0, prepares = 0, sweeps = 0, measures = 0;
  dddmr_mcl_observation_config cfg;
  const float *flat = nullptr, *ls = nullptr;
  size_t n_flat = 0, n_ls = 0, flat_stride = 0, ls_stride = 0;
  double T[12];
  int32_t source = -1;
  std::vector<float> states;
  bool null_inputs = false;
} F;
extern "C" {
int dddmr_rollout_mcl_create(dddmr_rollout_ctx*, const dddmr_mcl_config*) { return DDDMR_OK; }
int dddmr_rollout_mcl_set_map(dddmr_rollout_ctx*, const float*, size_t, size_t, const float*, const float*, size_t, size_t, size_t) {
  return DDDMR_OK; }
int dddmr_rollout_mcl_set_observation_config(dddmr_rollout_ctx*, const dddmr_mcl_observation_config* cfg) {
  ++F.configs; F.cfg = *cfg;
  return F.config_rc; }
int dddmr_rollout_mcl_prepare(dddmr_rollout_ctx*, const float* flat, size_t n_flat, size_t flat_stride, const float* ls, size_t n_ls,
                              size_t ls_stride, const double T[12], dddmr_mcl_observation_stats* stats) {
  ++F.prepares; F.flat = flat; F.n_flat = n_flat; F.flat_stride = flat_stride; F.ls = ls; F.n_ls = n_ls; F.ls_stride = ls_stride;
  std::memcpy(F.T, T, sizeof(F.T));
  if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->n_flat_in = (uint32_t)n_flat; stats->branch = 2; }
  return F.prepare_rc; }
int dddmr_rollout_mcl_prepare_from_sweep(dddmr_rollout_ctx*, int32_t source_id, const double T[12], dddmr_mcl_observation_stats* stats) {
  ++F.sweeps; F.source = source_id;
  std::memcpy(F.T, T, sizeof(F.T));
  if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->branch = 1; }
  return F.sweep_rc; }
int dddmr_rollout_mcl_measure_prepared(dddmr_rollout_ctx*, const float* states, size_t n, float* like, float* qual, dddmr_mcl_stats* stats) {
  ++F.measures;
  F.null_inputs = !states && !like && !qual;
  F.states.clear();
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
  Normals normals;
  flat.points.resize(2); ls.points.resize(3);
  Affine t{};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) t.m[4 * c + r] = 10.0 * r + c;         // T(r, c) = 10 r + c
  t.m[15] = 1.0;
  std::vector<State6DOF> particles(3);
  for (int i = 0; i < 3; ++i) particles[i] = State6DOF{{1.f + i, 2.f + i, 3.f + i}, {0.1f, 0.2f, 0.3f, 2.f + i}, i};
  std::vector<float> like{-1.f}, qual{-2.f};
  float qmin = -1, qmax = -1;
  dddmr_mcl_observation_stats st;

  LocalizationBridge b;
  // before a create nothing is sent
  assert(b.configureObservation(0.8, 3, 400, 1600) == DDDMR_ERR_STATE && F.configs == 0);
  assert(b.prepareObservation(flat, ls, t) == DDDMR_ERR_STATE && b.prepareObservation(0, t) == DDDMR_ERR_STATE && F.prepares + F.sweeps == 0);
  assert(b.measurePrepared(particles, like, qual) == DDDMR_ERR_STATE && F.measures == 0);
  assert(b.create(&ctx, 0.3, 0.05, 1.0, 6, 1000, 500, 60) == DDDMR_OK && b.setMap(map, ground, normals) == DDDMR_OK && b.ready());
  // ... and before a configuration neither
  assert(!b.prepared() && b.prepareObservation(flat, ls, t) == DDDMR_ERR_STATE && F.prepares == 0);
  F.config_rc = DDDMR_ERR_CAPACITY;
  assert(b.configureObservation(0.8, 3, 4000, 1600) == DDDMR_ERR_CAPACITY && F.configs == 1);
  assert(b.prepareObservation(0, t) == DDDMR_ERR_STATE && F.sweeps == 0);
  F.config_rc = DDDMR_OK;
  assert(b.configureObservation(0.8, 3, 400, 1600) == DDDMR_OK && F.configs == 2);
  assert(F.cfg.euc_cluster_distance == 0.8 && F.cfg.euc_cluster_min_size == 3 && F.cfg.max_flat_points == 400 &&
         F.cfg.max_less_sharp_points == 1600 && F.cfg.flags == 0 && F.cfg.reserved == 0);
  assert(!b.prepared() && b.measurePrepared(particles, like, qual) == DDDMR_ERR_STATE && F.measures == 0);

  // the two message clouds
  assert(b.prepareObservation(flat, ls, t, &st) == DDDMR_OK && b.prepared() && F.prepares == 1 && st.branch == 2 && st.n_flat_in == 2);
  assert(F.flat == &flat.points[0].x && F.n_flat == 2 && F.flat_stride == sizeof(PointXYZI) && F.ls == &ls.points[0].x && F.n_ls == 3 &&
         F.ls_stride == sizeof(PointXYZI));
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) assert(F.T[4 * r + c] == 10.0 * r + c);                          // row-major 3 x 4
  assert(b.prepareObservation(none, none, t) == DDDMR_OK && F.flat == nullptr && F.ls == nullptr && F.n_flat == 0 && F.n_ls == 0);
  // a sweep source
  std::memset(F.T, 0, sizeof(F.T));
  assert(b.prepareObservation(4, t, &st) == DDDMR_OK && F.sweeps == 1 && F.source == 4 && st.branch == 1 && F.T[6] == 12.0 && b.prepared());

  assert(b.measurePrepared(particles, like, qual, &qmin, &qmax) == DDDMR_OK && F.measures == 1);
  const float want1[7] = {2, 3, 4, 0.1f, 0.2f, 0.3f, 3};
  assert(F.states.size() == 21 && std::memcmp(&F.states[7], want1, sizeof(want1)) == 0);
  assert(like.size() == 3 && like[0] == 10.f && like[2] == 12.f && qual.size() == 3 && qual[1] == 0.2f);
  assert(qmin == 0.1f && qmax == 0.1f * 3.f);
  for (int code : {DDDMR_ERR_CAPACITY, DDDMR_ERR_STATE, DDDMR_ERR_HIP, DDDMR_ERR_BAD_ARG}) {     // a failing measure
    F.measure_rc = code;
    like[0] = 77.f; qmin = 5.f;
    assert(b.measurePrepared(particles, like, qual, &qmin, &qmax) == code && like[0] == 77.f && like.size() == 3 && qmin == 5.f && b.prepared());
  }
  F.measure_rc = DDDMR_OK;
  std::vector<State6DOF> nobody;
  assert(b.measurePrepared(nobody, like, qual) == DDDMR_OK && F.null_inputs && like.empty() && qual.empty());

  // a failing prepare: what the library still holds is the previous sweep's, so the bridge stops offering it
  const int measures = F.measures;
  F.prepare_rc = DDDMR_ERR_BAD_ARG;
  assert(b.prepareObservation(flat, ls, t) == DDDMR_ERR_BAD_ARG && !b.prepared());
  assert(b.measurePrepared(particles, like, qual) == DDDMR_ERR_STATE && F.measures == measures);
  F.prepare_rc = DDDMR_OK;
  assert(b.prepareObservation(flat, ls, t) == DDDMR_OK && b.prepared());
  F.sweep_rc = DDDMR_ERR_STATE;
  assert(b.prepareObservation(4, t) == DDDMR_ERR_STATE && !b.prepared());
  F.sweep_rc = DDDMR_OK;
  assert(b.prepareObservation(4, t) == DDDMR_OK && b.prepared());
  // a new configuration and a new create forget the observation
  assert(b.configureObservation(0.5, 2, 10, 20) == DDDMR_OK && !b.prepared() && F.cfg.euc_cluster_min_size == 2);
  assert(b.prepareObservation(flat, ls, t) == DDDMR_OK && b.prepared());
  assert(b.create(&ctx, 0.3, 0.05, 1.0, 6, 1000, 500, 60) == DDDMR_OK && !b.prepared());
  assert(b.setMap(map, ground, normals) == DDDMR_OK && !b.prepared());
  assert(b.prepareObservation(flat, ls, t) == DDDMR_ERR_STATE);                                   // the configuration went with the create
  std::printf("mcl observation bridge OK\n");
  return 0;
}
