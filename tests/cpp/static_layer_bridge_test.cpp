// StaticLayerBridge (static_layer_bridge.h) WITHOUT ROS, PCL or a GPU: stand-in cloud types against a fake C-ABI that
// records the calls and serves a small graph.  Checked: nothing is sent before a create; a build's first-point addresses,
// counts and record sizes; empty clouds pass no pointer; the getters are asked once per regeneration with the sizes the
// build reported; edges() is the reference's std::set in ascending neighbour order with the weights; dGraphValue's 0.0
// for an unknown index; a refused build keeps the earlier graph; setZones concatenates the enabled zones as packed x y z,
// is refused before the first regeneration and passes "no zone" as zero points; bindToStack hands its arguments on.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dddmr_rollout_adapter/static_layer_bridge.h"

struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };          // 32 bytes, as PCL lays it out
struct Cloud { std::vector<PointXYZI> points; };

struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  int create_rc = DDDMR_OK, build_rc = DDDMR_OK, zones_rc = DDDMR_OK, bind_rc = DDDMR_OK;
  int creates = 0, builds = 0, graphs = 0, dgraphs = 0, zones = 0, zone_gets = 0, binds = 0;
  dddmr_static_layer_config cfg;
  const float *ground = nullptr, *map = nullptr;
  size_t n_ground = 0, n_map = 0, ground_stride = 0, map_stride = 0, edge_capacity = 0, dgraph_capacity = 0;
  std::vector<float> zone_xyz;
  size_t zone_stride = 0;
  bool zone_null = false;
  double inflation = 0;
  int32_t which = -1, slot = -1;
  // what the fake serves: 3 nodes, rows {0, 1}, {0, 1, 2}, {2}
  std::vector<uint32_t> row_start{0, 2, 5, 6}, neighbour{0, 1, 0, 1, 2, 2};
  std::vector<float> weight{0.f, 1.5f, 1.5f, 0.f, 0.75f, 0.f};
  std::vector<double> dgraph{9999.0, 0.25, 0.375, 9999.0}, zone{9999.0, 9999.0, 0.5, 9999.0};
} F;
extern "C" {
int dddmr_rollout_static_layer_create(dddmr_rollout_ctx*, const dddmr_static_layer_config* cfg) {
  ++F.creates; F.cfg = *cfg;
  return F.create_rc; }
int dddmr_rollout_static_layer_build(dddmr_rollout_ctx*, const float* ground, size_t n_ground, size_t ground_stride, const float* map, size_t n_map,
                                     size_t map_stride, dddmr_static_layer_stats* stats) {
  ++F.builds;
  F.ground = ground; F.n_ground = n_ground; F.ground_stride = ground_stride; F.map = map; F.n_map = n_map; F.map_stride = map_stride;
  if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->n_edges = F.neighbour.size(); stats->n_ground = (uint32_t)n_ground; }
  return F.build_rc; }
int dddmr_rollout_static_layer_get_graph(dddmr_rollout_ctx*, uint32_t* row_start_out, uint32_t* neighbour_out, float* weight_out, size_t edge_capacity,
                                         size_t* n_edges) {
  ++F.graphs; F.edge_capacity = edge_capacity;
  *n_edges = F.neighbour.size();
  if ((neighbour_out || weight_out) && edge_capacity < F.neighbour.size()) return DDDMR_ERR_CAPACITY;
  if (row_start_out) std::memcpy(row_start_out, F.row_start.data(), F.row_start.size() * 4);
  if (neighbour_out) std::memcpy(neighbour_out, F.neighbour.data(), F.neighbour.size() * 4);
  if (weight_out) std::memcpy(weight_out, F.weight.data(), F.weight.size() * 4);
  return DDDMR_OK; }
int dddmr_rollout_static_layer_get_dgraph(dddmr_rollout_ctx*, double* values_out, size_t capacity) {
  ++F.dgraphs; F.dgraph_capacity = capacity;
  if (capacity < F.dgraph.size()) return DDDMR_ERR_CAPACITY;
  std::memcpy(values_out, F.dgraph.data(), F.dgraph.size() * 8);
  return DDDMR_OK; }
int dddmr_rollout_static_layer_set_zones(dddmr_rollout_ctx*, const float* zone_xyz, size_t n_points, size_t stride, double inflation_distance,
                                         dddmr_static_layer_stats* stats) {
  ++F.zones; F.zone_null = zone_xyz == nullptr; F.zone_stride = stride; F.inflation = inflation_distance;
  F.zone_xyz.assign(zone_xyz, zone_xyz + (zone_xyz ? 3 * n_points : 0));
  if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->n_zone_points = (uint32_t)n_points; }
  return F.zones_rc; }
int dddmr_rollout_static_layer_get_zone_dgraph(dddmr_rollout_ctx*, double* values_out, size_t capacity) {
  ++F.zone_gets;
  if (capacity < F.zone.size()) return DDDMR_ERR_CAPACITY;
  std::memcpy(values_out, F.zone.data(), F.zone.size() * 8);
  return DDDMR_OK; }
int dddmr_rollout_static_layer_bind(dddmr_rollout_ctx*, int32_t which, int32_t slot) {
  ++F.binds; F.which = which; F.slot = slot;
  return F.bind_rc; }
}

using namespace dddmr_rollout_adapter;

int main() {
  dddmr_rollout_ctx ctx{0};
  StaticLayerBridge b;
  Cloud ground, map, none;
  ground.points.resize(3);
  map.points.resize(7);
  dddmr_static_layer_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.max_ground_points = 100; cfg.max_map_points = 200; cfg.max_edges = 1000; cfg.radius_of_ground_connection = 1.5;
  cfg.max_obstacle_distance = 9999.0;
  std::vector<const Cloud*> no_zone;

  // nothing before a create
  assert(b.regenerate(ground, map) == DDDMR_ERR_STATE && b.setZones(no_zone, 0.5) == DDDMR_ERR_STATE && b.bindToStack(0, 0) == DDDMR_ERR_STATE);
  assert(F.builds == 0 && F.zones == 0 && F.binds == 0 && !b.created() && !b.ready());
  assert(b.create(nullptr, cfg) == DDDMR_ERR_BAD_ARG && F.creates == 0);
  F.create_rc = DDDMR_ERR_BAD_ARG;
  assert(b.create(&ctx, cfg) == DDDMR_ERR_BAD_ARG && !b.created());
  F.create_rc = DDDMR_OK;
  assert(b.create(&ctx, cfg) == DDDMR_OK && b.created() && !b.ready() && F.creates == 2);
  assert(F.cfg.max_edges == 1000 && F.cfg.radius_of_ground_connection == 1.5);
  assert(b.edges(0).empty() && b.dGraphValue(0) == 0.0 && b.nodes() == 0);
  assert(b.setZones(no_zone, 0.5) == DDDMR_ERR_STATE && F.zones == 0);      // no regeneration yet

  // a regeneration: addresses, counts, record sizes; the getters once each, with the sizes the build reported
  dddmr_static_layer_stats st;
  assert(b.regenerate(ground, map, &st) == DDDMR_OK && b.ready() && st.n_edges == 6 && F.builds == 1 && F.graphs == 1 && F.dgraphs == 1);
  assert(F.ground == &ground.points[0].x && F.n_ground == 3 && F.ground_stride == 32 && F.map == &map.points[0].x && F.n_map == 7 && F.map_stride == 32);
  assert(F.edge_capacity == 6 && F.dgraph_capacity == 4 && b.nodes() == 3 && b.edgeCount() == 6);
  const StaticLayerBridge::edges_t e1 = b.edges(1);
  assert(e1.size() == 3);
  auto it = e1.begin();
  assert(it->first == 0 && it->second == 1.5f);
  ++it;
  assert(it->first == 1 && it->second == 0.f);
  ++it;
  assert(it->first == 2 && it->second == 0.75f);
  assert(b.edges(0).size() == 2 && b.edges(2).size() == 1 && b.edges(3).empty() && b.edges(4000000000u).empty());
  assert(b.dGraphValue(1) == 0.25 && b.dGraphValue(2) == 0.375 && b.dGraphValue(3) == 9999.0 && b.dGraphValue(4) == 0.0);
  assert(F.graphs == 1 && F.dgraphs == 1);                                  // edges() and dGraphValue() asked nothing
  // an empty map passes no pointer
  assert(b.regenerate(ground, none) == DDDMR_OK && F.map == nullptr && F.n_map == 0 && F.map_stride == 12 && F.graphs == 2);
  // a refused build keeps the earlier graph
  F.build_rc = DDDMR_ERR_CAPACITY;
  assert(b.regenerate(ground, map, &st) == DDDMR_ERR_CAPACITY && st.n_edges == 6 && b.ready() && b.edges(1).size() == 3 && F.graphs == 2);
  F.build_rc = DDDMR_OK;

  // zones: the enabled clouds concatenated as packed x y z; none enabled is zero points and no pointer
  Cloud za, zb;
  za.points.resize(2);
  zb.points.resize(1);
  za.points[0].x = 1.f; za.points[0].y = 2.f; za.points[0].z = 3.f;
  za.points[1].x = 4.f; za.points[1].y = 5.f; za.points[1].z = 6.f;
  zb.points[0].x = 7.f; zb.points[0].y = 8.f; zb.points[0].z = 9.f;
  std::vector<const Cloud*> zones{&za, nullptr, &zb};
  assert(b.setZones(zones, 0.6, &st) == DDDMR_OK && b.zonesReady() && st.n_zone_points == 3 && F.zones == 1 && F.zone_gets == 1);
  assert(F.zone_stride == 12 && F.inflation == 0.6 && F.zone_xyz == std::vector<float>({1, 2, 3, 4, 5, 6, 7, 8, 9}));
  assert(b.zoneDGraphValue(2) == 0.5 && b.zoneDGraphValue(0) == 9999.0 && b.zoneDGraphValue(9) == 0.0);
  assert(b.setZones(no_zone, 0.6) == DDDMR_OK && F.zone_null && F.zone_xyz.empty() && F.zones == 2);
  F.zones_rc = DDDMR_ERR_BAD_ARG;
  assert(b.setZones(zones, -1.0) == DDDMR_ERR_BAD_ARG && b.zonesReady() && F.zone_gets == 2);      // a refusal keeps the earlier values
  F.zones_rc = DDDMR_OK;
  // a regeneration drops the zones' values, as the library does
  assert(b.regenerate(ground, map) == DDDMR_OK && !b.zonesReady() && b.zoneDGraphValue(2) == 0.0);

  // the binding
  assert(b.bindToStack(1, 3) == DDDMR_OK && F.binds == 1 && F.which == 1 && F.slot == 3);
  F.bind_rc = DDDMR_ERR_STATE;
  assert(b.bindToStack(0, 0) == DDDMR_ERR_STATE && F.binds == 2);

  // a new create forgets the graph
  assert(b.create(&ctx, cfg) == DDDMR_OK && !b.ready() && b.edges(1).empty());
  std::printf("static layer bridge OK\n");
  return 0;
}
