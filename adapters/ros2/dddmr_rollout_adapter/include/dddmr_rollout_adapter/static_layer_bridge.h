// static_layer_bridge.h -- the perception_3d side of the static layer and the no-entry layer on the device: what a
// patched StaticLayer / NoEntryLayer calls instead of searching its kd-trees node by node.
//
//   StaticLayer::selfClear            (plugins/static_layer.cpp:201-231)     -> regenerate(ground, map)
//   sGraph_ptr_->getEdge(node)        (src/graph/static_graph.cpp:58-60)     -> edges(node), the reference's edges_t
//   StaticLayer::get_dGraphValue      (plugins/static_layer.cpp:429-434)     -> dGraphValue(i)
//   NoEntryLayer's inflation          (plugins/no_entry_layer.cpp:265-283)   -> setZones(...), zoneDGraphValue(i)
//   StackedPerception's layers        (src/stacked_perception.cpp:114-126)   -> bindToStack(which, slot)
//
// Everything here is a template over the cloud types it is handed (pcl::PointCloud<pcl::PointXYZI>): this header
// includes neither PCL nor ROS, so it is compiled and run in a plain C++ toolchain
// (tests/cpp/static_layer_bridge_test.cpp).  After a regenerate that returned DDDMR_OK the graph and the dGraph are held
// in host memory, so edges() and dGraphValue() cost no call into the library: the global planner's A* asks for them node
// by node (a_star_on_pre_graph.cpp:218-220).  The node weights (insertWeight, static_layer.cpp:417) stay with the plugin.
#ifndef DDDMR_ROLLOUT_ADAPTER_STATIC_LAYER_BRIDGE_H_
#define DDDMR_ROLLOUT_ADAPTER_STATIC_LAYER_BRIDGE_H_

#include <cstdint>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "dddmr_rollout.h"

namespace dddmr_rollout_adapter
{

class StaticLayerBridge
{
public:
  typedef std::pair<unsigned int, float> edge_t;        // perception_3d/static_graph.h:39-40
  typedef std::set<edge_t> edges_t;

  int create(dddmr_rollout_ctx * ctx, const dddmr_static_layer_config & cfg)
  {
    ctx_ = nullptr;
    forget();
    if (!ctx) {return DDDMR_ERR_BAD_ARG;}
    const int rc = dddmr_rollout_static_layer_create(ctx, &cfg);
    if (rc != DDDMR_OK) {return rc;}
    ctx_ = ctx;                      // only after a successful create
    return DDDMR_OK;
  }
  bool created() const {return ctx_ != nullptr;}
  bool ready() const {return ctx_ != nullptr && ready_;}          // is_static_layer_ready_
  bool zonesReady() const {return ready() && zones_ready_;}
  size_t nodes() const {return ready_ ? dgraph_.size() - 1 : 0;}
  size_t edgeCount() const {return neighbour_.size();}

  // One selfClear regeneration from pcl_ground_ and pcl_map_, then the graph and the dGraph come to the host once.  A
  // refused or failed call keeps what the last successful one left (the library does the same).
  template<class Cloud>
  int regenerate(const Cloud & ground, const Cloud & map, dddmr_static_layer_stats * stats = nullptr)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    const size_t ng = ground.points.size(), nm = map.points.size();
    dddmr_static_layer_stats st;
    std::memset(&st, 0, sizeof(st));
    int rc = dddmr_rollout_static_layer_build(
      ctx_, ng ? &ground.points[0].x : nullptr, ng, ng ? sizeof(ground.points[0]) : 12, nm ? &map.points[0].x : nullptr, nm,
      nm ? sizeof(map.points[0]) : 12, &st);
    if (stats) {*stats = st;}
    if (rc != DDDMR_OK) {return rc;}
    // (the build is in: what is held here is stale whatever the getters answer)
    forget();
    std::vector<uint32_t> row_start(ng + 1), neighbour((size_t)st.n_edges);
    std::vector<float> weight((size_t)st.n_edges);
    std::vector<double> dgraph(ng + 1);
    size_t n_edges = 0;
    rc = dddmr_rollout_static_layer_get_graph(
      ctx_, row_start.data(), neighbour.empty() ? nullptr : neighbour.data(), weight.empty() ? nullptr : weight.data(), neighbour.size(), &n_edges);
    if (rc != DDDMR_OK) {return rc;}
    if (n_edges != neighbour.size()) {return DDDMR_ERR_STATE;}
    rc = dddmr_rollout_static_layer_get_dgraph(ctx_, dgraph.data(), dgraph.size());
    if (rc != DDDMR_OK) {return rc;}
    row_start_.swap(row_start); neighbour_.swap(neighbour); weight_.swap(weight); dgraph_.swap(dgraph);
    ready_ = true;
    return DDDMR_OK;
  }

  // StaticGraph::getEdge: the node's (neighbour, weight) pairs as the reference's std::set; empty for an unknown node
  edges_t edges(unsigned int node) const
  {
    edges_t out;
    if (!ready_ || (size_t)node + 1 >= row_start_.size()) {return out;}
    for (uint32_t e = row_start_[node]; e < row_start_[node + 1]; ++e) {
      out.insert(out.end(), edge_t(neighbour_[e], weight_[e]));      // (ascending neighbour index: already the set's order)
    }
    return out;
  }

  // StaticLayer::get_dGraphValue: 0.0 for an index the dGraph does not hold (:431-432)
  double dGraphValue(unsigned int index) const
  {
    return ready_ && index < dgraph_.size() ? dgraph_[index] : 0.0;
  }

  // The enabled zones' clouds, concatenated here (none enabled: every value becomes max_obstacle_distance).
  // Zones: any range of pointers or references to clouds with .points (std::vector<const Cloud *>).
  template<class Cloud>
  int setZones(const std::vector<const Cloud *> & enabled_zones, double inflation_distance, dddmr_static_layer_stats * stats = nullptr)
  {
    if (!ctx_ || !ready_) {return DDDMR_ERR_STATE;}               // (the library refuses zones before the first build, too)
    std::vector<float> xyz;
    for (const Cloud * z : enabled_zones) {
      if (!z) {continue;}
      for (const auto & p : z->points) {
        xyz.push_back(p.x); xyz.push_back(p.y); xyz.push_back(p.z);
      }
    }
    const size_t n = xyz.size() / 3;
    int rc = dddmr_rollout_static_layer_set_zones(ctx_, n ? xyz.data() : nullptr, n, 12, inflation_distance, stats);
    if (rc != DDDMR_OK) {return rc;}
    zones_ready_ = false;
    std::vector<double> z(dgraph_.size());
    rc = dddmr_rollout_static_layer_get_zone_dgraph(ctx_, z.data(), z.size());
    if (rc != DDDMR_OK) {return rc;}
    zone_dgraph_.swap(z);
    zones_ready_ = true;
    return DDDMR_OK;
  }
  double zoneDGraphValue(unsigned int index) const
  {
    return zones_ready_ && index < zone_dgraph_.size() ? zone_dgraph_[index] : 0.0;
  }

  // which: 0 the static dGraph, 1 the no-entry dGraph -> host slot `slot` of the context's perception stack, device to
  // device; the next StackBridge update shows the change
  int bindToStack(int32_t which, int32_t slot)
  {
    if (!ctx_) {return DDDMR_ERR_STATE;}
    return dddmr_rollout_static_layer_bind(ctx_, which, slot);
  }

private:
  void forget()
  {
    ready_ = false; zones_ready_ = false;
    row_start_.clear(); neighbour_.clear(); weight_.clear(); dgraph_.clear(); zone_dgraph_.clear();
  }
  dddmr_rollout_ctx * ctx_ = nullptr;
  bool ready_ = false, zones_ready_ = false;
  std::vector<uint32_t> row_start_, neighbour_;
  std::vector<float> weight_;
  std::vector<double> dgraph_, zone_dgraph_;
};

}  // namespace dddmr_rollout_adapter
#endif
