/*
 * ref_gp_driver.cpp -- drives the reference's own pre-graph planner (dddmr_global_planner/src/a_star_on_pre_graph.cpp
 * and dddmr_perception_3d/src/graph/static_graph.cpp, compiled unmodified from the reference checkout by
 * `make -C oracle ref` against the stand-ins in oracle/ref/shim/) through a C API, so tests/test_global_plan_pin_cpu.py
 * can hold tests/helpers/global_plan_ref.py against it bit for bit.
 *
 * TEST INFRASTRUCTURE ONLY.  Our code: it includes the reference's headers and calls its classes, and includes nothing
 * under oracle/.
 *
 * What runs is reference code: StaticGraph::insertNode (so a row's order is the std::set's own), A_Star_on_PreGraph's
 * constructor, setupTurningWeight, getPath, AstarListPreGraph, getThetaFromParent2Expanding.  What this file does in
 * their place: the cloud, the graph's edges (handed to insertNode in the order the caller's permutation gives) and
 * get_min_dGraphValue's array are filled from the arrays handed in.
 *
 * Private members (ASLS_, f_priority_set_, getThetaFromParent2Expanding) are reached without touching the reference's
 * text: an explicit template instantiation may name a private member, and the instantiated struct defines a friend
 * that hands the member pointer out (in the spirit of ref_peek.hpp).  All three were reachable.
 *
 * Lifetime: StaticGraph is copied by value and owns a raw pointer, so the planner's and the list's destructors would
 * delete the graph of the StaticGraph they were copied from.  Nothing here ever destroys a StaticGraph, an
 * A_Star_on_PreGraph or an AstarListPreGraph: each is allocated with new and left.  That is one leak per call, a few
 * kilobytes at the sizes of the pin's cases.
 */
#include <cstddef>
#include <cstdint>
#include <memory>
#include <set>
#include <vector>

#include <global_planner/a_star_on_pre_graph.h>

#define REF_API extern "C" __attribute__((visibility("default")))

namespace {

template <class Tag, typename Tag::type Member> struct Expose {
  friend typename Tag::type ref_gp_member(Tag) { return Member; }
};
struct ListTag {
  using type = AstarListPreGraph* A_Star_on_PreGraph::*;
  friend type ref_gp_member(ListTag);
};
struct SetTag {
  using type = std::set<f_p_> AstarListPreGraph::*;
  friend type ref_gp_member(SetTag);
};
struct ThetaTag {
  using type = double (A_Star_on_PreGraph::*)(pcl::PointXYZI, pcl::PointXYZI, pcl::PointXYZI);
  friend type ref_gp_member(ThetaTag);
};
template struct Expose<ListTag, &A_Star_on_PreGraph::ASLS_>;
template struct Expose<SetTag, &AstarListPreGraph::f_priority_set_>;
template struct Expose<ThetaTag, &A_Star_on_PreGraph::getThetaFromParent2Expanding>;

using Cloud = pcl::PointCloud<pcl::PointXYZI>;

A_Star_on_PreGraph* planner_of(Cloud::Ptr cloud, perception_3d::StaticGraph* graph,
                               std::shared_ptr<perception_3d::Perception3D_ROS> perception, double radius, double tw) {
  A_Star_on_PreGraph* p = new A_Star_on_PreGraph(cloud, *graph, perception, radius);   // never deleted, see the head
  p->setupTurningWeight(tw);
  return p;
}

}  // namespace

// One getPath.  xyzi[n][4]; row_start[n + 1], neighbour / weight[n_edges] (CSR); order[n_edges]: the edge handed to
// insertNode k-th; dgraph[n_dgraph] (get_min_dGraphValue's array).  Out: path[<= path_cap] with *path_len (0: getPath
// left the vector empty), and per node i < n the record read back after getPath: g, f, parent, opened, closed;
// *set_size: what f_priority_set_ holds at the end.  Returns 0; -1 an index out of range; -2 a path longer than
// path_cap.
REF_API int ref_gp_plan(const float* xyzi, std::size_t n, const uint32_t* row_start, const uint32_t* neighbour,
                        const float* weight, const uint32_t* order, std::size_t n_edges, const double* dgraph,
                        std::size_t n_dgraph, double radius, double inscribed_radius, double descending_rate,
                        double max_obstacle_distance, double turning_weight, uint32_t start, uint32_t goal, uint32_t* path,
                        std::size_t path_cap, std::size_t* path_len, float* g, float* f, uint32_t* parent,
                        uint8_t* opened, uint8_t* closed, std::size_t* set_size) {
  if (start >= n || goal >= n || row_start[n] != n_edges) return -1;
  std::vector<uint32_t> source(n_edges);
  for (std::size_t i = 0; i < n; ++i) {
    if (row_start[i] > row_start[i + 1] || row_start[i + 1] > n_edges) return -1;
    for (uint32_t e = row_start[i]; e < row_start[i + 1]; ++e) source[e] = static_cast<uint32_t>(i);
  }
  for (std::size_t e = 0; e < n_edges; ++e)
    if (neighbour[e] >= n || neighbour[e] >= n_dgraph || order[e] >= n_edges) return -1;

  Cloud::Ptr cloud(new Cloud);
  for (std::size_t i = 0; i < n; ++i) {
    pcl::PointXYZI p;
    p.x = xyzi[4 * i];
    p.y = xyzi[4 * i + 1];
    p.z = xyzi[4 * i + 2];
    p.intensity = xyzi[4 * i + 3];
    cloud->push_back(p);
  }
  perception_3d::StaticGraph* graph = new perception_3d::StaticGraph;                    // never deleted, see the head
  for (std::size_t k = 0; k < n_edges; ++k) {
    const uint32_t e = order[k];
    edge_t edge(neighbour[e], weight[e]);
    graph->insertNode(source[e], edge);
  }
  auto perception = std::make_shared<perception_3d::Perception3D_ROS>();
  perception->min_dgraph.assign(dgraph, dgraph + n_dgraph);
  perception->getGlobalUtils()->inscribed_radius = inscribed_radius;
  perception->getGlobalUtils()->inflation_descending_rate = descending_rate;
  perception->getGlobalUtils()->max_obstacle_distance = max_obstacle_distance;

  A_Star_on_PreGraph* planner = planner_of(cloud, graph, perception, radius, turning_weight);
  std::vector<unsigned int> got;
  planner->getPath(start, goal, got);

  *path_len = got.size();
  if (got.size() > path_cap) return -2;
  for (std::size_t i = 0; i < got.size(); ++i) path[i] = got[i];
  AstarListPreGraph* list = planner->*ref_gp_member(ListTag());
  for (std::size_t i = 0; i < n; ++i) {
    const NodePreGraph_t r = list->getNode(static_cast<unsigned int>(i));
    g[i] = r.g;
    f[i] = r.f;
    parent[i] = r.parent_index;
    opened[i] = r.is_opened;
    closed[i] = r.is_closed;
  }
  *set_size = (list->*ref_gp_member(SetTag())).size();
  return 0;
}

// getThetaFromParent2Expanding(parent, current, expanding) for n triples of x, y: xy[n][6] -> theta[n]
REF_API void ref_gp_theta(const float* xy, std::size_t n, double* theta) {
  static A_Star_on_PreGraph* planner = nullptr;                                          // one for the process, never deleted
  if (!planner)
    planner = planner_of(Cloud::Ptr(new Cloud), new perception_3d::StaticGraph,
                         std::make_shared<perception_3d::Perception3D_ROS>(), 0.5, 0.0);
  const ThetaTag::type fn = ref_gp_member(ThetaTag());
  for (std::size_t i = 0; i < n; ++i) {
    pcl::PointXYZI p, c, e;
    p.x = xy[6 * i];
    p.y = xy[6 * i + 1];
    c.x = xy[6 * i + 2];
    c.y = xy[6 * i + 3];
    e.x = xy[6 * i + 4];
    e.y = xy[6 * i + 5];
    theta[i] = (planner->*fn)(p, c, e);
  }
}
