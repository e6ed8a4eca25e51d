// Stand-in at the include path the reference uses (a_star_on_pre_graph.h): what A_Star_on_PreGraph::getPath asks of
// Perception3D_ROS.  StaticGraph is the reference's own class (its header is included below and its unit is compiled).
// ASSUMPTIONS.md row 21: get_min_dGraphValue(i) is a plain read of the stacked minimum for node i; here it is served
// from an array that the driver fills, so the stack's minimum itself (stacked_perception.cpp) stays unpinned.
// getGlobalUtils() hands out the three values getPath reads.  It includes and calls nothing under oracle/.
#ifndef REF_SHIM_PERCEPTION_3D_ROS_H_
#define REF_SHIM_PERCEPTION_3D_ROS_H_
#include <algorithm>
#include <memory>
#include <vector>
#include "../ref_pcl.hpp"
#include <perception_3d/static_graph.h>
namespace perception_3d {
class GlobalUtils {
 public:
  double inscribed_radius = 0.0, inflation_descending_rate = 0.0, max_obstacle_distance = 0.0;
  double getInscribedRadius() { return inscribed_radius; }
  double getInflationDescendingRate() { return inflation_descending_rate; }
  double getMaxObstacleDistance() { return max_obstacle_distance; }
};
class Perception3D_ROS {
 public:
  std::shared_ptr<GlobalUtils> getGlobalUtils() { return utils_; }
  double get_min_dGraphValue(unsigned int index) { return min_dgraph.at(index); }
  std::vector<double> min_dgraph;
 private:
  std::shared_ptr<GlobalUtils> utils_ = std::make_shared<GlobalUtils>();
};
}  // namespace perception_3d
#endif
