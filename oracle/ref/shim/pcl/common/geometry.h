// Stand-in at the include path the reference uses (a_star_on_pre_graph.h).  ASSUMPTIONS.md row 20:
// pcl::geometry::squaredDistance is (p1 - p2).squaredNorm() on Vector3f maps, which Eigen reduces as
// (dx*dx + dy*dy) + dz*dz in float.  It includes and calls nothing under oracle/.
#ifndef REF_SHIM_PCL_COMMON_GEOMETRY_H_
#define REF_SHIM_PCL_COMMON_GEOMETRY_H_
#include "../../ref_pcl.hpp"
namespace pcl {
namespace geometry {
template <class PointT> inline float squaredDistance(const PointT& p1, const PointT& p2) {
  const float dx = p1.x - p2.x, dy = p1.y - p2.y, dz = p1.z - p2.z;
  return (dx * dx + dy * dy) + dz * dz;
}
}  // namespace geometry
}  // namespace pcl
#endif
