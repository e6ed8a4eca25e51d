// Stand-in at the include path the reference uses (a_star_on_pre_graph.h): the type of kdtree_lethal_, which only
// isLineOfSightClear reads and getPath never reaches.  No ASSUMPTIONS.md row: radiusSearch finds nothing and no pinned
// path calls it.  It includes and calls nothing under oracle/.
#ifndef REF_SHIM_NANOFLANN_PCL_HPP_
#define REF_SHIM_NANOFLANN_PCL_HPP_
#include <memory>
#include <vector>
namespace nanoflann {
template <class PointT> class KdTreeFLANN {
 public:
  using Ptr = std::shared_ptr<KdTreeFLANN<PointT>>;
  int radiusSearch(const PointT&, double, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const {
    k_indices.clear();
    k_sqr_distances.clear();
    return 0;
  }
};
}  // namespace nanoflann
#endif
