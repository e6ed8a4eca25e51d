// Functional stand-in for the PCL surface of the reference's rollout units: PointCloud, PointXYZ(I),
// transformPointCloud, getMinMax3D and KdTreeFLANN (exact search).  Written from the libraries' documented behaviour;
// it includes and calls nothing under oracle/.
#ifndef REF_SHIM_PCL_HPP_
#define REF_SHIM_PCL_HPP_
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <cstddef>
#include <memory>
#include <numeric>
#include <vector>
#include "ref_eigen.hpp"

// Point-type declaration macros: only enough for mcl_3dl's utilities.h to declare its pose point type, which the
// particle-measure unit never instantiates (no ASSUMPTIONS.md row: no arithmetic behind them).
#define PCL_ADD_POINT4D float x; float y; float z; float ref_shim_pad_;
#define PCL_ADD_INTENSITY float intensity
#define EIGEN_MAKE_ALIGNED_OPERATOR_NEW
#define EIGEN_ALIGN16 __attribute__((aligned(16)))
#define POINT_CLOUD_REGISTER_POINT_STRUCT(name, fields)

namespace pcl {
struct PointXYZ { float x = 0.f, y = 0.f, z = 0.f; };
struct PointXYZI { float x = 0.f, y = 0.f, z = 0.f, intensity = 0.f; };
// pcl::Normal: three floats read by name (no ASSUMPTIONS.md row: plain storage)
struct Normal { float normal_x = 0.f, normal_y = 0.f, normal_z = 0.f, curvature = 0.f; };

template <class PointT> class PointCloud {
 public:
  using Ptr = std::shared_ptr<PointCloud<PointT>>;
  using ConstPtr = std::shared_ptr<const PointCloud<PointT>>;
  std::vector<PointT> points;
  unsigned int width = 0, height = 1;
  bool is_dense = true;
  void push_back(const PointT& p) { points.push_back(p); width = (unsigned int)points.size(); height = 1; }
  std::size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
  void clear() { points.clear(); width = 0; }
  PointT& operator[](std::size_t i) { return points[i]; }
  const PointT& operator[](std::size_t i) const { return points[i]; }
};

// Row 4: transformPointCloud(in, out, Affine3d) with SSE/AVX off: per point, in double, left to right,
// x' = float(m00 x + m01 y + m02 z + m03)
template <class PointT>
void transformPointCloud(const PointCloud<PointT>& in, PointCloud<PointT>& out, const Eigen::Affine3d& tf) {
  if (&in != &out) out = in;
  for (auto& p : out.points) {
    const double q[3] = {p.x, p.y, p.z};
    p.x = static_cast<float>(tf(0, 0) * q[0] + tf(0, 1) * q[1] + tf(0, 2) * q[2] + tf(0, 3));
    p.y = static_cast<float>(tf(1, 0) * q[0] + tf(1, 1) * q[1] + tf(1, 2) * q[2] + tf(1, 3));
    p.z = static_cast<float>(tf(2, 0) * q[0] + tf(2, 1) * q[1] + tf(2, 2) * q[2] + tf(2, 3));
  }
}

// Row 5: getMinMax3D = per-axis min / max over the points, starting from +-FLT_MAX
template <class PointT> void getMinMax3D(const PointCloud<PointT>& c, PointT& mn, PointT& mx) {
  mn.x = mn.y = mn.z = FLT_MAX;
  mx.x = mx.y = mx.z = -FLT_MAX;
  for (const auto& p : c.points) {
    mn.x = std::min(mn.x, p.x); mn.y = std::min(mn.y, p.y); mn.z = std::min(mn.z, p.z);
    mx.x = std::max(mx.x, p.x); mx.y = std::max(mx.y, p.y); mx.z = std::max(mx.z, p.z);
  }
}

// KdTreeFLANN as an exact search with FLANN's arithmetic.  radiusSearch gathers candidates from a uniform grid (cells
// of the first radius asked for, the box [q - 1.01 r, q + 1.01 r] in double) and keeps those that pass FLANN's own
// float test below, so the result is the exhaustive one:
//  row 2: squared distance = L2_Simple<float>, diff*diff accumulated in x, y, z order in float;
//  row 1: radiusSearch(p, double r) hands static_cast<float>(r * r) to FLANN, which keeps a point iff dist < r2;
//         results sorted by distance (PCL's default), equal distances by index;
//  row 3: nearestKSearch is exact (eps = 0); on equal distances the lowest index;
//  row 19: radiusSearch(..., max_nn) with 0 < max_nn < cloud size keeps the max_nn closest of the points inside the
//         radius (FLANN's KNNRadiusResultSet), max_nn = 0 or >= the cloud size keeps all; both output vectors are
//         resized to the count kept (to 0 when nothing is inside the radius).
template <class PointT> class KdTreeFLANN {
 public:
  using Ptr = std::shared_ptr<KdTreeFLANN<PointT>>;
  using PointCloudConstPtr = std::shared_ptr<const PointCloud<PointT>>;
  void setInputCloud(const PointCloudConstPtr& cloud) { cloud_ = cloud; cell_ = 0.0; grid_.clear(); }
  int radiusSearch(const PointT& p, double radius, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances,
                   unsigned int max_nn = 0) const {
    const float r2 = static_cast<float>(radius * radius);
    k_indices.clear();
    k_sqr_distances.clear();
    if (cell_ == 0.0) build_grid(radius > 0.0 ? radius : 1.0);
    std::vector<std::pair<float, int>> hits;
    const double q[3] = {p.x, p.y, p.z}, reach = 1.01 * radius;
    int64_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = (int64_t)std::floor((q[a] - reach) / cell_);
      hi[a] = (int64_t)std::floor((q[a] + reach) / cell_);
    }
    for (int64_t x = lo[0]; x <= hi[0]; ++x)
      for (int64_t y = lo[1]; y <= hi[1]; ++y)
        for (int64_t z = lo[2]; z <= hi[2]; ++z) {
          auto it = grid_.find(key(x, y, z));
          if (it == grid_.end()) continue;
          for (int i : it->second) {
            const float d = l2_simple(cloud_->points[i], p);
            if (d < r2) hits.push_back({d, i});
          }
        }
    std::sort(hits.begin(), hits.end());
    if (max_nn != 0 && max_nn < cloud_->points.size() && hits.size() > max_nn) hits.resize(max_nn);
    for (auto& h : hits) { k_indices.push_back(h.second); k_sqr_distances.push_back(h.first); }
    return (int)hits.size();
  }
  int nearestKSearch(const PointT& p, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const {
    std::vector<std::pair<float, int>> all;
    for (std::size_t i = 0; i < cloud_->points.size(); ++i) all.push_back({l2_simple(cloud_->points[i], p), (int)i});
    const std::size_t n = std::min<std::size_t>((std::size_t)std::max(k, 0), all.size());
    std::partial_sort(all.begin(), all.begin() + n, all.end());
    k_indices.resize(n);
    k_sqr_distances.resize(n);
    for (std::size_t i = 0; i < n; ++i) { k_indices[i] = all[i].second; k_sqr_distances[i] = all[i].first; }
    return (int)n;
  }

 private:
  static float l2_simple(const PointT& a, const PointT& b) {
    float result = 0.f, diff;
    diff = a.x - b.x; result += diff * diff;
    diff = a.y - b.y; result += diff * diff;
    diff = a.z - b.z; result += diff * diff;
    return result;
  }
  static uint64_t key(int64_t x, int64_t y, int64_t z) {
    return ((uint64_t)(x & 0x1FFFFF) << 42) | ((uint64_t)(y & 0x1FFFFF) << 21) | (uint64_t)(z & 0x1FFFFF);
  }
  void build_grid(double cell) const {
    cell_ = cell;
    for (std::size_t i = 0; i < cloud_->points.size(); ++i) {
      const auto& q = cloud_->points[i];
      grid_[key((int64_t)std::floor(q.x / cell_), (int64_t)std::floor(q.y / cell_), (int64_t)std::floor(q.z / cell_))]
          .push_back((int)i);
    }
  }
  PointCloudConstPtr cloud_;
  mutable double cell_ = 0.0;
  mutable std::unordered_map<uint64_t, std::vector<int>> grid_;
};
}  // namespace pcl
#endif
