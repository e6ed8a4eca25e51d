// mcl_observation_plan.hip.h -- the parts of MCL3dlNode::cbLeGoFeatureCloud (dddmr_mcl_3dl/src/mcl_3dl.cpp:340-443) that
// are arithmetic alone: which branch the two normal sums select, what a less-sharp point weighs in either branch, and
// the order EuclideanClusterExtraction::extract leaves the kept clusters in.  No HIP call and no HIP type, so that
// tests/cpp/mcl_observation_plan_test.cpp builds it with a plain host compiler; mcl_observation.hip.h calls the same
// functions from its kernels and from the host half of dddmr_rollout_mcl_prepare.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#ifdef __HIPCC__
#define MCLOBS_HD __host__ __device__ inline
#else
#define MCLOBS_HD inline
#endif

namespace dddmr {

constexpr uint32_t kMclObsClusters = 0, kMclObsXDominant = 1, kMclObsYDominant = 2;

// :351-360.  0 / 0 is NaN and selects neither; x / 0 is inf and selects dominant.
MCLOBS_HD uint32_t mclobs_branch(double sum_normal_x, double sum_normal_y) {
  if (sum_normal_x / sum_normal_y >= 1.6) return kMclObsXDominant;
  if (sum_normal_y / sum_normal_x >= 1.6) return kMclObsYDominant;
  return kMclObsClusters;
}

// :371-395.  The test is isnan(normal_x) in BOTH branches; the ratio is a float division widened to double.
MCLOBS_HD float mclobs_dominant_intensity(uint32_t branch, float normal_x, float normal_y, double sum_normal_x, double sum_normal_y) {
  if (normal_x != normal_x) return 1.0f;
  if (branch == kMclObsXDominant) {
    const double y2x = normal_y / normal_x;
    return y2x >= 0.5 ? (float)(0.05 * sum_normal_y / sum_normal_x) : 1.0f;
  }
  const double x2y = normal_x / normal_y;
  return x2y >= 0.5 ? (float)(0.05 * sum_normal_x / sum_normal_y) : 1.0f;
}

// :430-436.  (1.0 * size) / (1.0 * N), halved when size < euc_cluster_min_size + 1.
MCLOBS_HD float mclobs_cluster_intensity(uint32_t size, uint32_t n_points, int32_t min_size) {
  const double w = (1.0 * size) / (1.0 * n_points);
  return (int64_t)size < (int64_t)min_size + 1 ? (float)(w / 2.0) : (float)w;
}

// The kept clusters (min_size <= size; the maximum is the cloud's own size) arrive in creation order = ascending lowest
// point index; extract() ends with std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters), which compares
// sizes only (oracle/ASSUMPTIONS.md row 10).  This is that call on the same sizes: order[q] = which kept cluster is
// output q-th.  Equal sizes fall as libstdc++'s introsort leaves them.
struct MclObsItem { uint32_t size, ci; };
inline void mclobs_order_clusters(const uint32_t* kept_sizes, size_t n_kept, std::vector<uint32_t>& order) {
  std::vector<MclObsItem> v(n_kept);
  for (size_t c = 0; c < n_kept; ++c) v[c] = MclObsItem{kept_sizes[c], (uint32_t)c};
  std::sort(v.rbegin(), v.rend(), [](const MclObsItem& a, const MclObsItem& b) { return a.size < b.size; });
  order.resize(n_kept);
  for (size_t q = 0; q < n_kept; ++q) order[q] = v[q].ci;
}

}  // namespace dddmr
