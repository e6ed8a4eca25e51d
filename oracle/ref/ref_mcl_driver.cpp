/*
 * ref_mcl_driver.cpp -- drives mcl_3dl's own LidarMeasurementModelLikelihood (lidar_measurement_model_likelihood.cpp
 * compiled from the reference checkout by `make -C oracle ref`, with the reference's state_6dof.h / quat.h / vec3.h /
 * pf.h, against the stand-ins in oracle/ref/shim/) through a C API, so tests/test_mcl_measure_pin_cpu.py can hold
 * tests/helpers/mcl_measure_ref.py against it bit for bit.
 *
 * TEST INFRASTRUCTURE ONLY.  Our code: it includes the reference's headers and calls its classes, and includes nothing
 * under oracle/.
 *
 * What runs is reference code: loadConfig() (the four values reach the class through its own declare_parameter /
 * get_parameter calls and its own narrowing into float members), measure(), State6DOF::transform with Quat and Vec3.
 * What this file does in their place:
 *  - the parameter file: the four config values are written into the node's parameter map under the reference's names;
 *  - the kd-trees and the normal cloud of sub_maps: built here from the arrays handed in;
 *  - the trace: the library is built with -DREF_SHIM_TRACE_DEBUG, so the stand-in's RCLCPP_DEBUG leaves one record per
 *    call of measure()'s own debug lines; they are read back per particle below;
 *  - the lambda of mcl_3dl.cpp:476-498 (inside the node class): RESTATED in ref_mcl_quality_minmax, labelled as such.
 */
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <mcl_3dl/lidar_measurement_models/lidar_measurement_model_likelihood.h>

#define REF_API extern "C" __attribute__((visibility("default")))

namespace {

using Cloud = pcl::PointCloud<mcl_3dl::pcl_t>;

Cloud::Ptr cloud_of(const float* p, std::size_t n, std::size_t stride, bool intensity) {
  Cloud::Ptr c(new Cloud);
  for (std::size_t i = 0; i < n; ++i) {
    mcl_3dl::pcl_t q;
    q.x = p[i * stride];
    q.y = p[i * stride + 1];
    q.z = p[i * stride + 2];
    q.intensity = intensity ? p[i * stride + 3] : 0.f;
    c->push_back(q);
  }
  return c;
}

mcl_3dl::State6DOF state_of(const float* s) {
  return mcl_3dl::State6DOF(mcl_3dl::Vec3(s[0], s[1], s[2]), mcl_3dl::Quat(s[3], s[4], s[5], s[6]));
}

}  // namespace

enum { REF_MCL_TRACE_WIDTH = 8 };   // n_ground, avg_nx, avg_ny, avg_nz, roll, pitch, yaw, roll_diff
enum { REF_MCL_BRANCH_UNTRUSTED = 0, REF_MCL_BRANCH_STEEP = 1, REF_MCL_BRANCH_ROLL = 2 };

// likelihood[N], quality[N]; trace[N][8] doubles (what measure()'s debug lines carried, NaN where the particle's branch
// logged none); branch[N]: 0 "Not enough ground information" logged, 1 the averaged normals logged and nothing after
// (the 3x test took 0.2), 2 R/P/Y and roll diff logged.  Returns 0, or -(1 + particle) when a particle's records are
// not one of those three shapes.
REF_API int ref_mcl_measure(double match_dist_min, double match_dist_flat, double radius_of_ground_search,
                            int threshold_for_trusted_ground, const float* map_xyz, std::size_t n_map,
                            const float* ground_xyz, std::size_t n_ground, const float* ground_normals,
                            const float* flat_xyz, std::size_t n_flat, const float* less_sharp_xyzi, std::size_t n_ls,
                            const float* states, std::size_t n_states, float* likelihood, float* quality, double* trace,
                            int32_t* branch) {
  auto node = std::make_shared<rclcpp::Node>("ref_mcl");
  node->set_override("likelihood.match_dist_min", rclcpp::ParameterValue(match_dist_min));
  node->set_override("likelihood.match_dist_flat", rclcpp::ParameterValue(match_dist_flat));
  node->set_override("likelihood.radius_of_ground_search", rclcpp::ParameterValue(radius_of_ground_search));
  node->set_override("likelihood.threshold_for_trusted_ground", rclcpp::ParameterValue(threshold_for_trusted_ground));
  mcl_3dl::LidarMeasurementModelLikelihood model;
  model.loadConfig(std::make_shared<rclcpp::node_interfaces::NodeLoggingInterface>(),
                   std::make_shared<rclcpp::node_interfaces::NodeParametersInterface>(node));

  pcl::KdTreeFLANN<mcl_3dl::pcl_t> kdtree, kdtree_ground;
  kdtree.setInputCloud(cloud_of(map_xyz, n_map, 3, false));
  kdtree_ground.setInputCloud(cloud_of(ground_xyz, n_ground, 3, false));
  pcl::PointCloud<pcl::Normal> normals;
  for (std::size_t i = 0; i < n_ground; ++i) {
    pcl::Normal n;
    n.normal_x = ground_normals[3 * i];
    n.normal_y = ground_normals[3 * i + 1];
    n.normal_z = ground_normals[3 * i + 2];
    normals.push_back(n);
  }
  std::map<std::string, Cloud::Ptr> segmentations;
  segmentations["flat"] = cloud_of(flat_xyz, n_flat, 3, false);
  segmentations["less_sharp"] = cloud_of(less_sharp_xyzi, n_ls, 4, true);

  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double>& log = ref_shim_trace::buffer();
  for (std::size_t p = 0; p < n_states; ++p) {
    log.clear();
    const mcl_3dl::LidarMeasurementResult r =
        model.measure(kdtree, kdtree_ground, normals, segmentations, state_of(states + 7 * p));
    likelihood[p] = r.likelihood;
    quality[p] = r.quality;
    double* t = trace + REF_MCL_TRACE_WIDTH * p;
    for (int k = 0; k < REF_MCL_TRACE_WIDTH; ++k) t[k] = nan;
    // the records, each [count, values...]: [1 n] then [5 n thr x y z], or [3 nx ny nz], or [3 ..][3 R P Y][1 diff]
    std::vector<std::vector<double>> rec;
    for (std::size_t i = 0; i < log.size();) {
      const std::size_t k = static_cast<std::size_t>(log[i]);
      if (i + 1 + k > log.size()) return -static_cast<int>(1 + p);
      rec.emplace_back(log.begin() + i + 1, log.begin() + i + 1 + k);
      i += 1 + k;
    }
    if (rec.size() < 2 || rec[0].size() != 1) return -static_cast<int>(1 + p);
    t[0] = rec[0][0];
    if (rec.size() == 2 && rec[1].size() == 5 && rec[1][0] == rec[0][0]) {
      branch[p] = REF_MCL_BRANCH_UNTRUSTED;
    } else if (rec[1].size() == 3 && (rec.size() == 2 || (rec.size() == 4 && rec[2].size() == 3 && rec[3].size() == 1))) {
      t[1] = rec[1][0]; t[2] = rec[1][1]; t[3] = rec[1][2];
      branch[p] = REF_MCL_BRANCH_STEEP;
      if (rec.size() == 4) {
        t[4] = rec[2][0]; t[5] = rec[2][1]; t[6] = rec[2][2];
        t[7] = rec[3][0];
        branch[p] = REF_MCL_BRANCH_ROLL;
      }
    } else {
      return -static_cast<int>(1 + p);
    }
  }
  log.clear();
  return 0;
}

// State6DOF::transform of M points by N states -> out[N][M][3]
REF_API void ref_mcl_transform(const float* points_xyz, std::size_t n_points, const float* states, std::size_t n_states,
                               float* out) {
  const Cloud::Ptr src = cloud_of(points_xyz, n_points, 3, false);
  for (std::size_t p = 0; p < n_states; ++p) {
    Cloud moved = *src;
    state_of(states + 7 * p).transform(moved);
    for (std::size_t i = 0; i < n_points; ++i) {
      float* o = out + 3 * (p * n_points + i);
      o[0] = moved.points[i].x;
      o[1] = moved.points[i].y;
      o[2] = moved.points[i].z;
    }
  }
}

// RESTATED, not reference code: the running minimum and maximum of the match ratios that the lambda of
// mcl_3dl.cpp:476-498 keeps while the particle filter calls it once per particle (the lambda lives inside the node
// class and cannot be compiled alone) -> out[0] = match_ratio_min, out[1] = match_ratio_max
REF_API void ref_mcl_quality_minmax(const float* quality, std::size_t n, float* out) {
  float lo = 1.0f, hi = 0.0f;       // the lambda's starting values; strict comparisons, so a NaN quality changes neither
  for (std::size_t p = 0; p < n; ++p) {
    if (lo > quality[p]) lo = quality[p];
    if (hi < quality[p]) hi = quality[p];
  }
  out[0] = lo;
  out[1] = hi;
}
