// mcl_measure.hip.h -- the particle filter's lidar likelihood on the device: one
// LidarMeasurementModelLikelihood::measure() per particle, for a batch of particles
// (citations relative to the reference's src/dddmr_mcl_3dl/):
//   measure()                       src/lidar_measurement_model_likelihood.cpp:86-252  -> k_mcl_ground, k_mcl_match
//   State6DOF::transform            include/mcl_3dl/state_6dof.h:188-198               -> mcl_rotation(), mcl_transform()
//   Quat::normalized / operator*    include/mcl_3dl/quat.h:87-93,131-143,175-178
//   the lambda around measure()     src/mcl_3dl.cpp:476-498 (quality minimum / maximum) -> k_mcl_finish
//
// Both kd-trees become PointGrids (point_grid.hip.h): every radius query is answered with FLANN's float L2_Simple distance
// and its strict <.  What is summed in an order the result shows is summed in that order by ONE lane: score_like over
// the flat points and then the less-sharp points, the normal averages over the ground neighbours in FLANN's sorted
// order (ascending float d2; ties by ground index).  Everything else runs in parallel.
//
// One route for every size: k_mcl_ground takes a wave per particle, k_mcl_match stages the observation in LDS once per
// workgroup and walks its share of the particles with a wave each, k_mcl_finish is one workgroup.  No kernel leaves a
// table behind that the next call would have to clear, so a call enqueues no memset.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_memory.hip.h"        // Owned, dev_alloc, Drain, feed_wait
#include "point_grid.hip.h"
#include "point_grid_plan.hip.h"   // grid_shape, HostCloud, cloud_arg_ok, cloud_coords_ok
#include "wave_ops.hip.h"          // wave_min, wave_sum

#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kMclMaxGroundNb = 1024;   // ground neighbours of one particle (LDS of k_mcl_ground)
constexpr uint32_t kMclMaxObs = 2000;        // flat + less-sharp points of one call (LDS of k_mcl_match: 32 bytes each)
constexpr uint32_t kMclMaxParticles = 1u << 20;
// By how much the search boxes are widened.  The distance test decides; this only has to cover the rounding of
// (q - origin) + r against (p - origin): three float operations, half an ulp each of a number no larger than the
// cloud's extent plus the radius.  Below 8192 m an ulp is 4.9e-4 m and 1.5 of them stay under the pad, so set_map
// refuses a cloud wider than kMclMaxExtent on any axis (radii are at most 1000 m).
constexpr float kMclPad = 1e-3f;
constexpr float kMclMaxExtent = kCloudMaxExtent;   // (the name the messages print)
// The unhealthy branch's 1-NN has no radius in the reference.  sqrtf(d2) >= 1 gives a weight <= 0: exactly 0 stays 0,
// anything below becomes 0.01, as "none found" does.  sqrtf rounds every d2 < 1.001f that is not 1.0f itself or its
// successor to more than 1.0f, so searching to d2 < 1.001f loses nothing.
constexpr float kMclNnD2 = 1.001f;
constexpr float kMclNnRadius = 1.001f;       // > sqrt(kMclNnD2)

constexpr uint32_t kMclHealthy = 1u, kMclBadState = 2u, kMclOverCap = 4u;

struct MclParams {
  float mdm, mdf;               // match_dist_min_, match_dist_flat_ (floats in the reference)
  float r2_match;               // static_cast<float>(double(mdm) * double(mdm)): pcl::KdTreeFLANN::radiusSearch
  float r_ground, r2_ground;    // (float)radius_of_ground_search_, static_cast<float>(radius * radius)
  uint32_t threshold;           // threshold_for_trusted_ground_
  uint32_t cap_nb;              // max_ground_neighbours (<= kMclMaxGroundNb)
  uint32_t n_flat, n_ls, n_states;
};

struct MclTerms {               // per particle, device memory (dddmr_rollout_mcl_get_terms)
  float* score;                 // score_like
  float* pos_weight;
  uint32_t* n_match;            // num
  uint32_t* n_ground;           // pointIdxRadiusSearch.size()
  uint32_t* flags;              // kMclHealthy | kMclBadState | kMclOverCap
};

struct MclResult {              // host-mapped; seq is stored last
  float q_min, q_max;
  uint32_t n_bad, n_over, max_ground;
  uint32_t seq;
};

__device__ __forceinline__ bool mcl_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// rot_.normalized(): q * float(1.0 / double(norm)), norm = sqrtf(x*x + y*y + z*z + w*w) added left to right
__device__ __forceinline__ float4 mcl_rotation(float x, float y, float z, float w) {
  const float n = sqrtf(fadd(fadd(fadd(fmul(x, x), fmul(y, y)), fmul(z, z)), fmul(w, w)));
  const float s = (float)(1.0 / (double)n);
  return make_float4(fmul(x, s), fmul(y, s), fmul(z, s), fmul(w, s));
}
// Quat::operator*(const Quat&), each component's sum left to right
__device__ __forceinline__ float4 mcl_qmul(float4 a, float4 b) {
  return make_float4(fsub(fadd(fadd(fmul(a.w, b.x), fmul(a.x, b.w)), fmul(a.y, b.z)), fmul(a.z, b.y)),
                     fsub(fadd(fadd(fmul(a.w, b.y), fmul(a.y, b.w)), fmul(a.z, b.x)), fmul(a.x, b.z)),
                     fsub(fadd(fadd(fmul(a.w, b.z), fmul(a.z, b.w)), fmul(a.x, b.y)), fmul(a.y, b.x)),
                     fsub(fsub(fsub(fmul(a.w, b.w), fmul(a.x, b.x)), fmul(a.y, b.y)), fmul(a.z, b.z)));
}
// r * Vec3(p) + pos_: (r * Quat(p, 0)) * conj(r), then the translation
__device__ __forceinline__ float3 mcl_transform(float4 r, float px, float py, float pz, float tx, float ty, float tz) {
  const float4 a = mcl_qmul(r, make_float4(px, py, pz, 0.0f));
  const float4 b = mcl_qmul(a, make_float4(-r.x, -r.y, -r.z, r.w));
  return make_float3(fadd(b.x, tx), fadd(b.y, ty), fadd(b.z, tz));
}

// The healthy branch's weight from the normal averages on (:133-177), in double like the reference's tf2 chain:
// axis x up, tf2::Quaternion(axis, angle) (which divides by the axis' length: a zero axis gives NaN, every band test
// then fails and roll_diff is 0.55), q_pose * q_normal with the RAW rot_, normalize, Matrix3x3(q).getRPY.
__device__ inline float mcl_weight_healthy(float avg_nx, float avg_ny, float avg_nz, float qx_, float qy_, float qz_, float qw_, float d2_nn) {
  if (fabs((double)avg_nx) >= 3. * fabs((double)avg_nz) || fabs((double)avg_ny) >= 3. * fabs((double)avg_nz)) return (float)0.2;
  const double ax = avg_nx, ay = avg_ny, az = avg_nz;
  const double rx = ay * 1.0 - az * 0.0, ry = az * 0.0 - ax * 1.0, rz = ax * 0.0 - ay * 0.0;      // axis.cross(up)
  const double angle = -1.0 * acos(ax * 0.0 + ay * 0.0 + az * 1.0);
  const double d = sqrt(rx * rx + ry * ry + rz * rz);
  const double s = sin(angle * 0.5) / d;
  double nx = rx * s, ny = ry * s, nz = rz * s, nw = cos(angle * 0.5);
  double inv = 1.0 / sqrt(nx * nx + ny * ny + nz * nz + nw * nw);                                  // q_normal.normalize()
  nx *= inv; ny *= inv; nz *= inv; nw *= inv;
  const double px = qx_, py = qy_, pz = qz_, pw = qw_;
  double x = pw * nx + px * nw + py * nz - pz * ny;                                                // q_pose * q_normal
  double y = pw * ny + py * nw + pz * nx - px * nz;
  double z = pw * nz + pz * nw + px * ny - py * nx;
  double w = pw * nw - px * nx - py * ny - pz * nz;
  inv = 1.0 / sqrt(x * x + y * y + z * z + w * w);                                                 // q_new.normalize()
  x *= inv; y *= inv; z *= inv; w *= inv;
  const double dd = x * x + y * y + z * z + w * w;                                                 // Matrix3x3::setRotation
  const double s2 = 2.0 / dd;
  const double xs = x * s2, ys = y * s2, zs = z * s2;
  const double wx = w * xs, wy = w * ys;
  const double xx = x * xs, xz = x * zs, yy = y * ys, yz = y * zs;
  const double m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
  double roll;
  if (fabs(m20) >= 1.0) {
    roll = atan2(m21, m22);                                                                        // getEulerYPR's gimbal branch
  } else {
    const double pitch = -asin(m20);
    roll = atan2(m21 / cos(pitch), m22 / cos(pitch));
  }
  double roll_diff;
  if (fabs(roll) > 2.6 && fabs(roll) < 3.1415926) roll_diff = 3.1415926 - fabs(roll);
  else if (fabs(roll) >= 0 && fabs(roll) < 0.5) roll_diff = fabs(roll);
  else roll_diff = 0.55;
  float pos_weight = (float)((1.0 - sqrtf(d2_nn)) * (1 - roll_diff));
  if (pos_weight < 0) pos_weight = (float)0.01;
  return pos_weight;
}

// Ground health, the normal averages and pos_weight of one particle per wave (:105-192).
//   states   [n][7] pos xyz, rot xyzw, raw
//   normals  one per ground point, by the ground cloud's own index
__global__ __launch_bounds__(64) void k_mcl_ground(MclParams k, PointGrid ground, PointGrid map, const float4* __restrict__ normals,
                                                   const float* __restrict__ states, MclTerms t) {
  __shared__ float s_d2[kMclMaxGroundNb];
  __shared__ uint32_t s_idx[kMclMaxGroundNb];
  __shared__ float s_n[3][kMclMaxGroundNb];      // normal_x, normal_y, fabs(normal_z) in sorted order
  __shared__ uint32_t s_cnt;
  __shared__ float s_nn;
  const uint32_t p = blockIdx.x;
  const int lane = threadIdx.x;
  if (p >= k.n_states) return;
  const float* st = states + 7 * (size_t)p;
  const float px = st[0], py = st[1], pz = st[2], qx = st[3], qy = st[4], qz = st[5], qw = st[6];
  if (!(mcl_finite3(px, py, pz) && mcl_finite3(qx, qy, qz) && isfinite(qw))) {
    if (lane == 0) { t.pos_weight[p] = 0.f; t.n_ground[p] = 0; t.flags[p] = kMclBadState; }
    return;
  }
  if (lane == 0) s_cnt = 0;
  __syncthreads();
  grid_for_each_wave(ground, px, py, pz, k.r_ground + kMclPad, lane, [&](const float4 g) {
    const float d2 = l2_simple(g.x, g.y, g.z, px, py, pz);
    if (d2 < k.r2_ground) {
      const uint32_t slot = atomicAdd(&s_cnt, 1u);
      if (slot < k.cap_nb) { s_d2[slot] = d2; s_idx[slot] = (uint32_t)__float_as_int(g.w); }
    }
  });
  __syncthreads();
  const uint32_t cnt = s_cnt;
  if (cnt > k.cap_nb) {
    if (lane == 0) { t.pos_weight[p] = 0.f; t.n_ground[p] = cnt; t.flags[p] = kMclOverCap; }
    return;
  }
  const bool healthy = cnt >= k.threshold;
  // FLANN's sorted result: rank by (d2, ground index); the normals go to their rank
  for (uint32_t i = lane; i < cnt; i += 64) {
    const float d2 = s_d2[i];
    const uint32_t idx = s_idx[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < cnt; ++j) {
      const float dj = s_d2[j];
      rank += (dj < d2 || (dj == d2 && s_idx[j] < idx)) ? 1u : 0u;
    }
    const float4 nrm = normals[idx];
    s_n[0][rank] = nrm.x; s_n[1][rank] = nrm.y; s_n[2][rank] = fabsf(nrm.z);
    if (rank == 0) s_nn = d2;
  }
  // the 1-NN of the pose where the radius search does not give it: in the map when the ground is not trusted, in the
  // ground when it is trusted with no neighbour at all (threshold 0)
  float best = 3.0e38f;
  if (!healthy || cnt == 0) {
    const PointGrid& G = healthy ? ground : map;
    grid_for_each_wave(G, px, py, pz, kMclNnRadius + kMclPad, lane, [&](const float4 g) {
      best = fminf(best, l2_simple(g.x, g.y, g.z, px, py, pz));
    });
    best = wave_min(best);
  }
  __syncthreads();
  if (lane != 0) return;
  float w;
  if (healthy) {
    float avg_nx = 0.f, avg_ny = 0.f, avg_nz = 0.f;
    for (uint32_t i = 0; i < cnt; ++i) {
      avg_nx = fadd(avg_nx, s_n[0][i]);
      avg_ny = fadd(avg_ny, s_n[1][i]);
      avg_nz = fadd(avg_nz, s_n[2][i]);
    }
    const float c = (float)cnt;
    avg_nx /= c; avg_ny /= c; avg_nz /= c;
    // (no neighbour: the averages are 0 / 0 = NaN, the 3x test is false, roll is NaN and roll_diff 0.55; a nearest
    // ground point beyond the bounded search leaves a negative product either way)
    const float d2_nn = cnt ? s_nn : (best < kMclNnD2 ? best : 4.0f);
    w = mcl_weight_healthy(avg_nx, avg_ny, avg_nz, qx, qy, qz, qw, d2_nn);
  } else {
    w = (float)0.01;
    if (best < kMclNnD2) {
      w = (float)(1.0 - sqrtf(best));
      if (w < 0) w = (float)0.01;
    }
  }
  t.pos_weight[p] = w;
  t.n_ground[p] = cnt;
  t.flags[p] = healthy ? kMclHealthy : 0u;
}

// one point's term of score_like (:198-248); w = 1 for a flat point, the intensity for a less-sharp one (x / 1.0f is x)
__device__ __forceinline__ float mcl_term(const MclParams& k, const PointGrid& g, float4 r, float tx, float ty, float tz, float4 o,
                                          uint32_t* cnt) {
  const float3 q = mcl_transform(r, o.x, o.y, o.z, tx, ty, tz);
  if (!mcl_finite3(q.x, q.y, q.z)) return 0.f;
  // FLANN's radiusSearch(p, match_dist_min_, id, sqdist, 1) keeps the nearest neighbour inside the radius
  const float d2 = grid_nearest(g, q.x, q.y, q.z, k.mdm + kMclPad);
  if (!(d2 < k.r2_match)) return 0.f;
  const float dist = fsub(k.mdm, fmaxf(sqrtf(d2), k.mdf));
  if (dist < 0.0f) return 0.f;
  ++*cnt;
  return fmul(dist, dist) / o.w;
}

// score_like, num, likelihood and quality: the observation staged in LDS once per workgroup, then a wave per particle.
//   obs         [n_flat + n_ls] x y z w, flat points first with w = 1
//   dynamic LDS (n_flat + n_ls) * (16 + 4 * 4) bytes: the observation, then each wave's terms
// Likelihood and quality go straight to host-mapped memory; the host reads them after k_mcl_finish's result word.
__global__ __launch_bounds__(256) void k_mcl_match(MclParams k, PointGrid ground, PointGrid map, const float4* __restrict__ obs,
                                                   const float* __restrict__ states, MclTerms t, float* __restrict__ quality,
                                                   float* __restrict__ likelihood_out, float* __restrict__ quality_out) {
  extern __shared__ __attribute__((aligned(16))) char mcl_smem[];
  const uint32_t n_obs = k.n_flat + k.n_ls;
  float4* s_obs = reinterpret_cast<float4*>(mcl_smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* term = reinterpret_cast<float*>(mcl_smem + (size_t)n_obs * sizeof(float4)) + (size_t)wave * n_obs;
  for (uint32_t i = threadIdx.x; i < n_obs; i += 256) s_obs[i] = obs[i];
  __syncthreads();
  for (uint32_t base = blockIdx.x * 4u; base < k.n_states; base += gridDim.x * 4u) {     // (the same trips for every wave)
    const uint32_t p = base + (uint32_t)wave;
    const bool valid = p < k.n_states;
    const uint32_t flags = valid ? t.flags[p] : kMclBadState;
    const bool run = valid && !(flags & (kMclBadState | kMclOverCap));
    uint32_t cnt = 0;
    if (run) {
      const float* st = states + 7 * (size_t)p;
      const float tx = st[0], ty = st[1], tz = st[2];
      const float4 r = mcl_rotation(st[3], st[4], st[5], st[6]);
      const PointGrid& gf = (flags & kMclHealthy) ? ground : map;
      for (uint32_t i = lane; i < k.n_flat; i += 64) term[i] = mcl_term(k, gf, r, tx, ty, tz, s_obs[i], &cnt);
      for (uint32_t i = k.n_flat + lane; i < n_obs; i += 64) term[i] = mcl_term(k, map, r, tx, ty, tz, s_obs[i], &cnt);
      cnt = wave_sum(cnt);
    }
    __syncthreads();
    if (valid && lane == 0) {
      float score = 0.f;
      if (run)
        for (uint32_t i = 0; i < n_obs; ++i) score = fadd(score, term[i]);      // the reference's order: flat, then less sharp
      t.score[p] = score;
      t.n_match[p] = cnt;
      const float q = run ? (float)cnt / (float)n_obs : 0.f;
      quality[p] = q;                                                             // k_mcl_finish reduces the device copy
      likelihood_out[p] = run ? fmul(score, t.pos_weight[p]) : 0.f;               // host-mapped: the caller's two arrays
      quality_out[p] = q;                                                         // (complete when the kernel ends, before k_mcl_finish runs)
    }
    __syncthreads();
  }
}

// The call's quality minimum and maximum (mcl_3dl.cpp:476-498: they start at 1 and 0; a refused state's quality 0 takes
// part) and the refused particles, then the result word.  One workgroup, reading device memory only.
__global__ __launch_bounds__(256) void k_mcl_finish(MclParams k, MclTerms t, const float* __restrict__ quality, MclResult* __restrict__ res,
                                                    uint32_t seq) {
  __shared__ float s_min[256], s_max[256];
  __shared__ uint32_t s_bad[256], s_over[256], s_nb[256];
  float q_min = 1.0f, q_max = 0.0f;
  uint32_t bad = 0, over = 0, nb = 0;
  for (uint32_t p = threadIdx.x; p < k.n_states; p += 256) {
    const float q = quality[p];
    if (q_min > q) q_min = q;
    if (q_max < q) q_max = q;
    const uint32_t f = t.flags[p];
    bad += (f & kMclBadState) ? 1u : 0u;
    over += (f & kMclOverCap) ? 1u : 0u;
    nb = max(nb, t.n_ground[p]);
  }
  s_min[threadIdx.x] = q_min; s_max[threadIdx.x] = q_max; s_bad[threadIdx.x] = bad; s_over[threadIdx.x] = over; s_nb[threadIdx.x] = nb;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) {
      s_min[threadIdx.x] = fminf(s_min[threadIdx.x], s_min[threadIdx.x + m]);
      s_max[threadIdx.x] = fmaxf(s_max[threadIdx.x], s_max[threadIdx.x + m]);
      s_bad[threadIdx.x] += s_bad[threadIdx.x + m];
      s_over[threadIdx.x] += s_over[threadIdx.x + m];
      s_nb[threadIdx.x] = max(s_nb[threadIdx.x], s_nb[threadIdx.x + m]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    res->q_min = s_min[0]; res->q_max = s_max[0];
    res->n_bad = s_bad[0]; res->n_over = s_over[0]; res->max_ground = s_nb[0];
    __threadfence_system();
    __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace dddmr

// ---- host (included by rollout_engine.hip after the context) ---------------------------------------------------------
namespace {

struct MclObs;                             // the prepared observation, mcl_observation.hip.h
struct SubMapState;                        // the keyframe store and the warm-up generation, mcl_submap.hip.h
struct FilterState;                        // the resident particle set, mcl_filter.hip.h

struct MclMap {                            // one swapKdTree generation
  GridBuf map, ground;
  float4 *map_pts = nullptr, *ground_pts = nullptr, *normals = nullptr;
};

struct MclState {
  dddmr_mcl_config cfg{};
  MclParams k{};
  MclMap maps[2];
  MclMap warm;                             // a third generation for the sub-maps' warm-up, allocated by the first submap_create
  bool has_warm = false;                   // (owned by `mem` like the other two: submap_swap exchanges it with maps[cur])
  int cur = -1;                            // maps[cur] answers; -1 before the first set_map
  uint64_t serial = 0;                     // grows with every new current generation (set_map, submap_swap)
  uint2* slot = nullptr;                   // grid builder scratch
  char* temp = nullptr;                    // rocPRIM storage of the grid builder's scan
  size_t temp_bytes = 0;
  MclTerms t{};
  float* qual_dev = nullptr;
  Owned mem;
  // host-mapped: the call's inputs (read in place by the kernels) and results
  float4 *obs_host = nullptr, *obs_dev = nullptr;
  float *states_host = nullptr, *states_dev = nullptr;
  float *out_host = nullptr, *out_dev = nullptr;       // likelihood [max_particles], quality [max_particles]
  MclResult *res_host = nullptr, *res_dev = nullptr;
  uint32_t seq = 0;
  uint32_t last_n = 0;                     // particles of the last successful measure (get_terms)
  std::unique_ptr<MclObs, LateDelete<MclObs>> obs;   // dddmr_rollout_mcl_set_observation_config
  std::unique_ptr<SubMapState, LateDelete<SubMapState>> submap;   // dddmr_rollout_submap_create
  std::unique_ptr<FilterState, LateDelete<FilterState>> filter;   // dddmr_rollout_mcl_filter_create
};
static_assert(!std::is_copy_constructible_v<MclState>);

constexpr uint32_t kMclCells = 1u << 21;   // cells of each grid (grid_shape coarsens the cell until the cloud's box fits)

int mcl_alloc_generation(dddmr_rollout_ctx* ctx, MclState* s, MclMap& m) {
  const dddmr_mcl_config& c = s->cfg;
  DevAllocs& mem = s->mem.dev;
  if (grid_alloc(mem, m.map, kMclCells, c.max_map_points) != 0 || grid_alloc(mem, m.ground, kMclCells, c.max_ground_points) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "mcl_create: the grids' allocation failed");
  HIPCHK(ctx, dev_alloc(mem, &m.map_pts, std::max<size_t>(c.max_map_points, 1)));
  HIPCHK(ctx, dev_alloc(mem, &m.ground_pts, std::max<size_t>(c.max_ground_points, 1)));
  HIPCHK(ctx, dev_alloc(mem, &m.normals, std::max<size_t>(c.max_ground_points, 1)));
  return DDDMR_OK;
}

int mcl_alloc(dddmr_rollout_ctx* ctx, MclState* s) {
  const dddmr_mcl_config& c = s->cfg;
  DevAllocs& mem = s->mem.dev;
  {
    size_t e = 0;
    uint32_t* v = nullptr;
    HIPCHK(ctx, rocprim::exclusive_scan(nullptr, e, v, v, 0u, (size_t)kMclCells + 1, rocprim::plus<uint32_t>(), ctx->stream));
    s->temp_bytes = std::max(e, (size_t)4096) + 256;
    HIPCHK(ctx, dev_alloc(mem, &s->temp, s->temp_bytes));
  }
  HIPCHK(ctx, dev_alloc(mem, &s->slot, std::max<size_t>(std::max(c.max_map_points, c.max_ground_points), 1)));
  for (MclMap& m : s->maps)
    if (const int rc = mcl_alloc_generation(ctx, s, m)) return rc;
  const size_t N = c.max_particles;
  HIPCHK(ctx, dev_alloc(mem, &s->t.score, N));
  HIPCHK(ctx, dev_alloc(mem, &s->t.pos_weight, N));
  HIPCHK(ctx, dev_alloc(mem, &s->t.n_match, N));
  HIPCHK(ctx, dev_alloc(mem, &s->t.n_ground, N));
  HIPCHK(ctx, dev_alloc(mem, &s->t.flags, N));
  HIPCHK(ctx, dev_alloc(mem, &s->qual_dev, N));
  if (host_mapped_alloc(s->mem.host, &s->obs_host, &s->obs_dev, (size_t)c.max_observation_points * sizeof(float4)) != 0 ||
      host_mapped_alloc(s->mem.host, &s->states_host, &s->states_dev, N * 7 * sizeof(float)) != 0 ||
      host_mapped_alloc(s->mem.host, &s->out_host, &s->out_dev, N * 2 * sizeof(float)) != 0 ||
      host_mapped_alloc(s->mem.host, &s->res_host, &s->res_dev, sizeof(MclResult)) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "mcl_create: host-mapped staging");
  std::memset(s->res_host, 0, sizeof(MclResult));
  return DDDMR_OK;
}

// The grid of a generation's cloud, which lies in `dev` with its box known: enqueued on the context's stream, no wait.
// set_map's upload and the sub-maps' warm-up (mcl_submap.hip.h) both build their grids here.
int mcl_grid(dddmr_rollout_ctx* ctx, MclState* s, GridBuf& b, const float4* dev, const float lo[3], const float hi[3], size_t n) {
  const float cell = 2.02f * (s->k.mdm + kMclPad);
  grid_shape(b.g, lo, hi, cell, cell, b.cap_cells);
  return grid_build(ctx, s->temp, s->temp_bytes, b, dev, (uint32_t)n, s->slot, ctx->stream);
}

// One cloud into a generation's buffers: the points, their box, the grid.  Cells at least twice the match radius wide,
// so that a point's query touches at most 2 x 2 rows of cells (grid_for_each's fast path).  Waits for the stream: the
// caller's `h` is pageable.
int mcl_upload(dddmr_rollout_ctx* ctx, MclState* s, GridBuf& b, float4* dev, const HostCloud& h, size_t n) {
  Drain drain{ctx->stream};
  if (n) HIPCHK(ctx, hipMemcpyAsync(dev, h.pts.data(), n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  const int rc = mcl_grid(ctx, s, b, dev, h.lo, h.hi, n);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  drain.armed = false;
  return rc;
}

// The measure's three kernels over states the device can read ([n][7]: the host-mapped staging below, or the resident
// particles of mcl_filter.hip.h), enqueued on the context's stream.  Likelihood and quality go to the two pointers given.
// Returns the sequence number k_mcl_finish stores into the result word.
uint32_t mcl_launch(dddmr_rollout_ctx* ctx, MclState* s, const float4* obs_dev, size_t n_flat, size_t n_less_sharp, const float* states_dev,
                    uint32_t N, float* likelihood_dev, float* quality_dev) {
  MclParams k = s->k;
  k.n_flat = (uint32_t)n_flat;
  k.n_ls = (uint32_t)n_less_sharp;
  k.n_states = N;
  const MclMap& m = s->maps[s->cur];
  const uint32_t n_obs = k.n_flat + k.n_ls;
  const uint32_t seq = next_seq(s->seq);
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_mcl_ground, dim3(N), dim3(64), 0, st, k, m.ground.g, m.map.g, m.normals, states_dev, s->t);
  const uint32_t blocks = std::min<uint32_t>((N + 3) / 4, 2048u);
  hipLaunchKernelGGL(k_mcl_match, dim3(blocks), dim3(256), (size_t)n_obs * 32, st, k, m.ground.g, m.map.g, obs_dev, states_dev, s->t,
                     s->qual_dev, likelihood_dev, quality_dev);
  hipLaunchKernelGGL(k_mcl_finish, dim3(1), dim3(256), 0, st, k, s->t, s->qual_dev, s->res_dev, seq);
  return seq;
}

// One measure over an observation the device can read (k_mcl_match's layout): the host-mapped staging of
// dddmr_rollout_mcl_measure, or the prepared observation of mcl_observation.hip.h.  tick_mu held.
int mcl_run(dddmr_rollout_ctx* ctx, const char* what, MclState* s, const float4* obs_dev, size_t n_flat, size_t n_less_sharp, const float* states,
            size_t n_states, float* likelihood_out, float* quality_out, dddmr_mcl_stats* stats) {
  if (s->cur < 0) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_set_map", what);
  if (n_states > s->cfg.max_particles)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu particles, capacity %u", what, n_states, s->cfg.max_particles);
  if (n_states == 0) {
    if (stats) { stats->quality_min = 1.0f; stats->quality_max = 0.0f; }
    s->last_n = 0;
    return DDDMR_OK;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::memcpy(s->states_host, states, n_states * 7 * sizeof(float));
  const uint32_t N = (uint32_t)n_states;
  hipStream_t st = ctx->stream;
  const uint32_t seq = mcl_launch(ctx, s, obs_dev, n_flat, n_less_sharp, s->states_dev, N, s->out_dev, s->out_dev + s->cfg.max_particles);
  uint32_t waits = 0;                                  // the spin on the result word, and the stream's when the spin ran out
  if (const int rc = feed_wait(st, &s->res_host->seq, seq, &waits)) return fail(ctx, DDDMR_ERR_HIP, "%s: launch or wait failed (%d)", what, rc);
  const MclResult r = *s->res_host;
  if (stats) {
    stats->quality_min = r.q_min; stats->quality_max = r.q_max;
    stats->n_bad_states = r.n_bad; stats->n_over_capacity = r.n_over; stats->max_ground_neighbours_seen = r.max_ground;
    stats->launches = 3; stats->host_waits = waits;
  }
  if (r.n_over) {
    s->last_n = 0;
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %u particles with more than max_ground_neighbours %u ground points inside the radius (up to %u)",
                what, r.n_over, s->cfg.max_ground_neighbours, r.max_ground);
  }
  std::memcpy(likelihood_out, s->out_host, n_states * sizeof(float));
  std::memcpy(quality_out, s->out_host + s->cfg.max_particles, n_states * sizeof(float));
  s->last_n = N;
  return DDDMR_OK;
}

}  // namespace

extern "C" {

int dddmr_rollout_mcl_create(dddmr_rollout_ctx* ctx, const dddmr_mcl_config* cfg) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  if (!std::isfinite(cfg->match_dist_min) || !std::isfinite(cfg->match_dist_flat) || !std::isfinite(cfg->radius_of_ground_search) ||
      !(cfg->match_dist_min > 0) || !(cfg->radius_of_ground_search > 0) || cfg->match_dist_flat < 0 ||
      !((float)cfg->match_dist_min > 0.f) || cfg->match_dist_min > 1e3 || cfg->radius_of_ground_search > 1e3)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "mcl_create: match_dist_min and radius_of_ground_search must be positive, finite and at most 1000 m, match_dist_flat not negative");
  if (cfg->threshold_for_trusted_ground < 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "mcl_create: negative threshold_for_trusted_ground");
  if (cfg->max_particles == 0 || cfg->max_observation_points == 0 || cfg->max_ground_neighbours == 0)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "mcl_create: a capacity of 0");
  if (cfg->max_map_points > (1u << 24) || cfg->max_ground_points > (1u << 24) || cfg->max_particles > kMclMaxParticles ||
      cfg->max_observation_points > kMclMaxObs || cfg->max_ground_neighbours > kMclMaxGroundNb)
    return fail(ctx, DDDMR_ERR_CAPACITY, "mcl_create: at most 2^24 map / ground points, %u particles, %u observation points, %u ground neighbours",
                kMclMaxParticles, kMclMaxObs, kMclMaxGroundNb);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "mcl_create while a tick_begin is pending");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  auto s = std::make_unique<MclState>();
  s->cfg = *cfg;
  MclParams& k = s->k;
  k.mdm = (float)cfg->match_dist_min;
  k.mdf = (float)cfg->match_dist_flat;
  k.r2_match = static_cast<float>((double)k.mdm * (double)k.mdm);      // radiusSearch(p, double(match_dist_min_), ...)
  k.r_ground = (float)cfg->radius_of_ground_search;
  k.r2_ground = static_cast<float>(cfg->radius_of_ground_search * cfg->radius_of_ground_search);
  k.threshold = (uint32_t)cfg->threshold_for_trusted_ground;
  k.cap_nb = cfg->max_ground_neighbours;
  const int rc = mcl_alloc(ctx, s.get());
  if (rc == DDDMR_OK) ctx->mcl.reset(s.release());       // only a complete state is ever visible; the old one survives a failed create
  return rc;
}

int dddmr_rollout_mcl_set_map(dddmr_rollout_ctx* ctx, const float* map_xyz, size_t n_map, size_t map_stride_bytes,
                              const float* ground_xyz, const float* ground_normals, size_t n_ground, size_t ground_stride_bytes,
                              size_t normal_stride_bytes) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!cloud_arg_ok(map_xyz, n_map, map_stride_bytes) || !cloud_arg_ok(ground_xyz, n_ground, ground_stride_bytes) ||
      !cloud_arg_ok(ground_normals, n_ground, normal_stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "mcl_set_map: bad cloud pointer / stride");
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "mcl_set_map while a tick_begin is pending");
  MclState* s = ctx->mcl.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "mcl_set_map before mcl_create");
  if (n_map > s->cfg.max_map_points || n_ground > s->cfg.max_ground_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "mcl_set_map: %zu map / %zu ground points, capacity %u / %u", n_map, n_ground, s->cfg.max_map_points,
                s->cfg.max_ground_points);
  const HostCloud map_h(map_xyz, n_map, map_stride_bytes), ground_h(ground_xyz, n_ground, ground_stride_bytes);
  if (!cloud_coords_ok(map_h) || !cloud_coords_ok(ground_h))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "mcl_set_map: a map or ground coordinate is not finite or beyond 1e6 m, or a cloud is wider than %g m on an axis", (double)kMclMaxExtent);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  MclMap& m = s->maps[s->cur == 0 ? 1 : 0];              // beside the current one
  int rc = mcl_upload(ctx, s, m.map, m.map_pts, map_h, n_map);
  if (rc == DDDMR_OK) rc = mcl_upload(ctx, s, m.ground, m.ground_pts, ground_h, n_ground);
  if (rc != DDDMR_OK) return rc;
  if (n_ground)
    HIPCHK(ctx, hipMemcpy(m.normals, HostCloud(ground_normals, n_ground, normal_stride_bytes).pts.data(), n_ground * sizeof(float4), hipMemcpyHostToDevice));
  s->cur = s->cur == 0 ? 1 : 0;
  ++s->serial;
  return DDDMR_OK;
}

int dddmr_rollout_mcl_measure(dddmr_rollout_ctx* ctx, const float* flat_xyz, size_t n_flat, const float* less_sharp_xyzi,
                              size_t n_less_sharp, const float* states, size_t n_states, float* likelihood_out, float* quality_out,
                              dddmr_mcl_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (stats) *stats = dddmr_mcl_stats{};
  if ((n_flat && !flat_xyz) || (n_less_sharp && !less_sharp_xyzi) || (n_states && (!states || !likelihood_out || !quality_out)))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "mcl_measure: null argument");
  if (n_flat + n_less_sharp == 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "mcl_measure: no observation point (the reference divides 0 by 0)");
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "mcl_measure while a tick_begin is pending");
  MclState* s = ctx->mcl.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "mcl_measure before mcl_create");
  if (s->cur < 0) return fail(ctx, DDDMR_ERR_STATE, "mcl_measure before mcl_set_map");
  if (n_flat > s->cfg.max_observation_points || n_less_sharp > s->cfg.max_observation_points ||
      n_flat + n_less_sharp > s->cfg.max_observation_points || n_states > s->cfg.max_particles)
    return fail(ctx, DDDMR_ERR_CAPACITY, "mcl_measure: %zu particles, %zu + %zu observation points, capacity %u / %u", n_states, n_flat,
                n_less_sharp, s->cfg.max_particles, s->cfg.max_observation_points);
  if (n_states) {                                      // (without a particle nothing is read)
    for (size_t i = 0; i < n_flat; ++i) s->obs_host[i] = make_float4(flat_xyz[3 * i], flat_xyz[3 * i + 1], flat_xyz[3 * i + 2], 1.0f);
    if (n_less_sharp) std::memcpy(s->obs_host + n_flat, less_sharp_xyzi, n_less_sharp * sizeof(float4));
  }
  return mcl_run(ctx, "mcl_measure", s, s->obs_dev, n_flat, n_less_sharp, states, n_states, likelihood_out, quality_out, stats);
}

int dddmr_rollout_mcl_get_terms(dddmr_rollout_ctx* ctx, float* score_like_out, float* pos_weight_out, uint32_t* n_match_out,
                                uint32_t* n_ground_out, uint8_t* healthy_out, size_t capacity) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "mcl_get_terms while a tick_begin is pending");
  MclState* s = ctx->mcl.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "mcl_get_terms before mcl_create");
  const size_t n = s->last_n;
  if (capacity < n) return fail(ctx, DDDMR_ERR_CAPACITY, "mcl_get_terms: capacity %zu < %zu particles", capacity, n);
  if (n == 0) return DDDMR_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (score_like_out) HIPCHK(ctx, hipMemcpy(score_like_out, s->t.score, n * sizeof(float), hipMemcpyDeviceToHost));
  if (pos_weight_out) HIPCHK(ctx, hipMemcpy(pos_weight_out, s->t.pos_weight, n * sizeof(float), hipMemcpyDeviceToHost));
  if (n_match_out) HIPCHK(ctx, hipMemcpy(n_match_out, s->t.n_match, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (n_ground_out) HIPCHK(ctx, hipMemcpy(n_ground_out, s->t.n_ground, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (healthy_out) {
    std::vector<uint32_t> f(n);
    HIPCHK(ctx, hipMemcpy(f.data(), s->t.flags, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) healthy_out[i] = (f[i] & kMclHealthy) ? 1 : 0;
  }
  return DDDMR_OK;
}

}  // extern "C"
