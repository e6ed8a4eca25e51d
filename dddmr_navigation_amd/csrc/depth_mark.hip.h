// depth_mark.hip.h -- DepthCameraLayer::selfMark on the device: the clusters addPCPtr is to be called with.
//
// Restates, for the global-mode DepthCameraLayer (dddmr_perception_3d/plugins/depth_camera/depth_camera_layer.cpp:487-601),
// one selfMark from the aggregated observation on: pcl::EuclideanClusterExtraction, the per-cluster centroid, the ground
// search (radius 0.1, :539), the 0.2 m VoxelGrid (:545-548), the static-map loop (:552-562) and
// isinFrustumsObservations(centroid) (:591).  The host keeps pct_marking_, addPCPtr and its dGraph: the call returns
// what addPCPtr is to be called with, in the order the reference would call it.  Nothing is stored on the device between
// calls.
//
// The observation is the one depth_clear.hip.h searches (the depth sources' alive frames behind one another) and so is
// its grid: 0.05 m cells, keyed by the feeds' epoch, built by whichever of the two calls comes first after a depth
// source has published.  The cluster tolerance's ball (0.1 m by default) spans five cells per axis of it.
//
// Launch sequence (the general route of marking_host.hip.h, whose kernels are used unchanged where they fit):
//   k_mk_cc_init, k_dm_cc_union (lock-free union-find over the grid: a component's root is its lowest point index, the
//   seed PCL starts the cluster from), k_mk_cc_keys + a stable radix sort by (root, index), k_mk_flags + scan +
//   k_mk_cluster_starts, k_dm_stage1 (one lane per cluster: float sums in ascending point index, / (float)size; min
//   size; ground), k_mk_ds_keys + radix sort + k_mk_flags + scan + k_mk_group_reduce (the 0.2 m VoxelGrid: one lane per
//   voxel adding floats in input order; voxels in index order, x fastest), k_dm_stage2 (static map, frustums, voxel
//   key), k_dm_pack (records and points into pinned, mapped memory).  One host wait; the host then replays the
//   reference's std::sort over the kept clusters' sizes (oracle/ASSUMPTIONS.md row 10) and writes the caller's arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "depth_clear.hip.h"
#include "dev_memory.hip.h"        // Owned, dev_alloc
#include "marking.hip.h"           // the cluster kernels of the general route
#include "marking_host.hip.h"      // ... and its host side: cluster_temp_bytes, the static grids, base_plane
#include "point_grid_plan.hip.h"   // cloud_arg_ok
#include "sensor_sources.hip.h"    // the depth sources' frustums and observation grid

#pragma clang fp contract(off)

namespace dddmr {

// what became of a cluster
enum : uint32_t { kDmBelowMin = 0, kDmGround = 1, kDmStatic = 2, kDmOutside = 3, kDmAccepted = 4, kDmPending = 5 };

struct DmRecord {             // one per cluster, in creation order (host-mapped)
  float cx, cy, cz;
  uint32_t size;              // before downsampling
  int32_t vx, vy, vz;         // addPCPtr's voxel key
  uint32_t fate;              // kDm*
  uint32_t ds_first, ds_count;   // its 0.2 m downsampled points: rows of the packed point array
};
struct DmHeader {             // host-mapped
  uint32_t n_clusters, n_groups, overflow, pad;
};

struct DmParams {
  double res, hres, ignore_ratio;
  float tol, tol2;            // cluster tolerance and static_cast<float>(tol * tol)
  int min_cluster;
  uint32_t n_obs, n_map;
};

// k_mk_cc_union with the grid's geometry read from the header in device memory (the box of the observation never
// reaches the host)
__global__ __launch_bounds__(256) void k_dm_cc_union(DmParams k, const PointGrid* __restrict__ hdr, const float4* __restrict__ pts,
                                                     uint32_t* parent) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= k.n_obs) return;
  const PointGrid obs = *hdr;
  const float4 p = pts[i];
  grid_for_each(obs, p.x, p.y, p.z, k.tol + kDcPad, [&](const float4 q) {
    const uint32_t j = (uint32_t)__float_as_int(q.w);
    if (j < i && l2_simple(q.x, q.y, q.z, p.x, p.y, p.z) < k.tol2) {
      uint32_t u = cc_find(parent, i), v = cc_find(parent, j);
      while (u != v) {
        if (u < v) { const uint32_t t = u; u = v; v = t; }          // u is the larger root
        const uint32_t old = atomicCAS(&parent[u], u, v);
        if (old == u) break;
        u = cc_find(parent, old);
        v = cc_find(parent, v);
      }
    }
    return false;
  });
}

// per cluster: centroid (:514-533: floats added in ascending point index, each divided by (float)size), min size,
// "cluster attaches the ground" (:539: radius 0.1, where the lidar layer uses 0.05)
__global__ __launch_bounds__(64) void k_dm_stage1(DmParams k, const MarkCounters* __restrict__ cnt, ClusterArrays c,
                                                  const unsigned long long* __restrict__ keys1, const float4* __restrict__ pts,
                                                  PointGrid ground, uint32_t* __restrict__ fate) {
  const uint32_t ci = blockIdx.x * 64 + threadIdx.x;
  if (ci >= cnt->n_clusters) return;
  const uint32_t b = c.start[ci], e = c.start[ci + 1];
  float cx = 0.f, cy = 0.f, cz = 0.f;
  for (uint32_t m = b; m < e; ++m) {
    const float4 p = pts[(uint32_t)(keys1[m] & 0xFFFFFu)];
    cx += p.x; cy += p.y; cz += p.z;
  }
  const float sz = (float)(e - b);
  cx /= sz; cy /= sz; cz /= sz;
  c.size[ci] = e - b;
  c.centroid[ci] = make_float4(cx, cy, cz, 0.f);
  c.ds_count[ci] = 0;
  uint32_t f = (int)(e - b) >= k.min_cluster ? kDmPending : kDmBelowMin;       // what extractEuclideanClusters returns
  if (f == kDmPending && grid_radius_count(ground, cx, cy, cz, 0.1f + kDcPad, static_cast<float>(0.1 * 0.1), 1) > 0) f = kDmGround;
  fate[ci] = f;
  c.state[ci] = f == kDmPending ? 1u : 0u;       // k_mk_ds_keys downsamples the clusters with a state
}

// per cluster that reached the VoxelGrid: the static-map loop (:549-562), isinFrustumsObservations on the raw float
// centroid (:591), addPCPtr's voxel key (a float divided by a double, truncated)
__global__ __launch_bounds__(64) void k_dm_stage2(DmParams k, DcFrustums S, const MarkCounters* __restrict__ cnt, ClusterArrays c,
                                                  PointGrid map, uint32_t* __restrict__ fate) {
  const uint32_t ci = blockIdx.x * 64 + threadIdx.x;
  if (ci >= cnt->n_clusters || fate[ci] != kDmPending) return;
  const float4 cen = c.centroid[ci];
  const size_t nds = c.ds_count[ci];
  size_t hit = 0;
  if (k.ignore_ratio <= 0.999) {
    // the loop searches with the CENTROID for every downsampled point (:554): all hit or none do
    const bool near = k.n_map > 0 && grid_radius_count(map, cen.x, cen.y, cen.z, 0.1f + kDcPad, static_cast<float>(0.1 * 0.1), 1) > 0;
    if (near)
      for (size_t a = 0; a < nds; ++a) {
        hit++;
        if (hit > nds * k.ignore_ratio) break;
      }
  }
  c.vkey[3 * ci + 0] = (int)(cen.x / k.res);
  c.vkey[3 * ci + 1] = (int)(cen.y / k.res);
  c.vkey[3 * ci + 2] = (int)(cen.z / k.hres);
  if (!(hit <= nds * k.ignore_ratio)) { fate[ci] = kDmStatic; return; }
  fate[ci] = dc_in_frustums(S, cen.x, cen.y, cen.z) ? kDmAccepted : kDmOutside;
}

// the results into pinned, mapped memory: a record per cluster, the downsampled points of the accepted clusters at the
// rows the records name, the counts
__global__ __launch_bounds__(256) void k_dm_pack(uint32_t n_obs, const MarkCounters* __restrict__ cnt, const uint32_t* __restrict__ n_groups,
                                                 ClusterArrays c, const uint32_t* __restrict__ fate, const uint32_t* __restrict__ ds_first,
                                                 const float4* __restrict__ ds, DmHeader* __restrict__ hdr_out,
                                                 DmRecord* __restrict__ rec_out, float* __restrict__ pts_out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_obs) return;
  const uint32_t nc = cnt->n_clusters, ng = *n_groups;
  if (i == 0) {
    hdr_out->n_clusters = nc;
    hdr_out->n_groups = ng;
    hdr_out->overflow = cnt->overflow;
    hdr_out->pad = 0;
  }
  if (i < nc) {
    const float4 cen = c.centroid[i];
    const uint32_t f = fate[i];
    DmRecord r;
    r.cx = cen.x; r.cy = cen.y; r.cz = cen.z;
    r.size = c.size[i];
    const bool keyed = f >= kDmStatic;
    r.vx = keyed ? c.vkey[3 * i + 0] : 0;
    r.vy = keyed ? c.vkey[3 * i + 1] : 0;
    r.vz = keyed ? c.vkey[3 * i + 2] : 0;
    r.fate = f;
    r.ds_first = ds_first[i];
    r.ds_count = c.ds_count[i];
    rec_out[i] = r;
  }
  if (i < ng) {
    const float4 p = ds[i];
    if (fate[(uint32_t)__float_as_int(p.w)] == kDmAccepted) {
      pts_out[3 * (size_t)i + 0] = p.x;
      pts_out[3 * (size_t)i + 1] = p.y;
      pts_out[3 * (size_t)i + 2] = p.z;
    }
  }
}

}  // namespace dddmr

// ---- host ---------------------------------------------------------------------------------------------------------
namespace {

struct DepthMarkState {
  dddmr_depth_mark_config cfg{};
  uint32_t max_obs = 0;
  StaticGrids grids;
  ClusterScratch sc;                       // scratch of one call (sized for max_obs), with fate and the counters below
  uint32_t* fate = nullptr;
  MarkCounters* counters = nullptr;
  Owned mem;                               // (of the two above and the staging below)
  // pinned + mapped results, grown on demand
  void* out_host = nullptr;
  void* out_dev = nullptr;
  size_t out_cap = 0;
};

static_assert(!std::is_copy_constructible_v<DepthMarkState>);

// `table`: slots of the marking store that does its housekeeping with this state's rocPRIM storage (depth_layer.hip.h), 0: none
int depth_mark_init(dddmr_rollout_ctx* ctx, DepthMarkState* s, size_t table, const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                    const float* map_xyz, size_t n_map, size_t map_stride_bytes) {
  size_t temp_bytes = 0;
  int rc = cluster_temp_bytes(ctx, s->max_obs, table, &temp_bytes);
  if (rc != DDDMR_OK) return rc;
  if (cluster_scratch_alloc(s->sc, s->max_obs, temp_bytes) != 0) return fail(ctx, DDDMR_ERR_HIP, "depth mark: the cluster scratch's allocation failed");
  rc = static_grids_upload(ctx, s->grids, s->sc.temp, s->sc.temp_bytes, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes);
  if (rc != DDDMR_OK) return rc;
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->fate, s->max_obs));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->counters, 1));
  return DDDMR_OK;
}

// The enqueue part of one selfMark, shared by depth_mark_clusters and the depth layer's update (depth_layer.hip.h): from
// the Euclidean clusters to k_dm_stage2 on `st`, over the n points of the observation grid `d` holds.  Afterwards
// s->counters->n_clusters, s->sc.cl (start, size, centroid, ds_count, vkey), s->fate, s->sc.ds, s->sc.ds_first and s->sc.n_groups are what
// the launch sequence at the top of this file leaves.  *ops grows by the kernels enqueued (rocPRIM's are the caller's to add).
#define DM_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); ++*ops; } while (0)
int depth_mark_enqueue(dddmr_rollout_ctx* ctx, DepthMarkState* s, const double T_gbl_base[7], DepthClear& d, uint32_t n,
                       const DcFrustums& S, hipStream_t st, uint32_t* ops) {
  DmParams k;
  k.res = s->cfg.xy_resolution;
  k.hres = s->cfg.height_resolution;
  k.ignore_ratio = s->cfg.segmentation_ignore_ratio;
  k.tol = (float)s->cfg.euclidean_cluster_extraction_tolerance;
  k.tol2 = static_cast<float>(s->cfg.euclidean_cluster_extraction_tolerance * s->cfg.euclidean_cluster_extraction_tolerance);
  k.min_cluster = s->cfg.euclidean_cluster_extraction_min_cluster_size;
  k.n_obs = n;
  k.n_map = s->grids.n_map;
  MarkParams mk{};                        // what the general route's kernels read of it
  mk.n_obs = n;
  const float4* pts = d.pts;
  const dim3 pb((n + 255) / 256), cb((n + 63) / 64);
  HIPCHK(ctx, hipMemsetAsync(s->counters, 0, sizeof(MarkCounters), st));
  // Euclidean clusters
  DM_LAUNCH(k_mk_cc_init, pb, dim3(256), 0, st, n, s->sc.parent);
  DM_LAUNCH(k_dm_cc_union, pb, dim3(256), 0, st, k, d.hdr, pts, s->sc.parent);
  DM_LAUNCH(k_mk_cc_keys, pb, dim3(256), 0, st, n, s->sc.parent, s->sc.keys_a);
  size_t tb = s->sc.temp_bytes;
  HIPCHK(ctx, rocprim::radix_sort_keys(s->sc.temp, tb, s->sc.keys_a, s->sc.keys1, (size_t)n, 0, 40, st));
  DM_LAUNCH(k_mk_flags, pb, dim3(256), 0, st, n, s->sc.keys1, 20, s->sc.flags);
  tb = s->sc.temp_bytes;
  HIPCHK(ctx, rocprim::inclusive_scan(s->sc.temp, tb, s->sc.flags, s->sc.cid_incl, (size_t)n, rocprim::plus<uint32_t>(), st));
  DM_LAUNCH(k_mk_cluster_starts, pb, dim3(256), 0, st, n, s->sc.flags, s->sc.cid_incl, s->sc.cl, s->counters);
  DM_LAUNCH(k_dm_stage1, cb, dim3(64), 0, st, k, s->counters, s->sc.cl, s->sc.keys1, pts, s->grids.ground.g, s->fate);
  // 0.2 m VoxelGrid of every cluster that is still in: stable sort by (cluster, voxel), one lane per voxel.  The voxel
  // indices are keyed relative to the robot's voxel - half the key range (+-6.5 km in x / y, +-102 m in z).
  const int ox = (int)std::floor((float)T_gbl_base[0] / 0.2f) - kVgHalfXY, oy = (int)std::floor((float)T_gbl_base[1] / 0.2f) - kVgHalfXY,
            oz = (int)std::floor((float)T_gbl_base[2] / 0.2f) - kVgHalfZ;
  DM_LAUNCH(k_mk_ds_keys, pb, dim3(256), 0, st, mk, s->sc.keys1, s->sc.cid_incl, s->sc.cl, pts, ox, oy, oz, s->sc.keys_a, s->sc.vals_a, s->counters);
  tb = s->sc.temp_bytes;
  HIPCHK(ctx, rocprim::radix_sort_pairs(s->sc.temp, tb, s->sc.keys_a, s->sc.keys_b, s->sc.vals_a, s->sc.vals_b, (size_t)n, 0, 62, st));
  DM_LAUNCH(k_mk_flags, pb, dim3(256), 0, st, n, s->sc.keys_b, 0, s->sc.flags);
  tb = s->sc.temp_bytes;
  HIPCHK(ctx, rocprim::inclusive_scan(s->sc.temp, tb, s->sc.flags, s->sc.incl, (size_t)n, rocprim::plus<uint32_t>(), st));
  HIPCHK(ctx, hipMemsetAsync(s->sc.ds_first, 0xFF, (size_t)n * sizeof(uint32_t), st));
  DM_LAUNCH(k_mk_group_reduce, cb, dim3(64), 0, st, n, s->sc.keys_b, s->sc.vals_b, s->sc.flags, s->sc.incl, 0, s->sc.keys1, pts, s->sc.ds,
            s->sc.cl.ds_count, s->sc.ds_first, s->sc.n_groups);
  DM_LAUNCH(k_dm_stage2, cb, dim3(64), 0, st, k, S, s->counters, s->sc.cl, s->grids.map.g, s->fate);
  return DDDMR_OK;
}
#undef DM_LAUNCH

}  // namespace

extern "C" {

int dddmr_rollout_depth_mark_create(dddmr_rollout_ctx* ctx, const dddmr_depth_mark_config* cfg, const float* ground_xyz,
                                    size_t n_ground, size_t ground_stride_bytes, const float* map_xyz, size_t n_map,
                                    size_t map_stride_bytes) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  if (!cloud_arg_ok(ground_xyz, n_ground, ground_stride_bytes) || !cloud_arg_ok(map_xyz, n_map, map_stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_mark_create: bad cloud pointer / stride");
  if (!(cfg->xy_resolution > 0) || !(cfg->height_resolution > 0) || !(cfg->euclidean_cluster_extraction_tolerance > 0) ||
      !std::isfinite(cfg->xy_resolution) || !std::isfinite(cfg->height_resolution) ||
      !std::isfinite(cfg->euclidean_cluster_extraction_tolerance) || !std::isfinite(cfg->segmentation_ignore_ratio) ||
      cfg->euclidean_cluster_extraction_min_cluster_size < 0 || cfg->max_observation_points == 0)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_mark_create: resolutions, tolerance and max_observation_points must be positive and finite");
  // the sort keys of a call carry the observation point index in 20 bits ((root << 20) | i, cluster id << 42)
  if (n_ground >= (1u << 30) || n_map >= (1u << 30) || cfg->max_observation_points > kMarkMaxObs)
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_mark_create: at most %u observation points", kMarkMaxObs);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);          // the static grids are built on the tick's stream
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "depth_mark_create while a tick_begin is pending");
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  ctx->dmark.reset();                                    // (the old state goes first: after a failed create there is none)
  auto s = std::make_unique<DepthMarkState>();
  s->cfg = *cfg;
  s->max_obs = cfg->max_observation_points;
  const int rc = depth_mark_init(ctx, s.get(), 0, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes);
  if (rc == DDDMR_OK) ctx->dmark.reset(s.release());     // only a complete state is ever visible
  return rc;
}

int dddmr_rollout_depth_mark_clusters(dddmr_rollout_ctx* ctx, const double T_gbl_base[7], size_t capacity_clusters,
                                      size_t capacity_points, float* centroid_out, int32_t* voxel_out, uint32_t* size_out,
                                      uint32_t* offsets_out, float* cluster_xyz_out, float plane_out[4],
                                      dddmr_depth_mark_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!T_gbl_base || !stats) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_mark_clusters: null argument");
  for (int i = 0; i < 7; ++i)
    if (!std::isfinite(T_gbl_base[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_mark_clusters: non-finite transform");
  const int n_out = (centroid_out != nullptr) + (voxel_out != nullptr) + (size_out != nullptr) + (offsets_out != nullptr) +
                    (cluster_xyz_out != nullptr) + (plane_out != nullptr);
  if (n_out != 0 && n_out != 6)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_mark_clusters: the outputs besides stats are all given or all NULL (count only)");
  const bool count_only = n_out == 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthMarkState* s = ctx->dmark.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "depth_mark_clusters before depth_mark_create");
  DcFrustums S;
  int rc = depth_frustums(ctx, "depth_mark_clusters", &S);
  if (rc != DDDMR_OK) return rc;
  const size_t n_obs = ctx->sources.depth_points();
  if (n_obs > s->max_obs)
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_mark_clusters: %zu observation points, max_observation_points %u", n_obs, s->max_obs);
  dddmr_depth_mark_stats out{};
  out.n_observation = (uint32_t)n_obs;
  // coefficients (:568-578): tf2::quatRotate(q, (0, 0, 1)) and d in double, each rounded to float
  float plane[4];
  base_plane(T_gbl_base, plane);
  if (!(n_obs > 5)) {                                    // :491-492
    if (!count_only) {
      std::memcpy(plane_out, plane, sizeof(plane));
      offsets_out[0] = 0;
    }
    *stats = out;
    return DDDMR_OK;
  }
  if ((rc = depth_clear_scratch(ctx, "depth_mark_clusters")) != DDDMR_OK) return rc;
  DepthClear& d = *ctx->dclear;
  hipStream_t st = ctx->copy_stream;      // the stream the depth feeds ran on: their frames are complete before this work
  uint32_t ops = 0;
  Drain drain{st};                        // from the grid's launches on: an error exit below waits for them
  if ((rc = depth_observation_grid(ctx, d, n_obs, st, &ops)) != DDDMR_OK) return rc;
  const uint32_t n = (uint32_t)n_obs;
  const size_t rec_at = sizeof(DmHeader), pts_at = rec_at + (size_t)n * sizeof(DmRecord);
  if (host_mapped_reserve(s->mem.host, &s->out_host, &s->out_dev, &s->out_cap, pts_at + (size_t)n * 12) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "depth_mark_clusters: staging for %u observation points", n);

  if ((rc = depth_mark_enqueue(ctx, s, T_gbl_base, d, n, S, st, &ops)) != DDDMR_OK) return rc;
  const dim3 pb((n + 255) / 256);
#define DM_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); ++ops; } while (0)
  char* dev = static_cast<char*>(s->out_dev);
  DM_LAUNCH(k_dm_pack, pb, dim3(256), 0, st, n, s->counters, s->sc.n_groups, s->sc.cl, s->fate, s->sc.ds_first, s->sc.ds,
            reinterpret_cast<DmHeader*>(dev), reinterpret_cast<DmRecord*>(dev + rec_at), reinterpret_cast<float*>(dev + pts_at));
#undef DM_LAUNCH
  ops += 2 * 10 + 2 * 3 + 2;              // rocPRIM: two sorts (block sort + ~8 merge passes + id wrapper), two scans; two memsets
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));                 // the call's one host wait
  drain.armed = false;
  out.launches = ops;

  const char* host = static_cast<const char*>(s->out_host);
  const DmHeader hd = *reinterpret_cast<const DmHeader*>(host);
  const DmRecord* rec = reinterpret_cast<const DmRecord*>(host + rec_at);
  const float* dsp = reinterpret_cast<const float*>(host + pts_at);
  if (hd.overflow) {
    *stats = out;
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_mark_clusters: a cluster point lies beyond the VoxelGrid key range around the robot");
  }
  // what extractEuclideanClusters hands to the sort: the clusters of at least min_cluster_size points, in creation
  // order; then the reference's std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters), sizes only
  std::vector<DmItem> order;
  order.reserve(hd.n_clusters);
  for (uint32_t ci = 0; ci < hd.n_clusters; ++ci) {
    switch (rec[ci].fate) {
      case kDmBelowMin: continue;
      case kDmGround: ++out.n_ground_rejected; break;
      case kDmStatic: ++out.n_static_rejected; break;
      case kDmOutside: ++out.n_outside_frustums; break;
      default: ++out.n_accepted; out.n_points += rec[ci].ds_count; break;
    }
    order.push_back(DmItem{rec[ci].size, ci});
  }
  out.n_clusters = (uint32_t)order.size();
  *stats = out;
  if (count_only) return DDDMR_OK;
  if (out.n_accepted > capacity_clusters || out.n_points > capacity_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_mark_clusters: %u clusters / %u points, capacity %zu / %zu", out.n_accepted, out.n_points,
                capacity_clusters, capacity_points);
  dm_replay_sort(order);
  size_t c = 0, p = 0;
  offsets_out[0] = 0;
  for (const DmItem& it : order) {
    const DmRecord& r = rec[it.ci];
    if (r.fate != kDmAccepted) continue;
    centroid_out[3 * c + 0] = r.cx; centroid_out[3 * c + 1] = r.cy; centroid_out[3 * c + 2] = r.cz;
    voxel_out[3 * c + 0] = r.vx; voxel_out[3 * c + 1] = r.vy; voxel_out[3 * c + 2] = r.vz;
    size_out[c] = r.size;
    std::memcpy(cluster_xyz_out + 3 * p, dsp + 3 * (size_t)r.ds_first, (size_t)r.ds_count * 12);
    p += r.ds_count;
    offsets_out[++c] = (uint32_t)p;
  }
  std::memcpy(plane_out, plane, sizeof(plane));
  return DDDMR_OK;
}

}  // extern "C"
