// depth_layer.hip.h -- the global-mode DepthCameraLayer on the device: marking store, dGraph and lethal set.
//
// One dddmr_rollout_depth_layer_update is one selfClear + selfMark + updateLethalPointCloud pass
// (stacked_perception.cpp:82-88; dddmr_perception_3d/plugins/depth_camera/depth_camera_layer.cpp:252-426, :487-601;
// plugins/cluster_marking.cpp:49-138; src/graph/dynamic_graph.cpp:38-61) with pct_marking_, its dGraph and lethal_map_
// persistent in HBM.  include/dddmr_rollout.h restates the semantics; this file is the glue between three slices that
// are parity-tested on their own:
//   the verdict of a stored marking      dc_marking_verdict (depth_clear.hip.h), here fed from the device store
//   the clusters addPCPtr is called with depth_mark_enqueue (depth_mark.hip.h)
//   store, pool, dGraph, housekeeping    the marking store both layers share (marking_store.hip.h) and the lidar layer's
//                                        general route (marking.hip.h): k_mk_unmark, k_mk_proj_keys, k_mk_flags,
//                                        k_mk_group_reduce, k_mk_slots, k_mk_commit, k_mk_dgraph, k_mk_finish
//
// The store is a MarkStore with a MarkHead: per slot, the stored cluster pc_ (the 0.2 m cloud selfClear's engagement test
// searches with) lies in the pool directly in front of the slot's generator points:
//   pool[pc_ofs .. pc_ofs + pc_n)          pc_
//   pool[pts_ofs .. pts_ofs + pts_n)       generator points, pts_ofs = pc_ofs + pc_n
// so the kernels that only read generator points (k_mk_unmark, k_mk_dgraph) fit as they are, and the ones that move a
// slot or give it pool space (rehash, compaction, commit, the contested-voxel fix) carry the head along.
//
// Launch sequence of an update, all on the feeds' stream:
//   [observation grid, when a depth source has published: depth_observation_grid]
//   k_dl_begin                                  counters of the update (the pool fill stays on the device)
//   [k_mk_rehash] [k_mk_compact_sizes, scan, k_mk_compact_move]      housekeeping, rare (store_maintenance)
//   k_dl_window, k_dl_verdicts, k_mk_unmark     selfClear: one lane per alive marking, one wave per marking in the window
//                                               (lanes striding its pc_), one wave per removed marking
//   depth_mark_enqueue                          selfMark up to the clusters' fates (skipped with <= 5 observation points)
//   k_dl_accept, k_mk_proj_keys, sort, k_mk_flags, scan, k_mk_group_reduce      generator points
//   k_mk_slots, k_mk_commit, k_dl_store_pc, k_mk_dgraph                         addPCPtr: one wave per generator point
//   k_mk_finish, k_dl_out                       next update's alive list; counters into pinned, mapped memory
// One host wait.  k_dl_out also hands over the clusters' sizes, states and slots when (and only when) a voxel was
// contested; the host then replays the reference's sort (store_tie_fixes) and k_mk_fix_owner re-commits the voxels whose
// keeper differs: the second wait of such an update.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "depth_mark.hip.h"
#include "dev_memory.hip.h"   // Owned, dev_alloc, Drain
#include "wave_ops.hip.h"     // wave_append

#pragma clang fp contract(off)

namespace dddmr {

struct DlStore {              // what selfClear's two kernels take of the store beside MarkStore (device pointers)
  uint32_t* pc_ofs;           // [table] the store's MarkHead: first point of the stored pc_ in the pool
  uint32_t* pc_n;             // [table]
  uint32_t* clear_list;       // [table] alive slots inside selfClear's window, this update
};
struct DlCounters {           // counted by k_dl_accept
  uint32_t n_kept;            // clusters of at least min_cluster_size points
  uint32_t n_accepted;        // addPCPtr calls
};
struct DlOut {                // host-mapped: what an update reports
  MarkCounters c;
  DlCounters x;
  uint32_t mark_overflow;     // the cluster pipeline's capacity flag (VoxelGrid key range)
  uint32_t n_clusters;        // all clusters, the ones below the minimum size included (rows of the tie arrays)
};

__global__ void k_dl_begin(MarkCounters* __restrict__ cnt, DlCounters* __restrict__ x) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t pool_used = cnt->pool_used;
  uint32_t* w = reinterpret_cast<uint32_t*>(cnt);
  for (uint32_t i = 0; i < sizeof(MarkCounters) / sizeof(uint32_t); ++i) w[i] = 0u;
  cnt->pool_used = pool_used;
  x->n_kept = 0u;
  x->n_accepted = 0u;
}

// selfClear's window (:280-318): one lane per alive marking; keys in [min, max) on every axis because of lower_bound
__global__ __launch_bounds__(256) void k_dl_window(MarkParams k, MarkStore s, DlStore d, MarkCounters* __restrict__ cnt) {
  const uint32_t w = blockIdx.x * 256 + threadIdx.x;
  bool in = false;
  uint32_t slot = 0;
  if (w < k.n_alive_prev) {
    slot = s.alive_list[w];
    if (s.alive[slot]) {
      int x, y, z;
      voxel_unkey(s.keys[slot], &x, &y, &z);
      in = !(x < k.wx0 || x >= k.wx1 || y < k.wy0 || y >= k.wy1 || z < k.wz0 || z >= k.wz1);
    }
  }
  const uint32_t at = wave_append(in, &cnt->n_in_window);
  if (in) d.clear_list[at] = slot;
}

// The verdict of every marking in the window, one wave each, lanes striding its stored pc_ (as k_dc_verdicts does with
// the markings a host ships); a marking that is not kept is removed: Marking::removePCPtr, its node loop in k_mk_unmark.
__global__ __launch_bounds__(256) void k_dl_verdicts(MarkParams k, DcFrustums S, const PointGrid* __restrict__ hdr, uint32_t observation_clear,
                                                     MarkStore s, DlStore d, MarkCounters* __restrict__ cnt) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= cnt->n_in_window) return;                     // wave-uniform
  const int lane = threadIdx.x & 63;
  const uint32_t slot = d.clear_list[w];
  int x, y, z;
  voxel_unkey(s.keys[slot], &x, &y, &z);
  const uint32_t ofs = d.pc_ofs[slot], n = d.pc_n[slot];
  const float4* __restrict__ pool = s.pool;
  const uint2 v = dc_marking_verdict(k.res, k.hres, observation_clear != 0, S, hdr, x, y, z, n, lane, [&](uint32_t j) {
    const float4 p = pool[ofs + j];
    return make_float3(p.x, p.y, p.z);
  });
  if (!(v.x & 1u) && lane == 0) {
    s.alive[slot] = 0;
    s.removed_seq[slot] = k.seq;
    atomicAdd(&cnt->n_cleared, 1u);
    s.removed_list[atomicAdd(&cnt->n_removed, 1u)] = slot;
  }
}

// After k_dm_stage2: the accepted clusters get the state the general route's kernels look for (2), the generator
// bookkeeping is reset, the clusters are counted.  One lane per cluster.
__global__ __launch_bounds__(64) void k_dl_accept(const MarkCounters* __restrict__ cnt_in, const uint32_t* __restrict__ fate, ClusterArrays c,
                                                  DlCounters* __restrict__ x) {
  const uint32_t ci = blockIdx.x * 64 + threadIdx.x;
  bool kept = false, acc = false;
  if (ci < cnt_in->n_clusters) {
    const uint32_t f = fate[ci];
    kept = f != kDmBelowMin;
    acc = f == kDmAccepted;
    c.state[ci] = acc ? 2u : 0u;
    c.gen_count[ci] = 0;
    c.gen_first[ci] = 0xFFFFFFFFu;
  }
  const uint32_t nk = (uint32_t)__popcll(__ballot(kept)), na = (uint32_t)__popcll(__ballot(acc));
  if (threadIdx.x == 0) {
    if (nk) atomicAdd(&x->n_kept, nk);
    if (na) atomicAdd(&x->n_accepted, na);
  }
}

// After k_mk_commit: the 0.2 m points of the owners into the pool, one lane per point (the generator points go with k_mk_dgraph)
__global__ __launch_bounds__(256) void k_dl_store_pc(const uint32_t* __restrict__ n_ds, const float4* __restrict__ ds,
                                                     const uint32_t* __restrict__ ds_first, const uint32_t* __restrict__ pc_dst,
                                                     float4* __restrict__ pool) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= *n_ds) return;
  const float4 p = ds[g];
  const uint32_t ci = (uint32_t)__float_as_int(p.w);
  const uint32_t po = pc_dst[ci];
  if (po != 0xFFFFFFFFu) pool[po + (g - ds_first[ci])] = make_float4(p.x, p.y, p.z, 0.f);
}

// The update's counters into pinned, mapped memory; with a contested voxel also every cluster's size, state and slot
// (tie[0 .. N), [N .. 2N), [2N .. 3N)) for the host's replay of the reference's sort.
__global__ __launch_bounds__(256) void k_dl_out(uint32_t marked, uint32_t stride, const MarkCounters* __restrict__ cnt,
                                                const DlCounters* __restrict__ x, const MarkCounters* __restrict__ cnt_mark, ClusterArrays c,
                                                DlOut* __restrict__ out, uint32_t* __restrict__ tie) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t nc = marked ? cnt_mark->n_clusters : 0u;
  if (i == 0) {
    out->c = *cnt;
    out->x = *x;
    out->mark_overflow = marked ? cnt_mark->overflow : 0u;
    out->n_clusters = nc;
  }
  if (cnt->n_dup > 0 && i < nc && i < stride) {
    tie[i] = c.size[i];
    tie[stride + i] = c.state[i];
    tie[2 * (size_t)stride + i] = c.state[i] == 2u ? c.slot[i] : 0u;
  }
}

}  // namespace dddmr

// ---- host ---------------------------------------------------------------------------------------------------------
namespace {

struct DepthLayerState {
  dddmr_depth_layer_config cfg{};
  uint32_t max_obs = 0;
  std::unique_ptr<DepthMarkState> dm;      // the cluster pipeline's scratch (rocPRIM storage included) and the ground / map grids
  StoreBuf store;                          // with heads; its pool_used persists on the device between updates
  // scratch of one update beside dm's (sized for max_obs)
  float4 *proj = nullptr, *gen = nullptr;
  uint32_t *gen_first = nullptr, *gen_count = nullptr, *slot = nullptr, *pc_dst = nullptr, *gen_dst = nullptr;
  uint32_t* n_gen = nullptr;
  DlCounters* extra = nullptr;
  Owned mem;                               // (of the above and out_host)
  void* out_host = nullptr;                // DlOut, tie arrays [3 * max_obs], fix list [max_obs / 2] uint2
  void* out_dev = nullptr;
  uint32_t seq = 0;
};

static_assert(!std::is_copy_constructible_v<DepthLayerState>);

int depth_layer_init(dddmr_rollout_ctx* ctx, DepthLayerState* s, const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                     const float* map_xyz, size_t n_map, size_t map_stride_bytes) {
  if (store_alloc(s->store, 8, s->cfg.max_markings, s->cfg.max_cluster_points, (uint32_t)n_ground, false, true) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "depth_layer_create: the marking store's allocation failed");
  s->dm = std::make_unique<DepthMarkState>();
  s->dm->cfg.xy_resolution = s->cfg.xy_resolution;
  s->dm->cfg.height_resolution = s->cfg.height_resolution;
  s->dm->cfg.euclidean_cluster_extraction_tolerance = s->cfg.euclidean_cluster_extraction_tolerance;
  s->dm->cfg.euclidean_cluster_extraction_min_cluster_size = s->cfg.euclidean_cluster_extraction_min_cluster_size;
  s->dm->cfg.segmentation_ignore_ratio = s->cfg.segmentation_ignore_ratio;
  s->dm->cfg.max_observation_points = s->cfg.max_observation_points;
  s->dm->max_obs = s->max_obs;
  const int rc = depth_mark_init(ctx, s->dm.get(), s->store.table, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes);
  if (rc != DDDMR_OK) return rc;
  const size_t N = s->max_obs;
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->proj, N));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->gen, N));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->gen_first, N));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->gen_count, N));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->slot, N));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->pc_dst, N));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->gen_dst, N));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->n_gen, 1));
  HIPCHK(ctx, dev_alloc(s->mem.dev, &s->extra, 1));
  const size_t bytes = sizeof(DlOut) + 3 * N * sizeof(uint32_t) + (N / 2 + 1) * sizeof(uint2);
  if (host_mapped_alloc(s->mem.host, &s->out_host, &s->out_dev, bytes) != 0) return fail(ctx, DDDMR_ERR_HIP, "depth_layer_create: staging of %zu bytes", bytes);
  return store_reset(ctx, s->store, ctx->copy_stream, s->cfg.max_obstacle_distance);      // resetdGraph.  producer_mu held.
}

#define DL_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); ++ops; } while (0)

DepthLayerState* depth_layer_of(dddmr_rollout_ctx* ctx, const char* what) {
  if (!ctx->dlayer) (void)fail(ctx, DDDMR_ERR_STATE, "%s before depth_layer_create", what);
  return ctx->dlayer.get();
}

int depth_layer_update_locked(dddmr_rollout_ctx* ctx, const double T_gbl_base[7], dddmr_depth_layer_stats* stats);

}  // namespace

extern "C" {

int dddmr_rollout_depth_layer_create(dddmr_rollout_ctx* ctx, const dddmr_depth_layer_config* cfg, const float* ground_xyz,
                                     size_t n_ground, size_t ground_stride_bytes, const float* map_xyz, size_t n_map,
                                     size_t map_stride_bytes) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  if (!cloud_arg_ok(ground_xyz, n_ground, ground_stride_bytes) || !cloud_arg_ok(map_xyz, n_map, map_stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_layer_create: bad cloud pointer / stride");
  const double positive[] = {cfg->xy_resolution, cfg->height_resolution, cfg->euclidean_cluster_extraction_tolerance,
                             cfg->inflation_radius, cfg->perception_window_size, cfg->marking_height};
  for (double v : positive)
    if (!(v > 0) || !std::isfinite(v))
      return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_layer_create: resolutions, tolerance, inflation radius, window and marking height must be positive and finite");
  if (!std::isfinite(cfg->segmentation_ignore_ratio) || !std::isfinite(cfg->inscribed_radius) || !std::isfinite(cfg->max_obstacle_distance) ||
      cfg->euclidean_cluster_extraction_min_cluster_size < 0 || cfg->max_observation_points == 0 || cfg->max_markings == 0 ||
      cfg->max_cluster_points == 0)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_layer_create: non-finite parameter, negative minimum cluster size or a capacity of 0");
  // the sort keys of an update carry the observation point index in 20 bits, as depth_mark_create's do
  if (n_ground >= (1u << 30) || n_map >= (1u << 30) || cfg->max_observation_points > kMarkMaxObs || cfg->max_markings > (1u << 24) ||
      cfg->max_cluster_points > (1u << 30))
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_create: at most %u observation points, 2^24 markings, 2^30 pool points", kMarkMaxObs);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);          // the static grids are built on the tick's stream
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "depth_layer_create while a tick_begin is pending");
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  auto s = std::make_unique<DepthLayerState>();
  s->cfg = *cfg;
  s->max_obs = cfg->max_observation_points;
  const int rc = depth_layer_init(ctx, s.get(), ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes);
  if (rc != DDDMR_OK) return rc;                         // (the old layer and its stack survive a failed create)
  ctx->stack.reset();                                    // (a stack holds the layer it was created over)
  ctx->dlayer.reset(s.release());                        // only a complete state is ever visible
  return DDDMR_OK;
}

int dddmr_rollout_depth_layer_reset(dddmr_rollout_ctx* ctx) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_reset");
  if (!s) return DDDMR_ERR_STATE;
  return store_reset(ctx, s->store, ctx->copy_stream, s->cfg.max_obstacle_distance);
}

int dddmr_rollout_depth_layer_update(dddmr_rollout_ctx* ctx, const double T_gbl_base[7], dddmr_depth_layer_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!T_gbl_base || !stats) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_layer_update: null argument");
  for (int i = 0; i < 7; ++i)
    if (!std::isfinite(T_gbl_base[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_layer_update: non-finite transform");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  return depth_layer_update_locked(ctx, T_gbl_base, stats);
}

}  // extern "C"

namespace {
// One pass of the layer; producer_mu held, arguments checked.
int depth_layer_update_locked(dddmr_rollout_ctx* ctx, const double T_gbl_base[7], dddmr_depth_layer_stats* stats) {
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_update");
  if (!s) return DDDMR_ERR_STATE;
  DcFrustums S;
  int rc = depth_frustums(ctx, "depth_layer_update", &S);
  if (rc != DDDMR_OK) return rc;
  const size_t n_obs = ctx->sources.depth_points();
  if (n_obs > s->max_obs)
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_update: %zu observation points, max_observation_points %u", n_obs, s->max_obs);
  if ((rc = depth_clear_scratch(ctx, "depth_layer_update")) != DDDMR_OK) return rc;
  DepthClear& d = *ctx->dclear;
  hipStream_t st = ctx->copy_stream;      // the stream the depth feeds ran on: their frames are complete before this work
  uint32_t ops = 0;
  const bool observation_clear = !(n_obs > 5);           // :258-264, :491-492
  Drain drain{st};                        // from the first enqueue to either wait: an error exit in between waits for the stream
  if (!observation_clear && (rc = depth_observation_grid(ctx, d, n_obs, st, &ops)) != DDDMR_OK) return rc;
  const uint32_t n = (uint32_t)n_obs;
  const dddmr_depth_layer_config& c = s->cfg;
  DepthMarkState* dm = s->dm.get();
  StoreBuf& sb = s->store;
  MarkStore& m = sb.s;

  MarkParams k{};
  k.res = c.xy_resolution; k.hres = c.height_resolution; k.marking_height = c.marking_height; k.window = c.perception_window_size;
  k.inscribed = c.inscribed_radius; k.inflation = c.inflation_radius;
  mark_params_pose(k, T_gbl_base);
  k.n_obs = n;
  k.pad = kDcPad;
  k.table_mask = sb.table - 1;
  k.pool_cap = sb.pool_cap;
  k.n_ground = sb.n_ground;
  k.seq = next_seq(s->seq);

  dddmr_depth_layer_stats out{};
  out.n_observation = n;
  DL_LAUNCH(k_dl_begin, dim3(1), dim3(64), 0, st, sb.counters, s->extra);
  StoreOps hk;
  const int runs = store_maintenance(ctx, sb, st, dm->sc.temp, dm->sc.temp_bytes, hk);
  ops += hk.kernels + hk.other;
  if (runs < 0) return fail(ctx, DDDMR_ERR_HIP, "depth_layer_update: housekeeping failed");
  out.gc_runs = (uint32_t)runs;
  k.n_alive_prev = sb.n_alive;
  // ---- selfClear against the current observation ----
  if (sb.n_alive > 0) {
    const DlStore ds{sb.head.pc_ofs, sb.head.pc_n, sb.clear_list};
    DL_LAUNCH(k_dl_window, dim3((sb.n_alive + 255) / 256), dim3(256), 0, st, k, m, ds, sb.counters);
    DL_LAUNCH(k_dl_verdicts, dim3((sb.n_alive + 3) / 4), dim3(256), 0, st, k, S, d.hdr, observation_clear ? 1u : 0u, m, ds, sb.counters);
    DL_LAUNCH(k_mk_unmark, dim3((sb.n_alive + 3) / 4), dim3(256), 0, st, k, m, dm->grids.ground.g, sb.counters);
  }
  // ---- selfMark ----
  ClusterArrays cl = dm->sc.cl;
  cl.gen_first = s->gen_first;
  cl.gen_count = s->gen_count;
  cl.slot = s->slot;
  if (!observation_clear) {
    if ((rc = depth_mark_enqueue(ctx, dm, T_gbl_base, d, n, S, st, &ops)) != DDDMR_OK) return rc;
    const dim3 pb((n + 255) / 256), cb((n + 63) / 64);
    DL_LAUNCH(k_dl_accept, cb, dim3(64), 0, st, dm->counters, dm->fate, cl, s->extra);
    // projection on the base plane + 0.1 m VoxelGrid of the accepted clusters -> generator points (keyed like the 0.2 m one)
    const int ox = (int)std::floor((float)T_gbl_base[0] / 0.1f) - kVgHalfXY, oy = (int)std::floor((float)T_gbl_base[1] / 0.1f) - kVgHalfXY,
              oz = (int)std::floor((float)T_gbl_base[2] / 0.1f) - kVgHalfZ;
    DL_LAUNCH(k_mk_proj_keys, pb, dim3(256), 0, st, k, dm->sc.n_groups, dm->sc.ds, cl, ox, oy, oz, s->proj, dm->sc.keys_a, dm->sc.vals_a, n, sb.counters);
    size_t tb = dm->sc.temp_bytes;
    HIPCHK(ctx, rocprim::radix_sort_pairs(dm->sc.temp, tb, dm->sc.keys_a, dm->sc.keys_b, dm->sc.vals_a, dm->sc.vals_b, (size_t)n, 0, 62, st));
    DL_LAUNCH(k_mk_flags, pb, dim3(256), 0, st, n, dm->sc.keys_b, 0, dm->sc.flags);
    tb = dm->sc.temp_bytes;
    HIPCHK(ctx, rocprim::inclusive_scan(dm->sc.temp, tb, dm->sc.flags, dm->sc.incl, (size_t)n, rocprim::plus<uint32_t>(), st));
    DL_LAUNCH(k_mk_group_reduce, cb, dim3(64), 0, st, n, dm->sc.keys_b, dm->sc.vals_b, dm->sc.flags, dm->sc.incl, 1, dm->sc.keys1, s->proj, s->gen,
              cl.gen_count, cl.gen_first, s->n_gen);
    // addPCPtr
    DL_LAUNCH(k_mk_slots, cb, dim3(64), 0, st, k, dm->counters, cl, m, sb.counters);
    DL_LAUNCH(k_mk_commit, cb, dim3(64), 0, st, k, dm->counters, cl, m, sb.head, sb.counters, s->pc_dst, s->gen_dst);
    DL_LAUNCH(k_dl_store_pc, pb, dim3(256), 0, st, dm->sc.n_groups, dm->sc.ds, dm->sc.ds_first, s->pc_dst, m.pool);
    DL_LAUNCH(k_mk_dgraph, dim3((n + 3) / 4), dim3(256), 0, st, k, s->n_gen, s->gen, cl, s->gen_dst, m, dm->grids.ground.g);
    ops += 3 * 10 + 3 * 3 + 2;            // rocPRIM, estimated: three sorts (block sort + ~8 merge passes + id wrapper), three scans; two memsets
  }
  DL_LAUNCH(k_mk_finish, dim3((sb.table + 255) / 256), dim3(256), 0, st, k, m, sb.counters);
  char* dev = static_cast<char*>(s->out_dev);
  char* host = static_cast<char*>(s->out_host);
  const size_t tie_at = sizeof(DlOut), fix_at = tie_at + 3 * (size_t)s->max_obs * sizeof(uint32_t);
  DL_LAUNCH(k_dl_out, dim3(observation_clear ? 1u : (n + 255) / 256), dim3(256), 0, st, observation_clear ? 0u : 1u, s->max_obs, sb.counters,
            s->extra, dm->counters, cl, reinterpret_cast<DlOut*>(dev), reinterpret_cast<uint32_t*>(dev + tie_at));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));                 // the update's one host wait
  drain.armed = false;
  out.host_waits = 1;
  DlOut o = *reinterpret_cast<const DlOut*>(host);
  if (o.c.n_dup > 0 && !o.c.overflow && !o.mark_overflow) {
    const uint32_t* tie = reinterpret_cast<const uint32_t*>(host + tie_at);
    std::vector<uint2> fix;
    rc = store_tie_fixes(ctx, "depth_layer_update", s->max_obs, c.euclidean_cluster_extraction_min_cluster_size, o.n_clusters, tie,
                         tie + s->max_obs, tie + 2 * (size_t)s->max_obs, fix);
    if (rc != DDDMR_OK) return rc;
    if (!fix.empty()) {
      const uint32_t n_fix = (uint32_t)fix.size();
      std::memcpy(host + fix_at, fix.data(), fix.size() * sizeof(uint2));
      drain.armed = true;
      DL_LAUNCH(k_mk_fix_owner, dim3((n_fix + 3) / 4), dim3(256), 0, st, k, n_fix, reinterpret_cast<const uint2*>(dev + fix_at), dm->sc.ds,
                dm->sc.ds_first, s->gen, cl, m, sb.head, sb.counters);
      DL_LAUNCH(k_dl_out, dim3(1), dim3(256), 0, st, 0u, s->max_obs, sb.counters, s->extra, dm->counters, cl, reinterpret_cast<DlOut*>(dev),
                reinterpret_cast<uint32_t*>(dev + tie_at));
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipStreamSynchronize(st));             // the second wait of an update with a contested voxel
      drain.armed = false;
      out.host_waits = 2;
      const DlOut o2 = *reinterpret_cast<const DlOut*>(host);
      o.c.pool_used = o2.c.pool_used;
      o.c.overflow |= o2.c.overflow;
    }
  }
  sb.pool_used = o.c.pool_used;
  sb.n_alive = o.c.n_alive;
  sb.keys_used += o.c.n_new_keys;
  out.n_in_window = o.c.n_in_window;
  out.n_cleared = o.c.n_cleared;
  out.n_clusters = o.x.n_kept;
  out.n_accepted = o.x.n_accepted;
  out.n_contested = o.c.n_dup;
  out.n_alive = o.c.n_alive;
  out.launches = ops;
  *stats = out;
  if (o.c.overflow || o.mark_overflow)
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_update: capacity flag %u (1: max_markings, 2: max_cluster_points, 4: a cluster point beyond the VoxelGrid key range around the robot)",
                o.c.overflow | o.mark_overflow);
  return DDDMR_OK;
}
#undef DL_LAUNCH
}  // namespace

extern "C" {

int dddmr_rollout_depth_layer_get_voxels(dddmr_rollout_ctx* ctx, int32_t* xyz_out, size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_get_voxels");
  if (!s) return DDDMR_ERR_STATE;
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  return store_read_voxels(ctx, s->store, "depth_layer_get_voxels", xyz_out, capacity, n);
}

int dddmr_rollout_depth_layer_get_clusters(dddmr_rollout_ctx* ctx, int32_t* voxel_out, uint32_t* offsets_out, float* xyz_out,
                                           size_t cap_markings, size_t cap_points, size_t* n_markings, size_t* n_points) {
  if (!ctx || !n_markings || !n_points) return DDDMR_ERR_BAD_ARG;
  const int n_out = (voxel_out != nullptr) + (offsets_out != nullptr) + (xyz_out != nullptr);
  if (n_out != 0 && n_out != 3) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_layer_get_clusters: the outputs are all given or all NULL (counts only)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_get_clusters");
  if (!s) return DDDMR_ERR_STATE;
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  std::vector<StoreSlot> slots;
  int rc = store_read_slots(ctx, s->store, true, slots);
  if (rc != DDDMR_OK) return rc;
  const size_t nm = slots.size();
  size_t np = 0;
  for (const StoreSlot& sl : slots) np += sl.n;
  *n_markings = nm;
  *n_points = np;
  if (n_out == 0) return DDDMR_OK;
  if (nm > cap_markings || np > cap_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_get_clusters: %zu markings / %zu points, capacity %zu / %zu", nm, np, cap_markings, cap_points);
  std::vector<float4> pool;
  if ((rc = store_read_pool(ctx, s->store, pool)) != DDDMR_OK) return rc;
  size_t mi = 0, at = 0;
  offsets_out[0] = 0;
  for (const StoreSlot& sl : slots) {
    voxel_unkey(sl.key, &voxel_out[3 * mi], &voxel_out[3 * mi + 1], &voxel_out[3 * mi + 2]);
    if ((size_t)sl.ofs + sl.n > pool.size()) return fail(ctx, DDDMR_ERR_STATE, "depth_layer_get_clusters: slot %zu points past the pool", sl.slot);
    for (uint32_t j = 0; j < sl.n; ++j, ++at) {
      const float4 p = pool[(size_t)sl.ofs + j];
      xyz_out[3 * at] = p.x; xyz_out[3 * at + 1] = p.y; xyz_out[3 * at + 2] = p.z;
    }
    offsets_out[++mi] = (uint32_t)at;
  }
  return DDDMR_OK;
}

int dddmr_rollout_depth_layer_get_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity) {
  if (!ctx || !values_out) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_get_dgraph");
  if (!s) return DDDMR_ERR_STATE;
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  return store_read_dgraph(ctx, s->store, "depth_layer_get_dgraph", values_out, capacity);
}

int dddmr_rollout_depth_layer_get_lethal(dddmr_rollout_ctx* ctx, uint8_t* flags_out, size_t capacity) {
  if (!ctx || !flags_out) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_get_lethal");
  if (!s) return DDDMR_ERR_STATE;
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  return store_read_lethal(ctx, s->store, "depth_layer_get_lethal", flags_out, capacity);
}

}  // extern "C"
