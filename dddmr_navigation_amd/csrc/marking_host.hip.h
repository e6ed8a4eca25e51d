// marking_host.hip.h -- host side of the global-mode marking / clearing layer (included by
// rollout_engine.hip after the context and its helpers are defined): device state, the per-update
// launch sequence and the dddmr_rollout_marking_* entry points of include/dddmr_rollout.h.
#pragma once

#include "dev_memory.hip.h"      // DevScope, Drain, wait_seq
#include "marking.hip.h"
#include "marking_fused.hip.h"
#include "marking_plan.hip.h"
#include "marking_store.hip.h"

namespace {

using namespace dddmr;

constexpr uint32_t kMarkMaxObs = 1u << 20;   // points of one observation (20-bit point index inside the sort keys)

// The rocPRIM temporary storage a ClusterScratch for observations of up to N points needs: the largest request among the
// sorts and scans of the cluster pipeline, the static grids' builder (up to 2^22 cells) and the housekeeping of a marking
// store of `table` slots that scans with it (0: none).  rocPRIM asks the device, hence the stream.
int cluster_temp_bytes(dddmr_rollout_ctx* ctx, size_t N, size_t table, size_t* bytes) {
  size_t a = 0, b = 0, e = 0, d = 0;
  unsigned long long* k = nullptr;
  uint32_t* v = nullptr;
  HIPCHK(ctx, rocprim::radix_sort_keys(nullptr, a, k, k, N, 0, 40, ctx->stream));
  HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, b, k, k, v, v, N, 0, 62, ctx->stream));
  HIPCHK(ctx, rocprim::exclusive_scan(nullptr, e, v, v, 0u, std::max((size_t)(1u << 22) + 1, table), rocprim::plus<uint32_t>(), ctx->stream));
  HIPCHK(ctx, rocprim::inclusive_scan(nullptr, d, v, v, std::max(N, table), rocprim::plus<uint32_t>(), ctx->stream));
  *bytes = std::max({a, b, e, d, (size_t)4096}) + 256;
  return DDDMR_OK;
}

struct MarkingState {
  dddmr_marking_config cfg{};
  uint32_t max_obs = 0;
  StaticGrids grids;
  GridBuf obs[2];
  int prev = -1;              // obs[] entry holding pcl_msg_gbl_ of the last selfMark, -1 = none yet
  uint32_t n_prev = 0;
  StoreBuf store;             // its counters also count the update's clusters
  ClusterScratch sc;          // scratch of one update (sized for max_obs), with the layer's own below
  uint2* gslot = nullptr;
  float4 *proj = nullptr, *gen = nullptr;
  uint32_t* pool_ofs = nullptr;
  Owned mem;                  // the device allocations of this struct itself, and host_out
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  uint32_t seq = 0;
  // fused route (marking_fused.hip.h)
  float4* unmark_pts = nullptr;            // [pool_cap]
  float4* band_pts = nullptr;              // [2][kBandMax * kBandCap]: generator points of this update / of removed markings, by row of ground cells
  uint32_t* band_cnt = nullptr;            // [2][kBandMax], all zero between updates
  uint32_t* hi_rank = nullptr;             // [8][kFuseMaxObs - kFuseRegObs] grid builder scratch for observations past kFuseRegObs points
  uint32_t* cell_count = nullptr;          // [kFuseMaxCells], all zero between updates
  bool alive_list_stale = false;           // the fused route keeps no alive list: the general route rebuilds it first
  uint32_t* ticket = nullptr;              // [2]
  MarkCounters* host_out = nullptr;        // host-mapped, host_out_dev = its device address
  MarkCounters* host_out_dev = nullptr;
  bool counters_clean = false;             // device counters zeroed (pool fill kept) by the last fused update
  int route = -1;                          // DDDMR_MARKING_ROUTE: -1 by size, 0 general (rocPRIM), 1 fused only
  uint32_t updates_fused = 0, updates_general = 0, launches_last = 0;
  float last_clear_ms = 0.f, last_mark_ms = 0.f;
  hipStream_t own_stream = nullptr;        // the update's stream while a tick_begin is pending (else the context's)
  hipStream_t cur = nullptr;               // stream of the update in progress
  uint32_t updates_overlapped = 0;
  MarkKnobs knobs;                         // the DDDMR_MKF_* variables (marking_plan.hip.h)
  ~MarkingState() {
    if (own_stream) (void)hipStreamDestroy(own_stream);
    for (hipEvent_t e : {e0, e1, e2})
      if (e) (void)hipEventDestroy(e);
  }
};
static_assert(!std::is_copy_constructible_v<MarkingState>);

int upload_static(dddmr_rollout_ctx* ctx, DevAllocs& mem, void* temp, size_t temp_bytes, GridBuf& b, float4** dev, const float* xyz, size_t n,
                  size_t stride_bytes, float cell_xy, float cell_z) {
  const HostCloud h(xyz, n, stride_bytes);
  if (!small_pad_extent_ok(h.lo, h.hi))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "static cloud of %zu points: wider than %g m on an axis, beyond what the search boxes' pad of 1e-4 m covers", n,
                (double)kSmallPadMaxExtent);
  HIPCHK(ctx, dev_alloc(mem, dev, h.pts.size()));
  HIPCHK(ctx, hipMemcpy(*dev, h.pts.data(), h.pts.size() * sizeof(float4), hipMemcpyHostToDevice));
  grid_shape(b.g, h.lo, h.hi, cell_xy, cell_z, 1u << 22);
  if (grid_alloc(mem, b, (uint32_t)((size_t)b.g.nx * b.g.ny * b.g.nz), (uint32_t)n) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "static grid of %zu points: allocation failed", n);
  {
    std::vector<uint32_t> rows((size_t)b.g.ny * b.g.nz, 0u);
    for (size_t i = 0; i < n; ++i) ++rows[(size_t)host_cz(b.g, h.pts[i].z) * b.g.ny + host_cy(b.g, h.pts[i].y)];
    b.max_row = 0;
    for (uint32_t r : rows) b.max_row = std::max(b.max_row, r);
  }
  DevScope scope;
  uint2* slot = nullptr;
  HIPCHK(ctx, dev_alloc(scope.mem, &slot, std::max<size_t>(n, 1)));
  Drain drain{ctx->stream};                  // behind `scope`: an error exit waits before the builder's scratch is freed
  const int rb = grid_build(ctx, temp, temp_bytes, b, *dev, (uint32_t)n, slot, ctx->stream);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  drain.armed = false;
  return rb;
}

// the ground (0.5 m cells, one layer in z) and the static map (0.25 m cells)
int static_grids_upload(dddmr_rollout_ctx* ctx, StaticGrids& g, void* temp, size_t temp_bytes, const float* ground_xyz, size_t n_ground,
                        size_t ground_stride_bytes, const float* map_xyz, size_t n_map, size_t map_stride_bytes) {
  g.n_ground = (uint32_t)n_ground;
  g.n_map = (uint32_t)n_map;
  const int rc = upload_static(ctx, g.mem.dev, temp, temp_bytes, g.ground, &g.ground_pts, ground_xyz, n_ground, ground_stride_bytes, 0.5f, 1e6f);
  if (rc != DDDMR_OK) return rc;
  return upload_static(ctx, g.mem.dev, temp, temp_bytes, g.map, &g.map_pts, map_xyz, n_map, map_stride_bytes, 0.25f, 0.25f);
}

// Contested voxels (store_tie_fixes): the clusters' sizes, states and slots come to the host with three copies, and the
// voxels whose keeper differs are re-committed.
int marking_fix_ties(dddmr_rollout_ctx* ctx, MarkingState* m, const MarkParams& k, MarkCounters& out) {
  const uint32_t nc = out.n_clusters;
  if (nc == 0) return DDDMR_OK;
  hipStream_t st = m->cur;
  std::vector<uint32_t> size(nc), state(nc), slot(nc);
  std::vector<uint2> fix;
  MarkCounters after{};                                // (on the fused route the device copy holds only what k_mk_fix_owner touches)
  Drain drain{st};                                     // behind what the copies read and write: an error exit waits before they die
  HIPCHK(ctx, hipMemcpyAsync(size.data(), m->sc.cl.size, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(state.data(), m->sc.cl.state, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(slot.data(), m->sc.cl.slot, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  drain.armed = false;
  const int rc = store_tie_fixes(ctx, "marking_update", m->max_obs, m->cfg.euclidean_cluster_extraction_min_cluster_size, nc, size.data(),
                                 state.data(), slot.data(), fix);
  if (rc != DDDMR_OK || fix.empty()) return rc;
  // (vals_b is scratch of the update that just finished: >= max_obs words)
  uint2* fix_dev = reinterpret_cast<uint2*>(m->sc.vals_b);
  drain.armed = true;
  HIPCHK(ctx, hipMemcpyAsync(fix_dev, fix.data(), fix.size() * sizeof(uint2), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_mk_fix_owner, dim3((unsigned)((fix.size() + 3) / 4)), dim3(256), 0, st, k, (uint32_t)fix.size(), fix_dev,
                     (const float4*)nullptr, (const uint32_t*)nullptr, m->gen, m->sc.cl, m->store.s, m->store.head, m->store.counters);
  HIPCHK(ctx, hipMemcpyAsync(&after, m->store.counters, sizeof(after), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));               // (also keeps `fix` alive until the copy has run)
  drain.armed = false;
  HIPCHK(ctx, hipGetLastError());
  out.pool_used = after.pool_used;
  out.overflow |= after.overflow;
  if (after.overflow) m->counters_clean = false;
  m->store.pool_used = out.pool_used;
  return DDDMR_OK;
}

int marking_reset_locked(dddmr_rollout_ctx* ctx, struct MarkingState* m);
int marking_update_on(dddmr_rollout_ctx* ctx, struct MarkingState* m, const float4* obs, uint32_t n_obs, const double T_base_sensor[7],
                      const double T_gbl_base[7], dddmr_marking_stats* stats);

}  // namespace

extern "C" {

int dddmr_rollout_marking_create(dddmr_rollout_ctx* ctx, const dddmr_marking_config* cfg, const float* ground_xyz,
                                 size_t n_ground, size_t ground_stride_bytes, const float* map_xyz, size_t n_map,
                                 size_t map_stride_bytes) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  if (!cloud_arg_ok(ground_xyz, n_ground, ground_stride_bytes) || !cloud_arg_ok(map_xyz, n_map, map_stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "marking_create: bad cloud pointer / stride");
  if (!(cfg->xy_resolution > 0) || !(cfg->height_resolution > 0) || !(cfg->euclidean_cluster_extraction_tolerance > 0) ||
      !(cfg->inflation_radius > 0) || cfg->max_markings == 0 || cfg->max_cluster_points == 0)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "marking_create: resolutions, tolerance, inflation radius and capacities must be positive");
  if (n_ground >= (1u << 30) || cfg->max_markings > (1u << 24)) return fail(ctx, DDDMR_ERR_CAPACITY, "marking_create: too large");
  // the sort keys of an update carry the observation point index in 20 bits ((root << 20) | i, cluster id << 42)
  if (ctx->cfg.max_points > kMarkMaxObs)
    return fail(ctx, DDDMR_ERR_CAPACITY, "marking_create: the context's max_points %u exceeds the layer's %u-point observations",
                ctx->cfg.max_points, kMarkMaxObs);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "marking_create while a tick_begin is pending");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->stack.reset();                                    // (a stack holds the layer it was created over)
  ctx->marking.reset();                                  // (the old layer goes first: after a failed create there is none)
  auto m = std::make_unique<MarkingState>();
  m->cfg = *cfg;
  m->max_obs = ctx->cfg.max_points;
  auto init = [&]() -> int {
    const size_t N = m->max_obs;
    size_t temp_bytes = 0;
    if (store_alloc(m->store, 1024, cfg->max_markings, cfg->max_cluster_points, (uint32_t)n_ground, true, false) != 0)
      return fail(ctx, DDDMR_ERR_HIP, "marking_create: the marking store's allocation failed");
    int rc = cluster_temp_bytes(ctx, N, m->store.table, &temp_bytes);
    if (rc != DDDMR_OK) return rc;
    if (cluster_scratch_alloc(m->sc, N, temp_bytes) != 0) return fail(ctx, DDDMR_ERR_HIP, "marking_create: the cluster scratch's allocation failed");
    rc = static_grids_upload(ctx, m->grids, m->sc.temp, m->sc.temp_bytes, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map,
                             map_stride_bytes);
    if (rc != DDDMR_OK) return rc;
    DevAllocs& mem = m->mem.dev;
    for (int i = 0; i < 2; ++i)
      if (grid_alloc(mem, m->obs[i], 1u << 21, (uint32_t)N) != 0) return fail(ctx, DDDMR_ERR_HIP, "marking_create: the observation grids' allocation failed");
    HIPCHK(ctx, dev_alloc(mem, &m->sc.cl.gen_first, N));
    HIPCHK(ctx, dev_alloc(mem, &m->sc.cl.gen_count, N));
    HIPCHK(ctx, dev_alloc(mem, &m->sc.cl.slot, N));
    HIPCHK(ctx, dev_alloc(mem, &m->gslot, N));
    HIPCHK(ctx, dev_alloc(mem, &m->proj, N));
    HIPCHK(ctx, dev_alloc(mem, &m->gen, N));
    HIPCHK(ctx, dev_alloc(mem, &m->pool_ofs, N));
    HIPCHK(ctx, dev_alloc(mem, &m->unmark_pts, m->store.pool_cap));
    HIPCHK(ctx, dev_alloc(mem, &m->band_pts, (size_t)2 * kBandMax * kBandCap));
    HIPCHK(ctx, dev_alloc(mem, &m->band_cnt, (size_t)2 * kBandMax));
    HIPCHK(ctx, dev_alloc(mem, &m->hi_rank, (size_t)8 * (kFuseMaxObs - kFuseRegObs)));
    HIPCHK(ctx, hipMemset(m->band_cnt, 0, (size_t)2 * kBandMax * sizeof(uint32_t)));
    HIPCHK(ctx, dev_alloc(mem, &m->cell_count, kFuseMaxCells));
    HIPCHK(ctx, hipMemset(m->cell_count, 0, (size_t)kFuseMaxCells * sizeof(uint32_t)));
    HIPCHK(ctx, dev_alloc(mem, &m->ticket, 34));
    HIPCHK(ctx, hipMemset(m->ticket, 0, 34 * sizeof(uint32_t)));
    if (host_mapped_alloc(m->mem.host, &m->host_out, &m->host_out_dev, sizeof(MarkCounters)) != 0)
      return fail(ctx, DDDMR_ERR_HIP, "marking_create: host-mapped counters");
    MarkKnobs& kn = m->knobs;
    if (const char* e = std::getenv("DDDMR_MKF_UNMARK")) kn.unmark_with_groups = std::strcmp(e, "roots") != 0;
    if (const char* e = std::getenv("DDDMR_MKF_GRIDPARTS")) { const int v = std::atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8) kn.grid_parts = (uint32_t)v; }
    if (const char* e = std::getenv("DDDMR_MKF_GRID")) kn.grid_in_lds = std::strcmp(e, "global") != 0;
    if (const char* e = std::getenv("DDDMR_MKF_PARTS")) kn.splat_parts = (uint32_t)std::min(128, std::max(0, std::atoi(e)));
    if (const char* e = std::getenv("DDDMR_MKF_UNPARTS")) kn.unmark_parts = (uint32_t)std::min(64, std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("DDDMR_MKF_CELLS")) kn.fuse_cells = std::min<uint32_t>(kFuseMaxCells, std::max(4096, std::atoi(e)));
    if (const char* e = std::getenv("DDDMR_MARKING_ROUTE")) m->route = std::strcmp(e, "general") == 0 ? 0 : (std::strcmp(e, "fused") == 0 ? 1 : -1);
    HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_mkf_groups), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPartLdsBytes));
    HIPCHK(ctx, hipEventCreate(&m->e0));
    HIPCHK(ctx, hipEventCreate(&m->e1));
    HIPCHK(ctx, hipEventCreate(&m->e2));
    return DDDMR_OK;
  };
  int rc = init();
  if (rc == DDDMR_OK) rc = marking_reset_locked(ctx, m.get());
  if (rc == DDDMR_OK) ctx->marking.reset(m.release());   // only a complete state is ever visible
  return rc;
}

int dddmr_rollout_marking_reset(dddmr_rollout_ctx* ctx) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  return marking_reset_locked(ctx, ctx->marking.get());
}

}  // extern "C"

namespace {
// MultiLayerSpinningLidar::resetdGraph (:831-839)
int marking_reset_locked(dddmr_rollout_ctx* ctx, MarkingState* m) {
  if (!m) return fail(ctx, DDDMR_ERR_STATE, "marking_reset before marking_create");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int rc = store_reset(ctx, m->store, ctx->stream, m->cfg.max_obstacle_distance);
  if (rc != DDDMR_OK) return rc;
  m->counters_clean = false;
  m->alive_list_stale = false;               // (nothing alive: the empty list is right)
  // (pcl_msg_gbl_ is untouched by resetdGraph: the previous observation stays)
  return DDDMR_OK;
}

#define MK_LAUNCH(m, ...) do { hipLaunchKernelGGL(__VA_ARGS__); ++(m)->launches_last; } while (0)

// the store's housekeeping (rare); its kernels count as launches of the update
int marking_maintenance(dddmr_rollout_ctx* ctx, MarkingState* m, hipStream_t st) {
  StoreOps ops;
  const int runs = store_maintenance(ctx, m->store, st, m->sc.temp, m->sc.temp_bytes, ops);
  m->launches_last += ops.kernels;
  return runs < 0 ? runs : DDDMR_OK;
}

// selfMark of this observation, general route: rocPRIM sorts, any observation size (marking.hip.h)
int mark_general(dddmr_rollout_ctx* ctx, MarkingState* m, const UpdateFrame& f, const float4* obs, uint32_t n_obs, hipStream_t st) {
  const MarkParams& k = f.k;
  MarkStore& s = m->store.s;
  const int cur = m->prev >= 0 ? 1 - m->prev : 0;
  GridBuf& gb = m->obs[cur];
  float lo[3], hi[3];
  obs_grid_shape(m->cfg, f, gb.cap_cells, gb.g, lo, hi);
  const float4* pts = obs;                   // (the cloud buffer stays pinned until the update returns)
  int rc = grid_build(ctx, m->sc.temp, m->sc.temp_bytes, gb, pts, n_obs, m->gslot, st);
  m->launches_last += 5;                     // memset, count, rocPRIM scan (2 kernels), scatter
  if (rc != DDDMR_OK) return rc;
  const dim3 pb((n_obs + 255) / 256), cb((n_obs + 63) / 64);
  // Euclidean clusters
  MK_LAUNCH(m, k_mk_cc_init, pb, dim3(256), 0, st, n_obs, m->sc.parent);
  MK_LAUNCH(m, k_mk_cc_union, pb, dim3(256), 0, st, k, gb.g, pts, m->sc.parent);
  MK_LAUNCH(m, k_mk_cc_keys, pb, dim3(256), 0, st, n_obs, m->sc.parent, m->sc.keys_a);
  size_t tb = m->sc.temp_bytes;
  HIPCHK(ctx, rocprim::radix_sort_keys(m->sc.temp, tb, m->sc.keys_a, m->sc.keys1, (size_t)n_obs, 0, 40, st));
  MK_LAUNCH(m, k_mk_flags, pb, dim3(256), 0, st, n_obs, m->sc.keys1, 20, m->sc.flags);
  tb = m->sc.temp_bytes;
  HIPCHK(ctx, rocprim::inclusive_scan(m->sc.temp, tb, m->sc.flags, m->sc.cid_incl, (size_t)n_obs, rocprim::plus<uint32_t>(), st));
  MK_LAUNCH(m, k_mk_cluster_starts, pb, dim3(256), 0, st, n_obs, m->sc.flags, m->sc.cid_incl, m->sc.cl, m->store.counters);
  MK_LAUNCH(m, k_mk_cluster_stage1, cb, dim3(64), 0, st, k, m->store.counters, m->sc.cl, m->sc.keys1, pts, m->grids.ground.g);
  // 0.2 m VoxelGrid of every surviving cluster: stable sort by (cluster, voxel), one lane per voxel
  // (voxel indices are keyed relative to the window's centre - half the key range: an observation handed over uncropped may reach far
  // beyond the window -- a margin of 16 voxels around the crop box used to drop such points without a word)
  const float mid[3] = {0.5f * (lo[0] + hi[0]), 0.5f * (lo[1] + hi[1]), 0.5f * (lo[2] + hi[2])};
  const int ox2 = (int)std::floor(mid[0] / 0.2f) - kVgHalfXY, oy2 = (int)std::floor(mid[1] / 0.2f) - kVgHalfXY, oz2 = (int)std::floor(mid[2] / 0.2f) - kVgHalfZ;
  MK_LAUNCH(m, k_mk_ds_keys, pb, dim3(256), 0, st, k, m->sc.keys1, m->sc.cid_incl, m->sc.cl, pts, ox2, oy2, oz2, m->sc.keys_a, m->sc.vals_a, m->store.counters);
  tb = m->sc.temp_bytes;
  HIPCHK(ctx, rocprim::radix_sort_pairs(m->sc.temp, tb, m->sc.keys_a, m->sc.keys_b, m->sc.vals_a, m->sc.vals_b, (size_t)n_obs, 0, 62, st));
  MK_LAUNCH(m, k_mk_flags, pb, dim3(256), 0, st, n_obs, m->sc.keys_b, 0, m->sc.flags);
  tb = m->sc.temp_bytes;
  HIPCHK(ctx, rocprim::inclusive_scan(m->sc.temp, tb, m->sc.flags, m->sc.incl, (size_t)n_obs, rocprim::plus<uint32_t>(), st));
  HIPCHK(ctx, hipMemsetAsync(m->sc.ds_first, 0xFF, (size_t)n_obs * sizeof(uint32_t), st));
  MK_LAUNCH(m, k_mk_group_reduce, cb, dim3(64), 0, st, n_obs, m->sc.keys_b, m->sc.vals_b, m->sc.flags, m->sc.incl, 0, m->sc.keys1, pts, m->sc.ds,
            m->sc.cl.ds_count, m->sc.ds_first, m->sc.n_groups);
  MK_LAUNCH(m, k_mk_cluster_stage2, cb, dim3(64), 0, st, k, m->store.counters, m->sc.cl, m->grids.map.g, m->grids.n_map);
  // projection on the base plane + 0.1 m VoxelGrid of the accepted clusters -> generator points
  const int ox3 = (int)std::floor(mid[0] / 0.1f) - kVgHalfXY, oy3 = (int)std::floor(mid[1] / 0.1f) - kVgHalfXY, oz3 = (int)std::floor(mid[2] / 0.1f) - kVgHalfZ;
  MK_LAUNCH(m, k_mk_proj_keys, pb, dim3(256), 0, st, k, m->sc.n_groups, m->sc.ds, m->sc.cl, ox3, oy3, oz3, m->proj, m->sc.keys_a, m->sc.vals_a, n_obs, m->store.counters);
  tb = m->sc.temp_bytes;
  HIPCHK(ctx, rocprim::radix_sort_pairs(m->sc.temp, tb, m->sc.keys_a, m->sc.keys_b, m->sc.vals_a, m->sc.vals_b, (size_t)n_obs, 0, 62, st));
  MK_LAUNCH(m, k_mk_flags, pb, dim3(256), 0, st, n_obs, m->sc.keys_b, 0, m->sc.flags);
  tb = m->sc.temp_bytes;
  HIPCHK(ctx, rocprim::inclusive_scan(m->sc.temp, tb, m->sc.flags, m->sc.incl, (size_t)n_obs, rocprim::plus<uint32_t>(), st));
  MK_LAUNCH(m, k_mk_group_reduce, cb, dim3(64), 0, st, n_obs, m->sc.keys_b, m->sc.vals_b, m->sc.flags, m->sc.incl, 1, m->sc.keys1, m->proj, m->gen,
            m->sc.cl.gen_count, m->sc.cl.gen_first, m->sc.n_groups + 1);
  m->launches_last += 3 * 10 + 2 * 3 + 1;   // rocPRIM: three sorts (block sort + ~8 merge passes + id wrapper), three scans, memset
  // addPCPtr
  MK_LAUNCH(m, k_mk_slots, cb, dim3(64), 0, st, k, m->store.counters, m->sc.cl, s, m->store.counters);
  MK_LAUNCH(m, k_mk_commit, cb, dim3(64), 0, st, k, m->store.counters, m->sc.cl, s, m->store.head, m->store.counters, (uint32_t*)nullptr, m->pool_ofs);
  MK_LAUNCH(m, k_mk_dgraph, dim3((n_obs + 3) / 4), dim3(256), 0, st, k, m->sc.n_groups + 1, m->gen, m->sc.cl, m->pool_ofs, s, m->grids.ground.g);
  m->prev = cur;                                                               // pcl_msg_gbl_ of this selfMark
  m->n_prev = n_obs;
  return DDDMR_OK;
}

// The tail of an update whose counters live on the device: the alive list, the end event, the counters' copy and the wait.
int finish_on_device(dddmr_rollout_ctx* ctx, MarkingState* m, const MarkParams& k, bool timed, MarkCounters& out) {
  hipStream_t st = m->cur;
  MK_LAUNCH(m, k_mk_finish, dim3((m->store.table + 255) / 256), dim3(256), 0, st, k, m->store.s, m->store.counters);
  if (timed) HIPCHK(ctx, hipEventRecord(m->e2, st));
  HIPCHK(ctx, hipMemcpyAsync(&out, m->store.counters, sizeof(out), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, hipGetLastError());
  return DDDMR_OK;
}

// one update on the general route (~55 launches for a 6 k-point observation)
int update_general(dddmr_rollout_ctx* ctx, MarkingState* m, const UpdateFrame& f, const float4* obs, uint32_t n_obs, bool timed,
                   MarkCounters& out) {
  hipStream_t st = m->cur;
  const MarkParams& k = f.k;
  MarkStore& s = m->store.s;
  MarkCounters zero{};
  zero.pool_used = m->store.pool_used;
  HIPCHK(ctx, hipMemcpyAsync(m->store.counters, &zero, sizeof(zero), hipMemcpyHostToDevice, st));   // (pageable source: copied before return)
  m->counters_clean = false;
  if (timed) HIPCHK(ctx, hipEventRecord(m->e0, st));
  int rc = marking_maintenance(ctx, m, st);
  if (rc != DDDMR_OK) return rc;
  if (m->alive_list_stale) {                 // the last update ran fused: what selfClear walks has to be listed first
    MK_LAUNCH(m, k_mk_finish, dim3((m->store.table + 255) / 256), dim3(256), 0, st, k, s, m->store.counters);
    HIPCHK(ctx, hipMemsetAsync(&m->store.counters->n_alive, 0, sizeof(uint32_t), st));
    m->alive_list_stale = false;
  }
  // ---- selfClear against the previous observation ----
  const PointGrid empty_grid = m->obs[0].g;
  const PointGrid& prev_grid = m->prev >= 0 ? m->obs[m->prev].g : empty_grid;
  if (m->store.n_alive > 0) {
    MK_LAUNCH(m, k_mk_fov, dim3((m->store.n_alive + 255) / 256), dim3(256), 0, st, k, s, m->store.counters);
    MK_LAUNCH(m, k_mk_clear, dim3((m->store.n_alive + 3) / 4), dim3(256), 0, st, k, s, prev_grid, m->store.counters);
    MK_LAUNCH(m, k_mk_unmark, dim3((m->store.n_alive + 3) / 4), dim3(256), 0, st, k, s, m->grids.ground.g, m->store.counters);
  }
  if (timed) HIPCHK(ctx, hipEventRecord(m->e1, st));
  if (n_obs > 5) {                                                               // :320-321
    rc = mark_general(ctx, m, f, obs, n_obs, st);
    if (rc != DDDMR_OK) return rc;
  }
  if ((rc = finish_on_device(ctx, m, k, timed, out)) != DDDMR_OK) return rc;
  ++m->updates_general;
  return DDDMR_OK;
}

// A fused update that flagged `fallback`: a cluster beyond one partition workgroup, or voxel ranges beyond the 28-bit
// sort keys (points hundreds of metres apart: only a cloud handed over with set_cloud can do that).  The clear phase
// stands, nothing of the mark phase has reached the store but keys and claims, and the mark phase is redone on the
// general route.  out: the fused update's counters, replaced by the finished update's.
int fused_fallback(dddmr_rollout_ctx* ctx, MarkingState* m, const UpdateFrame& f, const float4* obs, uint32_t n_obs, bool timed,
                   MarkCounters& out) {
  hipStream_t st = m->cur;
  --m->updates_fused;
  m->counters_clean = false;
  HIPCHK(ctx, hipMemsetAsync(m->store.s.owner, 0, (size_t)m->store.table * sizeof(unsigned long long), st));
  MarkCounters zero{};
  zero.pool_used = out.pool_used;
  HIPCHK(ctx, hipMemcpyAsync(m->store.counters, &zero, sizeof(zero), hipMemcpyHostToDevice, st));
  int rc = mark_general(ctx, m, f, obs, n_obs, st);
  if (rc != DDDMR_OK) return rc;
  MarkCounters g{};
  if ((rc = finish_on_device(ctx, m, f.k, timed, g)) != DDDMR_OK) return rc;
  g.n_in_window = out.n_in_window; g.n_cleared = out.n_cleared; g.n_removed = out.n_removed; g.n_rehashed = out.n_rehashed;
  g.n_new_keys += out.n_new_keys;
  g.fallback = 1u;
  out = g;
  m->alive_list_stale = false;
  ++m->updates_general;
  return DDDMR_OK;
}

// one update on the fused route: five launches (a sixth with DDDMR_MKF_GRID=global), no copies (marking_fused.hip.h);
// what each launch gets is planned by plan_fused_update (marking_plan.hip.h)
int update_fused(dddmr_rollout_ctx* ctx, MarkingState* m, const UpdateFrame& f, const float4* obs, uint32_t n_obs, bool timed,
                 MarkCounters& out) {
  hipStream_t st = m->cur;
  const MarkParams& k = f.k;
  MarkStore& s = m->store.s;
  if (!m->counters_clean) {
    MarkCounters zero{};
    zero.pool_used = m->store.pool_used;
    HIPCHK(ctx, hipMemcpyAsync(m->store.counters, &zero, sizeof(zero), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(m->ticket, 0, 34 * sizeof(uint32_t), st));
  }
  m->counters_clean = false;                 // (until this update's last block has run)
  if (timed) HIPCHK(ctx, hipEventRecord(m->e0, st));
  int rc = marking_maintenance(ctx, m, st);
  if (rc != DDDMR_OK) return rc;
  const int cur = m->prev >= 0 ? 1 - m->prev : 0;
  GridBuf& gb = m->obs[cur];
  const PointGrid empty_grid = m->obs[0].g;
  const PointGrid prev_grid = m->prev >= 0 ? m->obs[m->prev].g : empty_grid;
  const PointGrid& ground = m->grids.ground.g;
  const uint32_t n_alive = m->store.n_alive;
  const FusedPlan p = plan_fused_update(m->knobs, m->cfg, f, ground, m->grids.ground.max_row, m->grids.n_ground, gb.cap_cells, n_obs,
                                        n_alive, m->store.table);
  if (p.mark) {                              // the planned geometry over this grid's storage
    PointGrid g = p.obs;
    g.cell_start = gb.g.cell_start;
    g.sorted = gb.g.sorted;
    gb.g = g;
  }
  FuseBufs fb{obs, m->sc.parent, m->sc.ds, m->gen, m->store.clear_list, m->unmark_pts,
              BandList{m->band_pts, m->band_cnt}, BandList{m->band_pts + (size_t)kBandMax * kBandCap, m->band_cnt + kBandMax}, p.rg,
              m->ticket, m->cell_count, m->sc.keys_a, m->host_out_dev, m->knobs.grid_in_lds ? 1u : 0u, m->hi_rank};
  if (m->seq == 3 && std::getenv("DDDMR_DEBUG_GRID"))
    std::fprintf(stderr, "[dddmr] marking update: %u points, %u alive; window rows %u x %u segments, %u bands, delta %d -> %u blocks per row segment\n",
                 n_obs, n_alive, p.rg.rows, p.rg.segs, p.rg.bands, p.rg.delta, p.n_part);
  if (p.count_blocks) MK_LAUNCH(m, k_mkf_count, dim3(p.count_blocks), dim3(256), 0, st, gb.g, fb);
  if (p.big) MK_LAUNCH(m, k_mkf_grid_fov<true>, dim3(p.grid_launch()), dim3(1024), 0, st, k, s, gb.g, fb, m->store.counters, p.nb_grid);
  else MK_LAUNCH(m, k_mkf_grid_fov<false>, dim3(p.grid_launch()), dim3(1024), 0, st, k, s, gb.g, fb, m->store.counters, p.nb_grid);
  if (p.clear_launch())
    MK_LAUNCH(m, k_mkf_clear_cc, dim3(p.clear_launch()), dim3(256), 0, st, k, s, prev_grid, gb.g, ground, fb, m->store.counters, p.nb_clear);
  if (timed) HIPCHK(ctx, hipEventRecord(m->e1, st));
  if (p.seed_launch())
    MK_LAUNCH(m, k_mkf_roots_unmark, dim3(p.seed_launch()), dim3(256), 0, st, k, fb, m->sc.cl, s, ground, m->store.counters, p.nb_roots, p.nb_un,
              p.seg_groups, p.n_part_un);
  if (p.part_launch())
    MK_LAUNCH(m, k_mkf_groups, dim3(p.part_launch()), dim3(kPartThreads), kPartLdsBytes, st, k, fb, m->sc.cl, s, ground, m->grids.map.g, m->grids.n_map,
              m->store.counters, p.nb_band_groups, p.seg_groups, p.n_part_un);
  // (the commit launch's last block publishes the counters to host-mapped memory)
  MK_LAUNCH(m, k_mkf_commit_dgraph, dim3(p.commit_launch()), dim3(256), 0, st, k, fb, m->sc.cl, s, ground, m->store.counters, p.nb_commit, p.nb_b,
            p.seg_groups, p.n_part);
  if (timed) HIPCHK(ctx, hipEventRecord(m->e2, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, hipGetLastError());
  out = *m->host_out;
  m->counters_clean = true;
  m->alive_list_stale = true;
  ++m->updates_fused;
  for (uint32_t v : out.n_cleared_shard) out.n_cleared += v;
  out.n_alive = n_alive - out.n_cleared + out.n_revived;
  out.n_clusters = n_obs;                                                        // extent of the per-cluster records (named by seed index)
  if (p.mark && !out.fallback) {
    m->prev = cur;                                                               // pcl_msg_gbl_ of this selfMark
    m->n_prev = n_obs;
  }
  return out.fallback ? fused_fallback(ctx, m, f, obs, n_obs, timed, out) : DDDMR_OK;
}
}  // namespace

extern "C" {

int dddmr_rollout_marking_update(dddmr_rollout_ctx* ctx, const double T_base_sensor[7], const double T_gbl_base[7],
                                 dddmr_marking_stats* stats) {
  if (!ctx || !T_base_sensor || !T_gbl_base) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MarkingState* m = ctx->marking.get();
  if (!m) return fail(ctx, DDDMR_ERR_STATE, "marking_update before marking_create");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // The observation = the context's published aggregate cloud (global frame), pinned like a tick pins it.
  // While a tick_begin is pending -- the reference runs the perception thread's doClear_then_Mark and the planner's
  // tick side by side -- the update runs on a stream of its own, next to the tick's kernels (the two touch disjoint
  // state), provided it reads the SAME observation the pending tick has pinned: a third pinned buffer would leave a
  // producer none to write into.
  const bool overlapped = ctx->pend.active;
  CloudPin pin(ctx, overlapped ? CloudPin::kOfPendingTick : CloudPin::kFront);
  if (overlapped) {
    if (!pin.is_front())
      return fail(ctx, DDDMR_ERR_STATE, "marking_update while a tick_begin is pending: a newer observation was published after tick_begin");
    if (!m->own_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking));
    m->cur = m->own_stream;
    HIPCHK(ctx, pin.wait_on(m->cur));      // (the tick's stream has its own wait enqueued)
    ++m->updates_overlapped;
  } else {
    m->cur = ctx->stream;
    HIPCHK(ctx, pin.wait_on(m->cur));
  }
  return marking_update_on(ctx, m, pin.dev(), pin.n_points(), T_base_sensor, T_gbl_base, stats);
}

}  // extern "C"

namespace {
// One doClear_then_Mark pass of the lidar layer on the observation obs[0 .. n_obs) (device, global frame), on m->cur.
// tick_mu held; the caller keeps `obs` from being recycled until this returns (the update waits for its stream).
int marking_update_on(dddmr_rollout_ctx* ctx, MarkingState* m, const float4* obs, uint32_t n_obs, const double T_base_sensor[7],
                      const double T_gbl_base[7], dddmr_marking_stats* stats) {
  if (n_obs > m->max_obs) return fail(ctx, DDDMR_ERR_CAPACITY, "marking_update: observation of %u points, layer sized for %u", n_obs, m->max_obs);
  float pad = 1e-4f;                           // half an ulp of extent + r_box below 2048 m: upload_static holds the clouds to kSmallPadMaxExtent
  if (const char* e = std::getenv("DDDMR_MK_PAD")) pad = (float)std::atof(e);      // (diagnosis)
  if (++m->seq == 0) m->seq = 1;
  const UpdateFrame f = make_update_frame(m->cfg, T_base_sensor, T_gbl_base, n_obs, m->prev >= 0 ? m->n_prev : 0, m->store.table,
                                          m->store.pool_cap, m->grids.n_ground, m->store.n_alive, m->seq, pad);
  const MarkParams& k = f.k;

  // HIP events serialise the queue around them: the update is timed like the tick (DDDMR_TIMING / _EVERY)
  const bool timed = stats && ctx->timing >= 1 && (m->seq % (uint32_t)ctx->timing_every) == 0;
  MarkCounters out{};
  m->launches_last = 0;
  const bool fused = m->route != 0 && n_obs <= kFuseMaxObs;
  if (m->route == 1 && !fused)
    return fail(ctx, DDDMR_ERR_CAPACITY, "marking_update: DDDMR_MARKING_ROUTE=fused, observation of %u points > %u", n_obs, kFuseMaxObs);
  // An error return below may leave work enqueued on m->cur that reads `obs` and the layer's buffers: wait for it, so
  // that the caller may release the observation and the next call finds the stream idle (the status of that wait does
  // not matter: the error being returned is the one to report).  The returns past the update's own wait are disarmed.
  Drain drain{m->cur};
  const int rc = fused ? update_fused(ctx, m, f, obs, n_obs, timed, out) : update_general(ctx, m, f, obs, n_obs, timed, out);
  if (rc != DDDMR_OK) return rc;
  m->store.pool_used = out.pool_used;
  m->store.n_alive = out.n_alive;
  m->store.keys_used += out.n_new_keys;
  if (out.n_dup > 0 && !out.overflow) {
    const int rt = marking_fix_ties(ctx, m, k, out);
    if (rt != DDDMR_OK) return rt;
  }
  drain.armed = false;                       // (the update and the tie fixes have waited for the stream)
  if (timed) {
    HIPCHK(ctx, hipEventElapsedTime(&m->last_clear_ms, m->e0, m->e1));
    HIPCHK(ctx, hipEventElapsedTime(&m->last_mark_ms, m->e1, m->e2));
  }
  if (stats) {
    stats->n_observation = n_obs > 5 ? n_obs : 0;
    stats->n_clusters = out.n_clusters_kept;
    stats->n_marked = out.n_marked;
    stats->n_in_window = out.n_in_window;
    stats->n_cleared = out.n_cleared;
    stats->n_alive = out.n_alive;
    stats->clear_ms = m->last_clear_ms;       // the latest timed update's
    stats->mark_ms = m->last_mark_ms;
  }
  if (out.overflow)
    return fail(ctx, DDDMR_ERR_CAPACITY, "marking_update: capacity flag %u (1: max_markings, 2: max_cluster_points, 4: a cluster more than 3.2 km (51 m in z) from the window)", out.overflow);
  return DDDMR_OK;
}
}  // namespace

extern "C" {

int dddmr_rollout_marking_route_counts(dddmr_rollout_ctx* ctx, uint32_t* updates_fused, uint32_t* updates_general,
                                       uint32_t* launches_last_update) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MarkingState* m = ctx->marking.get();
  if (!m) return fail(ctx, DDDMR_ERR_STATE, "marking_route_counts before marking_create");
  if (updates_fused) *updates_fused = m->updates_fused;
  if (updates_general) *updates_general = m->updates_general;
  if (launches_last_update) *launches_last_update = m->launches_last;
  return DDDMR_OK;
}

#ifdef DDDMR_PHASE_STAMPS
// diagnostic build only: phase stamps of the last fused update's two single-workgroup blocks
int dddmr_rollout_diag_mkstamps(unsigned long long* out, size_t n_words) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(dddmr::g_mk_stamps), n_words * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
int dddmr_rollout_diag_mkclear(unsigned long long* out) {
#ifdef DDDMR_CLEAR_CYCLES
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(dddmr::g_mk_clear_cyc), 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
#else
  for (int i = 0; i < 8; ++i) out[i] = 0;
  return 0;
#endif
}
#endif

int dddmr_rollout_marking_get_voxels(dddmr_rollout_ctx* ctx, int32_t* xyz_out, size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MarkingState* m = ctx->marking.get();
  if (!m) return fail(ctx, DDDMR_ERR_STATE, "marking_get_voxels before marking_create");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return store_read_voxels(ctx, m->store, "marking_get_voxels", xyz_out, capacity, n);
}

// The generator points of every alive marking (the cluster projected on the robot's ground plane, 0.1 m VoxelGrid): what
// Marking::computeMinDistanceFromObstacle2GroundNodes searches the ground with (cluster_marking.cpp:54-64).  Debug /
// visualisation (the reference publishes its markings as a cloud); order: by store slot.
int dddmr_rollout_marking_get_points(dddmr_rollout_ctx* ctx, float* xyz_out, int32_t* voxel_out, size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MarkingState* m = ctx->marking.get();
  if (!m) return fail(ctx, DDDMR_ERR_STATE, "marking_get_points before marking_create");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<StoreSlot> slots;
  int rc = store_read_slots(ctx, m->store, false, slots);
  if (rc != DDDMR_OK) return rc;
  size_t total = 0;
  for (const StoreSlot& sl : slots) total += sl.n;
  *n = total;
  if (!xyz_out) return DDDMR_OK;
  if (total > capacity) return fail(ctx, DDDMR_ERR_CAPACITY, "marking_get_points: capacity %zu < %zu", capacity, total);
  std::vector<float4> pool;
  if ((rc = store_read_pool(ctx, m->store, pool)) != DDDMR_OK) return rc;
  size_t at = 0;
  for (const StoreSlot& sl : slots) {
    if ((size_t)sl.ofs + sl.n > pool.size()) return fail(ctx, DDDMR_ERR_STATE, "marking_get_points: slot %zu points past the pool", sl.slot);
    for (uint32_t j = 0; j < sl.n; ++j, ++at) {
      const float4 p = pool[(size_t)sl.ofs + j];
      xyz_out[3 * at] = p.x; xyz_out[3 * at + 1] = p.y; xyz_out[3 * at + 2] = p.z;
      if (voxel_out) voxel_unkey(sl.key, &voxel_out[3 * at], &voxel_out[3 * at + 1], &voxel_out[3 * at + 2]);
    }
  }
  return DDDMR_OK;
}

int dddmr_rollout_marking_get_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity) {
  if (!ctx || !values_out) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MarkingState* m = ctx->marking.get();
  if (!m) return fail(ctx, DDDMR_ERR_STATE, "marking_get_dgraph before marking_create");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return store_read_dgraph(ctx, m->store, "marking_get_dgraph", values_out, capacity);
}

int dddmr_rollout_marking_get_lethal(dddmr_rollout_ctx* ctx, uint8_t* flags_out, size_t capacity) {
  if (!ctx || !flags_out) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MarkingState* m = ctx->marking.get();
  if (!m) return fail(ctx, DDDMR_ERR_STATE, "marking_get_lethal before marking_create");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return store_read_lethal(ctx, m->store, "marking_get_lethal", flags_out, capacity);
}

}  // extern "C"
