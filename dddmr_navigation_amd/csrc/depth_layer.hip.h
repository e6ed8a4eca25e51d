// depth_layer.hip.h -- the global-mode DepthCameraLayer on the device: marking store, dGraph and lethal set.
//
// One dddmr_rollout_depth_layer_update is one selfClear + selfMark + updateLethalPointCloud pass
// (stacked_perception.cpp:82-88; dddmr_perception_3d/plugins/depth_camera/depth_camera_layer.cpp:252-426, :487-601;
// plugins/cluster_marking.cpp:49-138; src/graph/dynamic_graph.cpp:38-61) with pct_marking_, its dGraph and lethal_map_
// persistent in HBM.  include/dddmr_rollout.h restates the semantics; this file is the glue between three slices that
// are parity-tested on their own:
//   the verdict of a stored marking      dc_marking_verdict (depth_clear.hip.h), here fed from the device store
//   the clusters addPCPtr is called with depth_mark_enqueue (depth_mark.hip.h)
//   store, pool, dGraph, housekeeping    the lidar layer's general route (marking.hip.h): k_mk_unmark, k_mk_proj_keys,
//                                        k_mk_flags, k_mk_group_reduce, k_mk_slots, k_mk_dgraph, k_mk_finish,
//                                        k_mk_fill_dgraph unchanged
//
// The store is the lidar layer's MarkStore plus, per slot, the stored cluster pc_ (the 0.2 m cloud selfClear's engagement
// test searches with).  A marking's pc_ and its generator points lie behind one another in the pool:
//   pool[pc_ofs .. pc_ofs + pc_n)          pc_
//   pool[pts_ofs .. pts_ofs + pts_n)       generator points, pts_ofs = pc_ofs + pc_n
// so the kernels that only read generator points (k_mk_unmark, k_mk_dgraph) fit as they are, and the ones that move a
// slot (rehash, compaction, the contested-voxel fix) have k_dl_ siblings that carry pc_ along.
//
// Launch sequence of an update, all on the feeds' stream:
//   [observation grid, when a depth source has published: depth_observation_grid]
//   k_dl_begin                                  counters of the update (the pool fill stays on the device)
//   [k_dl_rehash] [k_dl_compact_sizes, scan, k_dl_compact_move]      housekeeping, rare
//   k_dl_window, k_dl_verdicts, k_mk_unmark     selfClear: one lane per alive marking, one wave per marking in the window
//                                               (lanes striding its pc_), one wave per removed marking
//   depth_mark_enqueue                          selfMark up to the clusters' fates (skipped with <= 5 observation points)
//   k_dl_accept, k_mk_proj_keys, sort, k_mk_flags, scan, k_mk_group_reduce      generator points
//   k_mk_slots, k_dl_commit, k_dl_store_pc, k_mk_dgraph                         addPCPtr: one wave per generator point
//   k_mk_finish, k_dl_out                       next update's alive list; counters into pinned, mapped memory
// One host wait.  k_dl_out also hands over the clusters' sizes, states and slots when (and only when) a voxel was
// contested; the host then replays the reference's sort (dm_replay_sort) and k_dl_fix_owner re-commits the voxels whose
// keeper differs: the second wait of such an update.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <unordered_map>

#include "depth_mark.hip.h"

#pragma clang fp contract(off)

namespace dddmr {

struct DlStore {              // what the depth store keeps beside MarkStore's arrays (device pointers)
  uint32_t* pc_ofs;           // [table] first point of the stored pc_ in the pool
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

// Appends one entry per lane with `pred` to a list: one atomic per wave.  Every lane of the wave must call it.
__device__ __forceinline__ uint32_t dl_wave_append(uint32_t* counter, bool pred, int lane) {
  const unsigned long long m = __ballot(pred);
  uint32_t base = 0;
  if (m) {
    const int leader = __ffsll((long long)m) - 1;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, leader, 64);
  }
  return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

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
  const uint32_t at = dl_wave_append(&cnt->n_in_window, in, threadIdx.x & 63);
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

// Marking::addPCPtr, storage part: the cluster that owns its voxel gets pool space for its pc_ and its generator points
// (the ranges the slot had before become pool garbage: :106-111 reset the pointers without a clearValue)
__global__ __launch_bounds__(64) void k_dl_commit(MarkParams k, const MarkCounters* __restrict__ cnt_in, ClusterArrays c, MarkStore s, DlStore d,
                                                  MarkCounters* __restrict__ cnt, uint32_t* __restrict__ pc_dst, uint32_t* __restrict__ gen_dst) {
  const uint32_t ci = blockIdx.x * 64 + threadIdx.x;
  if (ci >= cnt_in->n_clusters) return;
  pc_dst[ci] = 0xFFFFFFFFu;
  gen_dst[ci] = 0xFFFFFFFFu;
  if (c.state[ci] != 2u) return;
  const uint32_t slot = c.slot[ci];
  const unsigned long long pr = ((unsigned long long)((1u << 20) - min(c.size[ci], (1u << 20) - 1u)) << 20) | (unsigned long long)(ci + 1u);
  if (s.owner[slot] != pr) return;
  const uint32_t npc = c.ds_count[ci], ng = c.gen_count[ci];
  const uint32_t ofs = atomicAdd(&cnt->pool_used, npc + ng);
  if ((unsigned long long)ofs + npc + ng > (unsigned long long)k.pool_cap) {
    atomicOr(&cnt->overflow, 2u);
    s.alive[slot] = 0; s.pts_n[slot] = 0; d.pc_n[slot] = 0;
    return;
  }
  pc_dst[ci] = ofs;
  gen_dst[ci] = ofs + npc;
  d.pc_ofs[slot] = ofs;
  d.pc_n[slot] = npc;
  s.pts_ofs[slot] = ofs + npc;
  s.pts_n[slot] = ng;
  s.alive[slot] = 1;
}
// ... the 0.2 m points of the owners into the pool, one lane per point (the generator points go with k_mk_dgraph)
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

// k_mk_fix_owner with pc_: the cluster that keeps a contested voxel in the reference's order replaces what k_dl_commit
// stored.  One wave per (slot, cluster) pair; `fix` is host-mapped.
__global__ __launch_bounds__(256) void k_dl_fix_owner(MarkParams k, uint32_t n_fix, const uint2* __restrict__ fix, const float4* __restrict__ ds,
                                                      const uint32_t* __restrict__ ds_first, const float4* __restrict__ gen, ClusterArrays c,
                                                      MarkStore s, DlStore d, MarkCounters* __restrict__ cnt) {
  const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (f >= n_fix) return;
  const uint32_t slot = fix[f].x, ci = fix[f].y;
  const uint32_t npc = c.ds_count[ci], ng = c.gen_count[ci], pc_first = ds_first[ci], gen_first = c.gen_first[ci];
  uint32_t ofs = 0;
  if (lane == 0) ofs = atomicAdd(&cnt->pool_used, npc + ng);
  ofs = (uint32_t)__builtin_amdgcn_readfirstlane((int)ofs);
  if ((unsigned long long)ofs + npc + ng > (unsigned long long)k.pool_cap) {
    if (lane == 0) { atomicOr(&cnt->overflow, 2u); s.alive[slot] = 0; s.pts_n[slot] = 0; d.pc_n[slot] = 0; }
    return;
  }
  for (uint32_t i = lane; i < npc; i += 64) {
    const float4 p = ds[pc_first + i];
    s.pool[ofs + i] = make_float4(p.x, p.y, p.z, 0.f);
  }
  for (uint32_t i = lane; i < ng; i += 64) {
    const float4 p = gen[gen_first + i];
    s.pool[ofs + npc + i] = make_float4(p.x, p.y, p.z, 0.f);
  }
  if (lane == 0) {
    d.pc_ofs[slot] = ofs; d.pc_n[slot] = npc;
    s.pts_ofs[slot] = ofs + npc; s.pts_n[slot] = ng;
    s.alive[slot] = 1;
  }
}

// k_mk_rehash with pc_ (store garbage collection: the alive markings move to a fresh table)
__global__ __launch_bounds__(256) void k_dl_rehash(uint32_t table_mask, MarkStore s, DlStore d, unsigned long long* __restrict__ keys_new,
                                                   uint32_t* __restrict__ alive_new, uint32_t* __restrict__ pts_ofs_new,
                                                   uint32_t* __restrict__ pts_n_new, uint32_t* __restrict__ pc_ofs_new,
                                                   uint32_t* __restrict__ pc_n_new, MarkCounters* __restrict__ cnt) {
  const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
  if (slot > table_mask || !s.alive[slot]) return;
  const unsigned long long key = s.keys[slot];
  uint32_t ns = voxel_hash(key) & table_mask;
  for (uint32_t probe = 0; probe <= table_mask; ++probe) {          // (alive markings are fewer than slots: always ends)
    if (atomicCAS(&keys_new[ns], 0ull, key) == 0ull) break;
    ns = (ns + 1) & table_mask;
  }
  alive_new[ns] = 1;
  pts_ofs_new[ns] = s.pts_ofs[slot];
  pts_n_new[ns] = s.pts_n[slot];
  pc_ofs_new[ns] = d.pc_ofs[slot];
  pc_n_new[ns] = d.pc_n[slot];
  s.alive_list[atomicAdd(&cnt->n_rehashed, 1u)] = ns;
}
// k_mk_compact_* with pc_ (pool compaction: an alive marking's pc_ + generator points move as one range)
__global__ __launch_bounds__(256) void k_dl_compact_sizes(uint32_t table, MarkStore s, DlStore d, uint32_t* __restrict__ sizes) {
  const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
  if (slot < table) sizes[slot] = s.alive[slot] ? d.pc_n[slot] + s.pts_n[slot] : 0u;
}
__global__ __launch_bounds__(256) void k_dl_compact_move(uint32_t table, MarkStore s, DlStore d, const uint32_t* __restrict__ new_ofs,
                                                         float4* __restrict__ dst, MarkCounters* __restrict__ cnt) {
  const uint32_t slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (slot >= table || !s.alive[slot]) return;
  const uint32_t npc = d.pc_n[slot], n = npc + s.pts_n[slot], from = d.pc_ofs[slot], to = new_ofs[slot];
  for (uint32_t i = lane; i < n; i += 64) dst[to + i] = s.pool[from + i];
  if (lane == 0) {
    d.pc_ofs[slot] = to;
    s.pts_ofs[slot] = to + npc;
    atomicMax(&cnt->pool_used, to + n);
  }
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
  uint32_t n_ground = 0, table = 0, pool_cap = 0, max_obs = 0;
  DepthMarkState* dm = nullptr;            // the cluster pipeline's scratch and the ground / map grids
  MarkStore store{};
  DlStore ds{};
  float4* pool_alt = nullptr;
  unsigned long long* keys_alt = nullptr;
  uint32_t *alive_alt = nullptr, *pts_ofs_alt = nullptr, *pts_n_alt = nullptr, *pc_ofs_alt = nullptr, *pc_n_alt = nullptr;
  uint32_t *compact_sizes = nullptr, *compact_ofs = nullptr;
  // scratch of one update beside dm's (sized for max_obs)
  float4 *proj = nullptr, *gen = nullptr;
  uint32_t *gen_first = nullptr, *gen_count = nullptr, *slot = nullptr, *pc_dst = nullptr, *gen_dst = nullptr;
  uint32_t* n_gen = nullptr;
  MarkCounters* counters = nullptr;        // device; pool_used persists between updates
  DlCounters* extra = nullptr;
  void* temp = nullptr;                    // rocPRIM scratch of the compaction's scan over the table
  size_t temp_bytes = 0;
  void* out_host = nullptr;                // DlOut, tie arrays [3 * max_obs], fix list [max_obs / 2] uint2
  void* out_dev = nullptr;
  uint32_t pool_used_host = 0, n_alive_host = 0, keys_used_host = 0, seq = 0;
};

void depth_layer_free(DepthLayerState* s) {
  if (!s) return;
  void* p[] = {s->store.keys, s->store.alive, s->store.pts_ofs, s->store.pts_n, s->store.removed_seq, s->store.owner, s->store.alive_list,
               s->store.removed_list, s->store.pool, s->store.dgraph, s->store.lethal, s->ds.pc_ofs, s->ds.pc_n, s->ds.clear_list,
               s->pool_alt, s->keys_alt, s->alive_alt, s->pts_ofs_alt, s->pts_n_alt, s->pc_ofs_alt, s->pc_n_alt, s->compact_sizes,
               s->compact_ofs, s->proj, s->gen, s->gen_first, s->gen_count, s->slot, s->pc_dst, s->gen_dst, s->n_gen, s->counters,
               s->extra, s->temp};
  for (void* q : p)
    if (q) (void)hipFree(q);
  if (s->out_host) (void)hipHostFree(s->out_host);
  depth_mark_free(s->dm);
  delete s;
}

// resetdGraph: empty store, dGraph = max_obstacle_distance on keys 0 .. n_ground.  producer_mu held.
int depth_layer_reset_locked(dddmr_rollout_ctx* ctx, DepthLayerState* s) {
  hipStream_t st = ctx->copy_stream;
  MarkStore& m = s->store;
  const size_t t = s->table;
  HIPCHK(ctx, hipMemsetAsync(m.keys, 0, t * sizeof(unsigned long long), st));
  HIPCHK(ctx, hipMemsetAsync(m.alive, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(m.pts_ofs, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(m.pts_n, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(m.removed_seq, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(m.owner, 0, t * sizeof(unsigned long long), st));
  HIPCHK(ctx, hipMemsetAsync(s->ds.pc_ofs, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(s->ds.pc_n, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(m.lethal, 0, (size_t)s->n_ground + 1, st));
  HIPCHK(ctx, hipMemsetAsync(s->counters, 0, sizeof(MarkCounters), st));
  hipLaunchKernelGGL(k_mk_fill_dgraph, dim3((s->n_ground + 1 + 255) / 256), dim3(256), 0, st, s->n_ground + 1, m.dgraph,
                     s->cfg.max_obstacle_distance);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));
  s->pool_used_host = 0;
  s->n_alive_host = 0;
  s->keys_used_host = 0;
  return DDDMR_OK;
}

int depth_layer_init(dddmr_rollout_ctx* ctx, DepthLayerState* s, const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                     const float* map_xyz, size_t n_map, size_t map_stride_bytes) {
  s->dm = new DepthMarkState();
  s->dm->cfg.xy_resolution = s->cfg.xy_resolution;
  s->dm->cfg.height_resolution = s->cfg.height_resolution;
  s->dm->cfg.euclidean_cluster_extraction_tolerance = s->cfg.euclidean_cluster_extraction_tolerance;
  s->dm->cfg.euclidean_cluster_extraction_min_cluster_size = s->cfg.euclidean_cluster_extraction_min_cluster_size;
  s->dm->cfg.segmentation_ignore_ratio = s->cfg.segmentation_ignore_ratio;
  s->dm->cfg.max_observation_points = s->cfg.max_observation_points;
  s->dm->n_ground = (uint32_t)n_ground;
  s->dm->n_map = (uint32_t)n_map;
  s->dm->max_obs = s->max_obs;
  int rc = depth_mark_init(ctx, s->dm, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes);
  if (rc != DDDMR_OK) return rc;
  const size_t N = s->max_obs, t = s->table;
  MarkStore& m = s->store;
  HIPCHK(ctx, hipMalloc(&m.keys, t * sizeof(unsigned long long)));
  HIPCHK(ctx, hipMalloc(&m.alive, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&m.pts_ofs, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&m.pts_n, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&m.removed_seq, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&m.owner, t * sizeof(unsigned long long)));
  HIPCHK(ctx, hipMalloc(&m.alive_list, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&m.removed_list, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&m.pool, (size_t)s->pool_cap * sizeof(float4)));
  HIPCHK(ctx, hipMalloc(&m.dgraph, (n_ground + 1) * sizeof(double)));
  HIPCHK(ctx, hipMalloc(&m.lethal, n_ground + 1));
  HIPCHK(ctx, hipMalloc(&s->ds.pc_ofs, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->ds.pc_n, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->ds.clear_list, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->pool_alt, (size_t)s->pool_cap * sizeof(float4)));
  HIPCHK(ctx, hipMalloc(&s->keys_alt, t * sizeof(unsigned long long)));
  HIPCHK(ctx, hipMalloc(&s->alive_alt, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->pts_ofs_alt, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->pts_n_alt, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->pc_ofs_alt, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->pc_n_alt, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->compact_sizes, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->compact_ofs, t * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->proj, N * sizeof(float4)));
  HIPCHK(ctx, hipMalloc(&s->gen, N * sizeof(float4)));
  HIPCHK(ctx, hipMalloc(&s->gen_first, N * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->gen_count, N * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->slot, N * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->pc_dst, N * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->gen_dst, N * sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->n_gen, sizeof(uint32_t)));
  HIPCHK(ctx, hipMalloc(&s->counters, sizeof(MarkCounters)));
  HIPCHK(ctx, hipMalloc(&s->extra, sizeof(DlCounters)));
  HIPCHK(ctx, rocprim::exclusive_scan(nullptr, s->temp_bytes, s->compact_sizes, s->compact_ofs, 0u, t, rocprim::plus<uint32_t>(), ctx->copy_stream));
  s->temp_bytes += 256;
  HIPCHK(ctx, hipMalloc(&s->temp, s->temp_bytes));
  const size_t bytes = sizeof(DlOut) + 3 * N * sizeof(uint32_t) + (N / 2 + 1) * sizeof(uint2);
  if (host_mapped_alloc(&s->out_host, &s->out_dev, bytes) != 0) return fail(ctx, DDDMR_ERR_HIP, "depth_layer_create: staging of %zu bytes", bytes);
  return depth_layer_reset_locked(ctx, s);
}

#define DL_LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); ++ops; } while (0)

// Store garbage collection when half the table holds keys and a good part of them is dead; pool compaction when half the
// pool is used or garbage: the lidar layer's rules (store_maintenance of marking_host.hip.h).  -> runs made, < 0 on error
int depth_layer_maintenance(dddmr_rollout_ctx* ctx, DepthLayerState* s, hipStream_t st, uint32_t& ops) {
  MarkStore& m = s->store;
  const size_t t = s->table;
  int runs = 0;
  if (s->keys_used_host > s->table / 2 && s->keys_used_host > s->n_alive_host + s->table / 8) {
    if (hipMemsetAsync(s->keys_alt, 0, t * sizeof(unsigned long long), st) != hipSuccess ||
        hipMemsetAsync(s->alive_alt, 0, t * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(s->pts_ofs_alt, 0, t * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(s->pts_n_alt, 0, t * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(s->pc_ofs_alt, 0, t * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(s->pc_n_alt, 0, t * sizeof(uint32_t), st) != hipSuccess)
      return -1;
    DL_LAUNCH(k_dl_rehash, dim3((s->table + 255) / 256), dim3(256), 0, st, s->table - 1, m, s->ds, s->keys_alt, s->alive_alt, s->pts_ofs_alt,
              s->pts_n_alt, s->pc_ofs_alt, s->pc_n_alt, s->counters);
    ops += 6;
    std::swap(m.keys, s->keys_alt);
    std::swap(m.alive, s->alive_alt);
    std::swap(m.pts_ofs, s->pts_ofs_alt);
    std::swap(m.pts_n, s->pts_n_alt);
    std::swap(s->ds.pc_ofs, s->pc_ofs_alt);
    std::swap(s->ds.pc_n, s->pc_n_alt);
    s->keys_used_host = s->n_alive_host;
    ++runs;
  }
  if (s->pool_used_host > s->pool_cap / 2) {
    DL_LAUNCH(k_dl_compact_sizes, dim3((s->table + 255) / 256), dim3(256), 0, st, s->table, m, s->ds, s->compact_sizes);
    size_t tb = s->temp_bytes;
    if (rocprim::exclusive_scan(s->temp, tb, s->compact_sizes, s->compact_ofs, 0u, t, rocprim::plus<uint32_t>(), st) != hipSuccess) return -1;
    if (hipMemsetAsync(&s->counters->pool_used, 0, sizeof(uint32_t), st) != hipSuccess) return -1;
    DL_LAUNCH(k_dl_compact_move, dim3((s->table + 3) / 4), dim3(256), 0, st, s->table, m, s->ds, s->compact_ofs, s->pool_alt, s->counters);
    ops += 4;
    std::swap(m.pool, s->pool_alt);
    ++runs;
  }
  return runs;
}

// Contested voxels: marking_fix_ties of the lidar layer for the depth store.  `tie` holds every cluster's size, state and
// slot; the voxels whose keeper in the reference's processing order differs from the device's priority are re-committed.
// -> pairs written to `fix`
uint32_t depth_layer_ties(const DepthLayerState* s, uint32_t nc, const uint32_t* tie, uint2* fix) {
  const uint32_t N = s->max_obs;
  const uint32_t *size = tie, *state = tie + N, *slot = tie + 2 * (size_t)N;
  std::vector<DmItem> order;
  order.reserve(nc);
  for (uint32_t ci = 0; ci < nc; ++ci)
    if ((int)size[ci] >= s->cfg.euclidean_cluster_extraction_min_cluster_size) order.push_back(DmItem{size[ci], ci});
  dm_replay_sort(order);
  struct Keep { uint32_t ref_ci, dev_ci, dev_size, claims; };
  std::unordered_map<uint32_t, Keep> keep;
  for (const DmItem& it : order) {                      // (processing order)
    if (state[it.ci] != 2u) continue;
    auto ins = keep.insert(std::make_pair(slot[it.ci], Keep{it.ci, it.ci, it.size, 1u}));
    if (ins.second) continue;
    Keep& kp = ins.first->second;
    kp.ref_ci = it.ci;
    ++kp.claims;
    if (it.size < kp.dev_size || (it.size == kp.dev_size && it.ci > kp.dev_ci)) { kp.dev_ci = it.ci; kp.dev_size = it.size; }   // k_mk_slots' priority
  }
  uint32_t n = 0;
  for (const auto& kv : keep)
    if (kv.second.claims > 1 && kv.second.ref_ci != kv.second.dev_ci && n < N / 2) fix[n++] = make_uint2(kv.first, kv.second.ref_ci);
  return n;
}

DepthLayerState* depth_layer_of(dddmr_rollout_ctx* ctx, const char* what) {
  if (!ctx->dlayer) (void)fail(ctx, DDDMR_ERR_STATE, "%s before depth_layer_create", what);
  return ctx->dlayer;
}

}  // namespace

extern "C" {

int dddmr_rollout_depth_layer_create(dddmr_rollout_ctx* ctx, const dddmr_depth_layer_config* cfg, const float* ground_xyz,
                                     size_t n_ground, size_t ground_stride_bytes, const float* map_xyz, size_t n_map,
                                     size_t map_stride_bytes) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  if ((n_ground && (!ground_xyz || ground_stride_bytes < 12 || ground_stride_bytes % 4)) ||
      (n_map && (!map_xyz || map_stride_bytes < 12 || map_stride_bytes % 4)))
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
  auto* s = new DepthLayerState();
  s->cfg = *cfg;
  s->n_ground = (uint32_t)n_ground;
  s->max_obs = cfg->max_observation_points;
  s->pool_cap = cfg->max_cluster_points;
  uint32_t table = 8;
  while (table < 2 * cfg->max_markings) table <<= 1;
  s->table = table;
  const int rc = depth_layer_init(ctx, s, ground_xyz, n_ground, ground_stride_bytes, map_xyz, n_map, map_stride_bytes);
  if (rc != DDDMR_OK) { depth_layer_free(s); return rc; }
  if (ctx->dlayer) depth_layer_free(ctx->dlayer);
  ctx->dlayer = s;                                       // only a complete state is ever visible
  return DDDMR_OK;
}

int dddmr_rollout_depth_layer_reset(dddmr_rollout_ctx* ctx) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_reset");
  if (!s) return DDDMR_ERR_STATE;
  return depth_layer_reset_locked(ctx, s);
}

int dddmr_rollout_depth_layer_update(dddmr_rollout_ctx* ctx, const double T_gbl_base[7], dddmr_depth_layer_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!T_gbl_base || !stats) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_layer_update: null argument");
  for (int i = 0; i < 7; ++i)
    if (!std::isfinite(T_gbl_base[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_layer_update: non-finite transform");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_update");
  if (!s) return DDDMR_ERR_STATE;
  DcFrustums S;
  int rc = depth_frustums(ctx, "depth_layer_update", &S);
  if (rc != DDDMR_OK) return rc;
  size_t n_obs = 0;
  for (int i = 0; i < dddmr_rollout_ctx::kMaxSources; ++i)
    if (ctx->depth[i]) n_obs += ctx->src_n[i];
  if (n_obs > s->max_obs)
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_update: %zu observation points, max_observation_points %u", n_obs, s->max_obs);
  if ((rc = depth_clear_scratch(ctx, "depth_layer_update")) != DDDMR_OK) return rc;
  DepthClear& d = *ctx->dclear;
  hipStream_t st = ctx->copy_stream;      // the stream the depth feeds ran on: their frames are complete before this work
  uint32_t ops = 0;
  const bool observation_clear = !(n_obs > 5);           // :258-264, :491-492
  if (!observation_clear && (rc = depth_observation_grid(ctx, d, n_obs, st, &ops)) != DDDMR_OK) return rc;
  const uint32_t n = (uint32_t)n_obs;
  const dddmr_depth_layer_config& c = s->cfg;
  DepthMarkState* dm = s->dm;
  MarkStore& m = s->store;

  MarkParams k{};
  k.res = c.xy_resolution; k.hres = c.height_resolution; k.marking_height = c.marking_height; k.window = c.perception_window_size;
  k.inscribed = c.inscribed_radius; k.inflation = c.inflation_radius;
  {
    // coefficients (:568-578): tf2::quatRotate(q, (0, 0, 1)) and d in double, each rounded to float
    const double qb[4] = {T_gbl_base[3], T_gbl_base[4], T_gbl_base[5], T_gbl_base[6]};
    double nb[3];
    quat_rotate_z(qb, nb);
    k.mc[0] = (float)nb[0]; k.mc[1] = (float)nb[1]; k.mc[2] = (float)nb[2];
    const double dd = -T_gbl_base[0] * nb[0] - T_gbl_base[1] * nb[1] - T_gbl_base[2] * nb[2];
    k.mc[3] = (float)dd;
  }
  k.wx0 = (int)((T_gbl_base[0] - c.perception_window_size) / c.xy_resolution);      // :280-287
  k.wx1 = (int)((T_gbl_base[0] + c.perception_window_size) / c.xy_resolution);
  k.wy0 = (int)((T_gbl_base[1] - c.perception_window_size) / c.xy_resolution);
  k.wy1 = (int)((T_gbl_base[1] + c.perception_window_size) / c.xy_resolution);
  k.wz0 = (int)((T_gbl_base[2] - c.marking_height) / c.height_resolution);
  k.wz1 = (int)((T_gbl_base[2] + c.marking_height) / c.height_resolution);
  k.n_obs = n;
  k.pad = kDcPad;
  k.table_mask = s->table - 1;
  k.pool_cap = s->pool_cap;
  k.n_ground = s->n_ground;
  k.seq = ++s->seq;
  if (k.seq == 0) k.seq = s->seq = 1;

  dddmr_depth_layer_stats out{};
  out.n_observation = n;
  DL_LAUNCH(k_dl_begin, dim3(1), dim3(64), 0, st, s->counters, s->extra);
  const int runs = depth_layer_maintenance(ctx, s, st, ops);
  if (runs < 0) return fail(ctx, DDDMR_ERR_HIP, "depth_layer_update: housekeeping failed");
  out.gc_runs = (uint32_t)runs;
  k.n_alive_prev = s->n_alive_host;
  // ---- selfClear against the current observation ----
  if (s->n_alive_host > 0) {
    DL_LAUNCH(k_dl_window, dim3((s->n_alive_host + 255) / 256), dim3(256), 0, st, k, m, s->ds, s->counters);
    DL_LAUNCH(k_dl_verdicts, dim3((s->n_alive_host + 3) / 4), dim3(256), 0, st, k, S, d.hdr, observation_clear ? 1u : 0u, m, s->ds, s->counters);
    DL_LAUNCH(k_mk_unmark, dim3((s->n_alive_host + 3) / 4), dim3(256), 0, st, k, m, dm->ground.g, s->counters);
  }
  // ---- selfMark ----
  ClusterArrays cl = dm->cl;
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
    DL_LAUNCH(k_mk_proj_keys, pb, dim3(256), 0, st, k, dm->n_groups, dm->ds, cl, ox, oy, oz, s->proj, dm->keys_a, dm->vals_a, n, s->counters);
    size_t tb = dm->temp_bytes;
    HIPCHK(ctx, rocprim::radix_sort_pairs(dm->temp, tb, dm->keys_a, dm->keys_b, dm->vals_a, dm->vals_b, (size_t)n, 0, 62, st));
    DL_LAUNCH(k_mk_flags, pb, dim3(256), 0, st, n, dm->keys_b, 0, dm->flags);
    tb = dm->temp_bytes;
    HIPCHK(ctx, rocprim::inclusive_scan(dm->temp, tb, dm->flags, dm->incl, (size_t)n, rocprim::plus<uint32_t>(), st));
    DL_LAUNCH(k_mk_group_reduce, cb, dim3(64), 0, st, n, dm->keys_b, dm->vals_b, dm->flags, dm->incl, 1, dm->keys1, s->proj, s->gen,
              cl.gen_count, cl.gen_first, s->n_gen);
    // addPCPtr
    DL_LAUNCH(k_mk_slots, cb, dim3(64), 0, st, k, dm->counters, cl, m, s->counters);
    DL_LAUNCH(k_dl_commit, cb, dim3(64), 0, st, k, dm->counters, cl, m, s->ds, s->counters, s->pc_dst, s->gen_dst);
    DL_LAUNCH(k_dl_store_pc, pb, dim3(256), 0, st, dm->n_groups, dm->ds, dm->ds_first, s->pc_dst, m.pool);
    DL_LAUNCH(k_mk_dgraph, dim3((n + 3) / 4), dim3(256), 0, st, k, s->n_gen, s->gen, cl, s->gen_dst, m, dm->ground.g);
    ops += 3 * 10 + 3 * 3 + 2;            // rocPRIM, estimated: three sorts (block sort + ~8 merge passes + id wrapper), three scans; two memsets
  }
  DL_LAUNCH(k_mk_finish, dim3((s->table + 255) / 256), dim3(256), 0, st, k, m, s->counters);
  char* dev = static_cast<char*>(s->out_dev);
  char* host = static_cast<char*>(s->out_host);
  const size_t tie_at = sizeof(DlOut), fix_at = tie_at + 3 * (size_t)s->max_obs * sizeof(uint32_t);
  DL_LAUNCH(k_dl_out, dim3(observation_clear ? 1u : (n + 255) / 256), dim3(256), 0, st, observation_clear ? 0u : 1u, s->max_obs, s->counters,
            s->extra, dm->counters, cl, reinterpret_cast<DlOut*>(dev), reinterpret_cast<uint32_t*>(dev + tie_at));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));                 // the update's one host wait
  out.host_waits = 1;
  DlOut o = *reinterpret_cast<const DlOut*>(host);
  if (o.c.n_dup > 0 && !o.c.overflow && !o.mark_overflow) {
    uint2* fix = reinterpret_cast<uint2*>(host + fix_at);
    const uint32_t n_fix = depth_layer_ties(s, o.n_clusters, reinterpret_cast<const uint32_t*>(host + tie_at), fix);
    if (n_fix > 0) {
      DL_LAUNCH(k_dl_fix_owner, dim3((n_fix + 3) / 4), dim3(256), 0, st, k, n_fix, reinterpret_cast<const uint2*>(dev + fix_at), dm->ds,
                dm->ds_first, s->gen, cl, m, s->ds, s->counters);
      DL_LAUNCH(k_dl_out, dim3(1), dim3(256), 0, st, 0u, s->max_obs, s->counters, s->extra, dm->counters, cl, reinterpret_cast<DlOut*>(dev),
                reinterpret_cast<uint32_t*>(dev + tie_at));
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipStreamSynchronize(st));             // the second wait of an update with a contested voxel
      out.host_waits = 2;
      const DlOut o2 = *reinterpret_cast<const DlOut*>(host);
      o.c.pool_used = o2.c.pool_used;
      o.c.overflow |= o2.c.overflow;
    }
  }
  s->pool_used_host = o.c.pool_used;
  s->n_alive_host = o.c.n_alive;
  s->keys_used_host += o.c.n_new_keys;
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

int dddmr_rollout_depth_layer_get_voxels(dddmr_rollout_ctx* ctx, int32_t* xyz_out, size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_get_voxels");
  if (!s) return DDDMR_ERR_STATE;
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  std::vector<unsigned long long> keys(s->table);
  std::vector<uint32_t> alive(s->table);
  HIPCHK(ctx, hipMemcpy(keys.data(), s->store.keys, keys.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(alive.data(), s->store.alive, alive.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  size_t cnt = 0;
  for (size_t i = 0; i < keys.size(); ++i) {
    if (!alive[i] || !keys[i]) continue;
    if (xyz_out) {
      if (cnt >= capacity) return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_get_voxels: capacity %zu too small", capacity);
      voxel_unkey(keys[i], &xyz_out[3 * cnt], &xyz_out[3 * cnt + 1], &xyz_out[3 * cnt + 2]);
    }
    ++cnt;
  }
  *n = cnt;
  return DDDMR_OK;
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
  const size_t t = s->table;
  std::vector<unsigned long long> keys(t);
  std::vector<uint32_t> alive(t), ofs(t), cnt(t);
  HIPCHK(ctx, hipMemcpy(keys.data(), s->store.keys, t * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(alive.data(), s->store.alive, t * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(ofs.data(), s->ds.pc_ofs, t * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(cnt.data(), s->ds.pc_n, t * sizeof(uint32_t), hipMemcpyDeviceToHost));
  size_t nm = 0, np = 0;
  for (size_t i = 0; i < t; ++i)
    if (alive[i] && keys[i]) { ++nm; np += cnt[i]; }
  *n_markings = nm;
  *n_points = np;
  if (n_out == 0) return DDDMR_OK;
  if (nm > cap_markings || np > cap_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_get_clusters: %zu markings / %zu points, capacity %zu / %zu", nm, np, cap_markings, cap_points);
  std::vector<float4> pool(std::min<size_t>(s->pool_used_host, s->pool_cap));
  if (!pool.empty()) HIPCHK(ctx, hipMemcpy(pool.data(), s->store.pool, pool.size() * sizeof(float4), hipMemcpyDeviceToHost));
  size_t mi = 0, at = 0;
  offsets_out[0] = 0;
  for (size_t i = 0; i < t; ++i) {
    if (!alive[i] || !keys[i]) continue;
    voxel_unkey(keys[i], &voxel_out[3 * mi], &voxel_out[3 * mi + 1], &voxel_out[3 * mi + 2]);
    if ((size_t)ofs[i] + cnt[i] > pool.size()) return fail(ctx, DDDMR_ERR_STATE, "depth_layer_get_clusters: slot %zu points past the pool", i);
    for (uint32_t j = 0; j < cnt[i]; ++j, ++at) {
      const float4 p = pool[(size_t)ofs[i] + j];
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
  if (capacity < (size_t)s->n_ground + 1) return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_get_dgraph: capacity %zu < %u", capacity, s->n_ground + 1);
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  HIPCHK(ctx, hipMemcpy(values_out, s->store.dgraph, ((size_t)s->n_ground + 1) * sizeof(double), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

int dddmr_rollout_depth_layer_get_lethal(dddmr_rollout_ctx* ctx, uint8_t* flags_out, size_t capacity) {
  if (!ctx || !flags_out) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DepthLayerState* s = depth_layer_of(ctx, "depth_layer_get_lethal");
  if (!s) return DDDMR_ERR_STATE;
  if (capacity < (size_t)s->n_ground + 1) return fail(ctx, DDDMR_ERR_CAPACITY, "depth_layer_get_lethal: capacity %zu < %u", capacity, s->n_ground + 1);
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  HIPCHK(ctx, hipMemcpy(flags_out, s->store.lethal, (size_t)s->n_ground + 1, hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

}  // extern "C"
