// marking_store.hip.h -- the marking store, owned once, for the lidar layer (marking_host.hip.h) and the depth camera
// layer (depth_layer.hip.h): its device arrays, reset, housekeeping, the contested-voxel replay and the host readers.
// Included by rollout_engine.hip after the context and its helpers are defined.
//
// The device side is in marking.hip.h: MarkStore (the per-slot arrays, the pool, dGraph and lethal set), MarkHead (what
// a slot owns in the pool in front of its generator points: the depth layer's stored cluster pc_, nothing for the lidar
// layer) and the kernels that move a slot or give it pool space -- k_mk_rehash, k_mk_compact_sizes, k_mk_compact_move,
// k_mk_commit, k_mk_fix_owner -- which take the head along when there is one.
#pragma once

#include <unordered_map>

#include "dev_memory.hip.h"        // DevAllocs
#include "marking_buffers.hip.h"   // StoreBuf and its allocation

namespace {

using namespace dddmr;

// resetdGraph (MultiLayerSpinningLidar :831-839, the depth camera layer's alike): empty store, zeroed counters,
// dGraph = max_obstacle_distance on keys 0 .. n_ground.  Waits for `st`.
int store_reset(dddmr_rollout_ctx* ctx, StoreBuf& b, hipStream_t st, double max_obstacle_distance) {
  MarkStore& s = b.s;
  const size_t t = b.table;
  Drain drain{st};                         // an error exit leaves no memset running over a store that may then be freed
  HIPCHK(ctx, hipMemsetAsync(s.keys, 0, t * sizeof(unsigned long long), st));
  HIPCHK(ctx, hipMemsetAsync(s.alive, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(s.pts_ofs, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(s.pts_n, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(s.removed_seq, 0, t * sizeof(uint32_t), st));
  HIPCHK(ctx, hipMemsetAsync(s.owner, 0, t * sizeof(unsigned long long), st));
  if (b.head.pc_n) {
    HIPCHK(ctx, hipMemsetAsync(b.head.pc_ofs, 0, t * sizeof(uint32_t), st));
    HIPCHK(ctx, hipMemsetAsync(b.head.pc_n, 0, t * sizeof(uint32_t), st));
  }
  HIPCHK(ctx, hipMemsetAsync(s.lethal, 0, (size_t)b.n_ground + 1, st));
  HIPCHK(ctx, hipMemsetAsync(b.counters, 0, sizeof(MarkCounters), st));
  hipLaunchKernelGGL(k_mk_fill_dgraph, dim3((b.n_ground + 1 + 255) / 256), dim3(256), 0, st, b.n_ground + 1, s.dgraph, max_obstacle_distance);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));
  drain.armed = false;
  b.pool_used = 0;
  b.n_alive = 0;
  b.keys_used = 0;
  return DDDMR_OK;
}

struct StoreOps {             // what store_maintenance enqueued: each layer counts its launches its own way
  uint32_t kernels = 0;       // the store's own kernels
  uint32_t other = 0;         // memsets and rocPRIM's kernels (estimated)
};

// Store garbage collection when half the table holds keys and a good part of them is dead; pool compaction when half of
// the pool is used or garbage.  Both rare; both leave the device counters consistent for every route.  `temp` is rocPRIM
// scratch that takes an exclusive scan over the table.  -> runs made, or an error code (< 0)
int store_maintenance(dddmr_rollout_ctx* ctx, StoreBuf& b, hipStream_t st, void* temp, size_t temp_bytes, StoreOps& ops) {
  MarkStore& s = b.s;
  const size_t t = b.table;
  int runs = 0;
  if (b.keys_used > b.table / 2 && b.keys_used > b.n_alive + b.table / 8) {
    HIPCHK(ctx, hipMemsetAsync(b.keys_alt, 0, t * sizeof(unsigned long long), st));
    HIPCHK(ctx, hipMemsetAsync(b.alive_alt, 0, t * sizeof(uint32_t), st));
    HIPCHK(ctx, hipMemsetAsync(b.pts_ofs_alt, 0, t * sizeof(uint32_t), st));
    HIPCHK(ctx, hipMemsetAsync(b.pts_n_alt, 0, t * sizeof(uint32_t), st));
    ops.other += 4;
    if (b.head.pc_n) {
      HIPCHK(ctx, hipMemsetAsync(b.head_alt.pc_ofs, 0, t * sizeof(uint32_t), st));
      HIPCHK(ctx, hipMemsetAsync(b.head_alt.pc_n, 0, t * sizeof(uint32_t), st));
      ops.other += 2;
    }
    hipLaunchKernelGGL(k_mk_rehash, dim3((b.table + 255) / 256), dim3(256), 0, st, b.table - 1, s, b.head, b.keys_alt, b.alive_alt,
                       b.pts_ofs_alt, b.pts_n_alt, b.head_alt, b.counters);
    ++ops.kernels;
    std::swap(s.keys, b.keys_alt);
    std::swap(s.alive, b.alive_alt);
    std::swap(s.pts_ofs, b.pts_ofs_alt);
    std::swap(s.pts_n, b.pts_n_alt);
    std::swap(b.head, b.head_alt);
    b.keys_used = b.n_alive;
    ++runs;
  }
  if (b.pool_used > b.pool_cap / 2) {
    hipLaunchKernelGGL(k_mk_compact_sizes, dim3((b.table + 255) / 256), dim3(256), 0, st, b.table, s, b.head, b.compact_sizes);
    HIPCHK(ctx, rocprim::exclusive_scan(temp, temp_bytes, b.compact_sizes, b.compact_ofs, 0u, t, rocprim::plus<uint32_t>(), st));
    HIPCHK(ctx, hipMemsetAsync(&b.counters->pool_used, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_mk_compact_move, dim3((b.table + 3) / 4), dim3(256), 0, st, b.table, s, b.head, b.compact_ofs, b.pool_alt, b.counters);
    ops.kernels += 2;
    ops.other += 4;
    std::swap(s.pool, b.pool_alt);
    ++runs;
  }
  return runs;
}

// What extractEuclideanClusters hands to the sort is the clusters of at least min_cluster_size points in creation order;
// this is the reference's std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters) over them, sizes only
// (oracle/ASSUMPTIONS.md row 10): the order addPCPtr is called in.
struct DmItem { uint32_t size, ci; };
void dm_replay_sort(std::vector<DmItem>& order) {
  std::sort(order.rbegin(), order.rend(), [](const DmItem& a, const DmItem& b) { return a.size < b.size; });
}

// Contested voxels.  When several accepted clusters of one scan have their centroid in the same voxel, the reference
// keeps the cluster processed LAST, and it processes the clusters in the order
// std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters) leaves them in (EuclideanClusterExtraction::
// extract): descending size, equal sizes in the order libstdc++'s introsort happens to produce.  k_mk_slots breaks
// equal sizes by cluster index; for the (rare) updates that have a contested voxel this replays the reference's sort on
// the host -- the same std::sort, on the same sizes in the same creation order (ascending first point index =
// ascending cluster index), with a comparator that compares sizes only -- and names the voxels whose keeper differs:
// (slot, cluster) pairs for k_mk_fix_owner.  The dGraph and the lethal set do not depend on the keeper (every cluster
// contributes its minimum); what does is which points a later selfClear of the voxel looks at and resets.
// size, state, slot: nc rows, one per cluster (size 0: a point index that seeds no cluster, fused route).  A contested
// voxel takes two accepted clusters, so max_obs / 2 pairs is all there can be.
int store_tie_fixes(dddmr_rollout_ctx* ctx, const char* what, uint32_t max_obs, int min_cluster_size, uint32_t nc, const uint32_t* size,
                    const uint32_t* state, const uint32_t* slot, std::vector<uint2>& fix) {
  std::vector<DmItem> order;
  order.reserve(nc);
  for (uint32_t ci = 0; ci < nc; ++ci)
    if (size[ci] > 0 && (int)size[ci] >= min_cluster_size) order.push_back(DmItem{size[ci], ci});
  dm_replay_sort(order);
  // per contested voxel: the accepted cluster the reference processes last, against the one the device kept
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
  fix.clear();
  for (const auto& kv : keep)
    if (kv.second.claims > 1 && kv.second.ref_ci != kv.second.dev_ci) fix.push_back(make_uint2(kv.first, kv.second.ref_ci));
  if (fix.size() * 2 > (size_t)max_obs) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu contested voxels", what, fix.size());
  return DDDMR_OK;
}

// ---- host readers (the caller holds its layer's mutex and has waited for the stream the store is written on) --------
struct StoreSlot { size_t slot; unsigned long long key; uint32_t ofs, n; };

// the alive slots in slot order, each with its generator points' range in the pool or (head) its head's
int store_read_slots(dddmr_rollout_ctx* ctx, const StoreBuf& b, bool head, std::vector<StoreSlot>& out) {
  const size_t t = b.table;
  std::vector<unsigned long long> keys(t);
  std::vector<uint32_t> alive(t), ofs(t), cnt(t);
  HIPCHK(ctx, hipMemcpy(keys.data(), b.s.keys, t * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(alive.data(), b.s.alive, t * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(ofs.data(), head ? b.head.pc_ofs : b.s.pts_ofs, t * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(cnt.data(), head ? b.head.pc_n : b.s.pts_n, t * sizeof(uint32_t), hipMemcpyDeviceToHost));
  out.clear();
  for (size_t i = 0; i < t; ++i)
    if (alive[i] && keys[i]) out.push_back(StoreSlot{i, keys[i], ofs[i], cnt[i]});
  return DDDMR_OK;
}
// the used part of the pool
int store_read_pool(dddmr_rollout_ctx* ctx, const StoreBuf& b, std::vector<float4>& pool) {
  pool.resize(std::min(b.pool_used, b.pool_cap));
  if (!pool.empty()) HIPCHK(ctx, hipMemcpy(pool.data(), b.s.pool, pool.size() * sizeof(float4), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}
// the alive voxels; xyz_out null: the count only
int store_read_voxels(dddmr_rollout_ctx* ctx, const StoreBuf& b, const char* what, int32_t* xyz_out, size_t capacity, size_t* n) {
  std::vector<StoreSlot> slots;
  const int rc = store_read_slots(ctx, b, false, slots);
  if (rc != DDDMR_OK) return rc;
  if (xyz_out) {
    if (slots.size() > capacity) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu too small", what, capacity);
    for (size_t i = 0; i < slots.size(); ++i) voxel_unkey(slots[i].key, &xyz_out[3 * i], &xyz_out[3 * i + 1], &xyz_out[3 * i + 2]);
  }
  *n = slots.size();
  return DDDMR_OK;
}
int store_read_dgraph(dddmr_rollout_ctx* ctx, const StoreBuf& b, const char* what, double* values_out, size_t capacity) {
  if (capacity < (size_t)b.n_ground + 1) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu < %u", what, capacity, b.n_ground + 1);
  HIPCHK(ctx, hipMemcpy(values_out, b.s.dgraph, ((size_t)b.n_ground + 1) * sizeof(double), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}
int store_read_lethal(dddmr_rollout_ctx* ctx, const StoreBuf& b, const char* what, uint8_t* flags_out, size_t capacity) {
  if (capacity < (size_t)b.n_ground + 1) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu < %u", what, capacity, b.n_ground + 1);
  HIPCHK(ctx, hipMemcpy(flags_out, b.s.lethal, (size_t)b.n_ground + 1, hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

}  // namespace
