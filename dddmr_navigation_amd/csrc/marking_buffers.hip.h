// marking_buffers.hip.h -- the building blocks the marking layers share, with their allocation: the static grids (a grid's
// storage is point_grid.hip.h's GridBuf), the cluster pipeline's scratch and the marking store.  Nothing here needs a
// context: each alloc takes the state and its sizes and returns 0 / -1 (the caller reports), and a state frees what it
// owns when it dies.
#pragma once

#include "dev_memory.hip.h"   // DevAllocs, dev_alloc
#include "marking.hip.h"
#include "point_grid.hip.h"   // GridBuf, grid_alloc

namespace dddmr {

// The ground and the static map: the points and a grid over each, uploaded once (static_grids_upload).
struct StaticGrids {
  uint32_t n_ground = 0, n_map = 0;
  float4 *ground_pts = nullptr, *map_pts = nullptr;
  GridBuf ground, map;
  Owned mem;
};
static_assert(!std::is_copy_constructible_v<StaticGrids>);

// Scratch of the cluster pipeline for one observation of up to N points (the general route's kernels of marking.hip.h,
// the depth camera's selfMark of depth_mark.hip.h).
struct ClusterScratch {
  uint32_t* parent = nullptr;
  unsigned long long *keys_a = nullptr, *keys_b = nullptr, *keys1 = nullptr;
  uint32_t *vals_a = nullptr, *vals_b = nullptr, *flags = nullptr, *incl = nullptr, *cid_incl = nullptr;
  float4* ds = nullptr;
  uint32_t* ds_first = nullptr;
  ClusterArrays cl{};                      // start, size, centroid, state, ds_count, vkey (the rest is the marking layers' own)
  uint32_t* n_groups = nullptr;            // [2]: groups of the 0.2 m and of the 0.1 m VoxelGrid
  char* temp = nullptr;                    // rocPRIM temporary storage
  size_t temp_bytes = 0;
  Owned mem;
};
static_assert(!std::is_copy_constructible_v<ClusterScratch>);

// temp_bytes: the rocPRIM temporary storage the scratch's users need (cluster_temp_bytes: the query needs the device)
inline int cluster_scratch_alloc(ClusterScratch& c, size_t N, size_t temp_bytes) {
  DevAllocs& mem = c.mem.dev;
  c.temp_bytes = temp_bytes;
  const bool ok =
      dev_alloc(mem, &c.temp, c.temp_bytes) == hipSuccess && dev_alloc(mem, &c.parent, N) == hipSuccess &&
      dev_alloc(mem, &c.keys_a, N) == hipSuccess && dev_alloc(mem, &c.keys_b, N) == hipSuccess && dev_alloc(mem, &c.keys1, N) == hipSuccess &&
      dev_alloc(mem, &c.vals_a, N) == hipSuccess && dev_alloc(mem, &c.vals_b, N) == hipSuccess && dev_alloc(mem, &c.flags, N) == hipSuccess &&
      dev_alloc(mem, &c.incl, N) == hipSuccess && dev_alloc(mem, &c.cid_incl, N) == hipSuccess && dev_alloc(mem, &c.ds, N) == hipSuccess &&
      dev_alloc(mem, &c.ds_first, N) == hipSuccess && dev_alloc(mem, &c.cl.start, N + 1) == hipSuccess &&
      dev_alloc(mem, &c.cl.size, N) == hipSuccess && dev_alloc(mem, &c.cl.centroid, N) == hipSuccess &&
      dev_alloc(mem, &c.cl.state, N) == hipSuccess && dev_alloc(mem, &c.cl.ds_count, N) == hipSuccess &&
      dev_alloc(mem, &c.cl.vkey, 3 * N) == hipSuccess && dev_alloc(mem, &c.n_groups, 2) == hipSuccess;
  return ok ? 0 : -1;
}

struct StoreBuf {
  MarkStore s{};
  MarkHead head{};                         // null pointers: a store without heads
  uint32_t* clear_list = nullptr;          // [table] alive slots selfClear has to test, this update
  // second set of the arrays a slot moves with, for the garbage collection (k_mk_rehash) and the pool compaction
  unsigned long long* keys_alt = nullptr;
  uint32_t *alive_alt = nullptr, *pts_ofs_alt = nullptr, *pts_n_alt = nullptr;
  MarkHead head_alt{};
  float4* pool_alt = nullptr;
  uint32_t *compact_sizes = nullptr, *compact_ofs = nullptr;
  MarkCounters* counters = nullptr;        // device
  uint32_t table = 0, pool_cap = 0, n_ground = 0;
  uint32_t pool_used = 0, n_alive = 0, keys_used = 0;   // host mirrors
  Owned mem;
};
static_assert(!std::is_copy_constructible_v<StoreBuf>);

// table: the power of two >= max(min_table, 2 * max_markings)
inline int store_alloc(StoreBuf& b, uint32_t min_table, uint32_t max_markings, uint32_t pool_cap, uint32_t n_ground, bool with_fov_flag,
                       bool with_head) {
  uint32_t t = min_table;
  while (t < 2 * max_markings) t <<= 1;
  b.table = t;
  b.pool_cap = pool_cap;
  b.n_ground = n_ground;
  MarkStore& s = b.s;
  DevAllocs& mem = b.mem.dev;
  bool ok = dev_alloc(mem, &s.keys, t) == hipSuccess && dev_alloc(mem, &s.alive, t) == hipSuccess && dev_alloc(mem, &s.pts_ofs, t) == hipSuccess &&
            dev_alloc(mem, &s.pts_n, t) == hipSuccess && dev_alloc(mem, &s.removed_seq, t) == hipSuccess && dev_alloc(mem, &s.owner, t) == hipSuccess &&
            dev_alloc(mem, &s.alive_list, t) == hipSuccess && dev_alloc(mem, &s.removed_list, t) == hipSuccess &&
            (!with_fov_flag || dev_alloc(mem, &s.fov_flag, t) == hipSuccess) && dev_alloc(mem, &s.pool, pool_cap) == hipSuccess &&
            dev_alloc(mem, &s.dgraph, (size_t)n_ground + 1) == hipSuccess && dev_alloc(mem, &s.lethal, (size_t)n_ground + 1) == hipSuccess &&
            dev_alloc(mem, &b.clear_list, t) == hipSuccess && dev_alloc(mem, &b.keys_alt, t) == hipSuccess && dev_alloc(mem, &b.alive_alt, t) == hipSuccess &&
            dev_alloc(mem, &b.pts_ofs_alt, t) == hipSuccess && dev_alloc(mem, &b.pts_n_alt, t) == hipSuccess &&
            dev_alloc(mem, &b.pool_alt, pool_cap) == hipSuccess;
  if (ok && with_head)
    ok = dev_alloc(mem, &b.head.pc_ofs, t) == hipSuccess && dev_alloc(mem, &b.head.pc_n, t) == hipSuccess &&
         dev_alloc(mem, &b.head_alt.pc_ofs, t) == hipSuccess && dev_alloc(mem, &b.head_alt.pc_n, t) == hipSuccess;
  ok = ok && dev_alloc(mem, &b.compact_sizes, t) == hipSuccess && dev_alloc(mem, &b.compact_ofs, t) == hipSuccess &&
       dev_alloc(mem, &b.counters, 1) == hipSuccess;
  return ok ? 0 : -1;
}

}  // namespace dddmr
