// mcl_submap.hip.h -- the localiser's sub-maps on the device: what SubMaps (dddmr_mcl_3dl/src/sub_maps.cpp) does between
// the pose graph on disk and the map measure() runs against:
//   readPoseGraph's loop             :126-156   the keyframes' clouds, transformed once     -> dddmr_rollout_submap_add_keyframe
//   the keyframe radius search       :225-235   host arithmetic (mcl_submap_plan.hip.h)     -> dddmr_rollout_submap_select
//   concatenation, kd-trees, normals :283-298   NormalEstimation, setKSearch(20), ground    -> dddmr_rollout_submap_warm_up
//   swapKdTree                       :319-342                                               -> dddmr_rollout_submap_swap
//
// The keyframes live in device memory (the store, append-only); their boxes and positions stay on the host, so a warm-up
// knows its clouds' sizes and boxes without asking the device.  A warm-up gathers the listed keyframes device to device
// into the third MclMap generation (MclState::warm), builds the two grids with set_map's own builder (mcl_grid), finds
// the normal_k nearest ground points of every ground point and computes the normals:
//   k_submap_knn      a lane per ground point, in the ground grid's sorted order (a wave's lanes share their cells): growing
//                     shells of cells around the point's own; the candidates as (d2 bits, index) keys in a per-lane LDS
//                     column, kept sorted by insertion, so that the order is FLANN's (d2, index) whatever order the cells
//                     come in.  A lane stops when its k-th key's d2 is not above the squared distance to the nearest cell it
//                     has not seen, less kSubmapPad.  A lane still open after kSubmapMaxRings shells goes to a list.
//   k_submap_knn_far  a wave per listed point: brute force over the whole cloud, each lane keeping the best k of its
//                     stride, then a k-round merge of the 64 sorted columns.
//   k_submap_normals  mclobs_normal (mcl_normal.hip.h) over the rows, the observation's arithmetic unchanged.
//   k_submap_finish   the counters to host-mapped memory and the result word: the call's one host wait.
// The launches of a warm-up do not depend on the clouds' sizes (an empty cloud only skips its own).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_memory.hip.h"        // Owned, dev_alloc, Drain
#include "mcl_measure.hip.h"       // MclState, MclMap, mcl_grid: a warm-up is a generation of the measure's
#include "mcl_normal.hip.h"
#include "mcl_submap_plan.hip.h"
#include "point_grid.hip.h"        // PointGrid, GridBuf, the cell walks
#include "point_grid_plan.hip.h"   // stage_cloud, cloud_arg_ok, cloud_box_ok
#include "wave_ops.hip.h"          // wave_min, wave_max

#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kSubmapMinK = 3, kSubmapMaxK = 32;
constexpr int kSubmapMaxRings = 6;           // shells 0 .. 6 around the point's cell, then the brute-force pass
constexpr uint32_t kSubmapFarBlocks = 256;
// By how much a shell's distance bound is narrowed.  The bound is computed in cell units from (q - origin) * inv_cell
// and multiplied back; against a point binned by the same expression that is five float roundings of numbers no larger
// than kMclMaxExtent (half an ulp of 4096, 2.4e-4 m, each), and the float d2 itself is good to a few parts in 1e7 of
// distances below 6 shells' width.  4e-3 m covers both; the distance test on the candidates decides.
constexpr float kSubmapPad = 4e-3f;
constexpr unsigned long long kSubmapNoKey = ~0ull;

struct SubmapCounters { uint32_t n_far, n_nan, max_rings, pad; };
struct SubmapResult {            // host-mapped; seq is stored last
  uint32_t n_far, n_nan, max_rings;
  uint32_t seq;
};

// out[i] = store[src + (i - dst)] over the segments (dst ascending): the listed keyframes' runs, in the list's order.
//   seg [n_seg] host-mapped: x = first output index, y = first store index
__global__ __launch_bounds__(256) void k_submap_gather(const uint2* __restrict__ seg, uint32_t n_seg, uint32_t total,
                                                       const float4* __restrict__ store, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  uint32_t lo = 0, hi = n_seg;               // the last segment that starts at or before i (empty ones share their successor's start)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg[mid].x <= i) lo = mid; else hi = mid;
  }
  const uint2 s = seg[lo];
  out[i] = store[s.y + (i - s.x)];
}

// One candidate into a lane's column (col[j * 64], ascending over j < have).  `worst` is the k-th key once the column
// is full, kSubmapNoKey before.
__device__ __forceinline__ void submap_insert(unsigned long long* col, uint32_t k, uint32_t& have, unsigned long long& worst,
                                              unsigned long long key) {
  if (key >= worst) return;
  uint32_t pos = have < k ? have : k - 1;
  while (pos > 0) {
    const unsigned long long prev = col[(pos - 1) * 64];
    if (prev <= key) break;
    col[pos * 64] = prev;
    --pos;
  }
  col[pos * 64] = key;
  if (have < k) ++have;
  if (have == k) worst = col[(k - 1) * 64];
}
__device__ __forceinline__ unsigned long long submap_key(float d2, uint32_t idx) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | idx;           // d2 >= 0: the bits order as the floats do
}

// dynamic LDS: k * 64 keys.  nb [n][k]: the neighbours of ground point i (its own index space), -1 padded.
__global__ __launch_bounds__(64) void k_submap_knn(PointGrid g, uint32_t k, int32_t* __restrict__ nb, uint32_t* __restrict__ far_list,
                                                   SubmapCounters* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long submap_keys[];
  const uint32_t lane = threadIdx.x;
  const uint32_t t = blockIdx.x * 64 + lane;
  const bool active = t < g.n;
  unsigned long long* col = submap_keys + lane;
  int rings = 0;
  if (active) {
    const float4 q = g.sorted[t];
    const uint32_t me = (uint32_t)__float_as_int(q.w);
    const float ux = (q.x - g.ox) * g.inv_xy, uy = (q.y - g.oy) * g.inv_xy, uz = (q.z - g.oz) * g.inv_z;
    const int cx = grid_cx(g, q.x), cy = grid_cy(g, q.y), cz = grid_cz(g, q.z);
    const float cell_xy = 1.0f / g.inv_xy, cell_z = 1.0f / g.inv_z;
    const float inf = __int_as_float(0x7F800000);
    uint32_t have = 0;
    unsigned long long worst = kSubmapNoKey;
    bool done = false;
    for (int r = 0; r <= kSubmapMaxRings && !done; ++r) {
      rings = r;
      const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1);
      const int y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
      const int x0 = max(cx - r, 0), x1 = min(cx + r, g.nx - 1);
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          const int row = (z * g.ny + y) * g.nx;
          const bool face = abs(z - cz) == r || abs(y - cy) == r;       // the whole run of the shell's x range
          for (int side = 0; side < (face ? 1 : 2); ++side) {
            int a, b;                                                     // cells [a, b] of this row
            if (face) { a = x0; b = x1; }
            else if (side == 0) { a = b = cx - r; if (a < 0) continue; }
            else { a = b = cx + r; if (a > g.nx - 1) continue; }
            const uint32_t e = g.cell_start[row + b + 1];
            for (uint32_t p = g.cell_start[row + a]; p < e; ++p) {
              const float4 c = g.sorted[p];
              submap_insert(col, k, have, worst, submap_key(l2_simple(c.x, c.y, c.z, q.x, q.y, q.z), (uint32_t)__float_as_int(c.w)));
            }
          }
        }
      // the nearest cell not seen yet, per axis and side; none on a side where the shell has reached the grid's edge
      float bound = inf;
      if (cx - r > 0) bound = fminf(bound, (ux - (float)(cx - r)) * cell_xy);
      if (cx + r < g.nx - 1) bound = fminf(bound, ((float)(cx + r + 1) - ux) * cell_xy);
      if (cy - r > 0) bound = fminf(bound, (uy - (float)(cy - r)) * cell_xy);
      if (cy + r < g.ny - 1) bound = fminf(bound, ((float)(cy + r + 1) - uy) * cell_xy);
      if (cz - r > 0) bound = fminf(bound, (uz - (float)(cz - r)) * cell_z);
      if (cz + r < g.nz - 1) bound = fminf(bound, ((float)(cz + r + 1) - uz) * cell_z);
      if (bound == inf) {
        done = true;                                                      // every cell seen: fewer than k points is all of them
      } else if (have == k) {
        const float b = bound - kSubmapPad - 1e-6f * bound;
        done = b > 0.0f && __uint_as_float((uint32_t)(worst >> 32)) <= b * b;
      }
    }
    if (done) {
      int32_t* out = nb + (size_t)me * k;
      for (uint32_t j = 0; j < k; ++j) out[j] = j < have ? (int32_t)(uint32_t)col[j * 64] : -1;
    } else {
      far_list[atomicAdd(&cnt->n_far, 1u)] = t;
    }
  }
  rings = wave_max(rings);
  if (lane == 0 && rings > 0) atomicMax(&cnt->max_rings, (uint32_t)rings);
}

// dynamic LDS: k * 64 keys.  pts: the ground cloud in its own order.
__global__ __launch_bounds__(64) void k_submap_knn_far(PointGrid g, const float4* __restrict__ pts, uint32_t k, int32_t* __restrict__ nb,
                                                       const uint32_t* __restrict__ far_list, const SubmapCounters* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long submap_keys[];
  const uint32_t lane = threadIdx.x;
  unsigned long long* col = submap_keys + lane;
  const uint32_t n_far = min(cnt->n_far, g.n);
  for (uint32_t e = blockIdx.x; e < n_far; e += gridDim.x) {
    const float4 q = g.sorted[far_list[e]];
    const uint32_t me = (uint32_t)__float_as_int(q.w);
    uint32_t have = 0;
    unsigned long long worst = kSubmapNoKey;
    for (uint32_t j = lane; j < g.n; j += 64) {
      const float4 c = pts[j];
      submap_insert(col, k, have, worst, submap_key(l2_simple(c.x, c.y, c.z, q.x, q.y, q.z), j));
    }
    uint32_t head = 0;
    for (uint32_t o = 0; o < k; ++o) {                                    // the 64 sorted columns merged: k rounds of a wave minimum
      const unsigned long long mine = head < have ? col[head * 64] : kSubmapNoKey;
      const unsigned long long best = wave_min(mine);
      if (mine == best && best != kSubmapNoKey) ++head;                   // (keys are distinct: one lane advances)
      if (lane == 0) nb[(size_t)me * k + o] = best == kSubmapNoKey ? -1 : (int32_t)(uint32_t)best;
    }
  }
}

__global__ __launch_bounds__(256) void k_submap_normals(const float4* __restrict__ pts, uint32_t n, uint32_t k, const int32_t* __restrict__ nb,
                                                        float4* __restrict__ normals, SubmapCounters* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool is_nan = false;
  if (i < n) {
    const int32_t* row = nb + (size_t)i * k;
    uint32_t have = 0;
    while (have < k && row[have] >= 0) ++have;
    const uint32_t want = min(n, k);
    const float3 nrm = mclobs_normal(pts, reinterpret_cast<const uint32_t*>(row), have == want ? want : 0u, pts[i]);
    normals[i] = make_float4(nrm.x, nrm.y, nrm.z, 0.f);
    is_nan = nrm.x != nrm.x;
  }
  const unsigned long long b = __ballot(is_nan);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&cnt->n_nan, (uint32_t)__popcll(b));
}

__global__ void k_submap_finish(const SubmapCounters* __restrict__ cnt, SubmapResult* __restrict__ res, uint32_t seq) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  res->n_far = cnt->n_far; res->n_nan = cnt->n_nan; res->max_rings = cnt->max_rings;
  __threadfence_system();
  __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace dddmr

// ---- host (included by rollout_engine.hip after the context) ---------------------------------------------------------
namespace {

struct SubMapKeyframe {
  uint32_t ofs[2], n[2];                    // 0 corner (the map cloud), 1 ground: the run in the store
  float lo[2][3], hi[2][3];                 // the runs' boxes (zeros for an empty run)
};

struct SubMapState {
  dddmr_submap_config cfg{};
  float4* store[2] = {nullptr, nullptr};    // [max_store_map_points], [max_store_ground_points]
  uint32_t used[2] = {0, 0};
  std::vector<SubMapKeyframe> kf;
  std::vector<float> kf_pos;                // [n][3] float(position)
  // neighbour rows [max_ground_points][normal_k]: nb[0] of the generation submap_swap made current (while
  // cur_serial == MclState::serial), nb[1] of the warm-up
  int32_t* nb[2] = {nullptr, nullptr};
  uint64_t cur_serial = 0;
  bool warm_ready = false;
  uint32_t* far_list = nullptr;
  SubmapCounters* counters = nullptr;
  Owned mem;
  uint2 *seg_host = nullptr, *seg_dev = nullptr;             // host-mapped [2][max_keyframes]
  SubmapResult *res_host = nullptr, *res_dev = nullptr;
  uint32_t seq = 0;
};
static_assert(!std::is_copy_constructible_v<SubMapState>);
static_assert(sizeof(dddmr_submap_config) == 24 && sizeof(dddmr_submap_stats) == 32, "the ctypes mirror (_capi.py) pins these sizes");

int submap_alloc(dddmr_rollout_ctx* ctx, MclState* s, SubMapState* m) {
  const dddmr_submap_config& c = m->cfg;
  const size_t G = std::max<size_t>(s->cfg.max_ground_points, 1);
  HIPCHK(ctx, dev_alloc(m->mem.dev, &m->store[0], std::max<size_t>(c.max_store_map_points, 1)));
  HIPCHK(ctx, dev_alloc(m->mem.dev, &m->store[1], std::max<size_t>(c.max_store_ground_points, 1)));
  for (int b = 0; b < 2; ++b) HIPCHK(ctx, dev_alloc(m->mem.dev, &m->nb[b], G * c.normal_k));
  HIPCHK(ctx, dev_alloc(m->mem.dev, &m->far_list, G));
  HIPCHK(ctx, dev_alloc_zeroed(m->mem.dev, &m->counters, 1));
  if (host_mapped_alloc(m->mem.host, &m->seg_host, &m->seg_dev, (size_t)2 * c.max_keyframes * sizeof(uint2)) != 0 ||
      host_mapped_alloc(m->mem.host, &m->res_host, &m->res_dev, sizeof(SubmapResult)) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "submap_create: host-mapped staging");
  std::memset(m->res_host, 0, sizeof(SubmapResult));
  if (!s->has_warm) {                        // (a failed attempt's buffers stay with the mcl state until it dies)
    if (const int rc = mcl_alloc_generation(ctx, s, s->warm)) return rc;
    s->has_warm = true;
  }
  return DDDMR_OK;
}

// the checks every sub-map entry starts with; tick_mu held
int submap_state(dddmr_rollout_ctx* ctx, const char* what, bool refuse_pending, MclState** s_out, SubMapState** m_out) {
  if (refuse_pending && ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  MclState* s = ctx->mcl.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_create", what);
  if (!s->submap) return fail(ctx, DDDMR_ERR_STATE, "%s before submap_create (a new mcl_create drops the store)", what);
  *s_out = s;
  *m_out = s->submap.get();
  return DDDMR_OK;
}

}  // namespace

extern "C" {

int dddmr_rollout_submap_create(dddmr_rollout_ctx* ctx, const dddmr_submap_config* cfg) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  const char* what = "submap_create";
  if (cfg->normal_k < kSubmapMinK || cfg->normal_k > kSubmapMaxK)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: normal_k %u outside %u .. %u", what, cfg->normal_k, kSubmapMinK, kSubmapMaxK);
  if (cfg->max_keyframes == 0 || cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: max_keyframes 0 or a reserved field set", what);
  if (cfg->max_keyframes > (1u << 20) || cfg->max_store_map_points > (1u << 28) || cfg->max_store_ground_points > (1u << 28))
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: at most 2^20 keyframes and 2^28 stored points of either kind", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  MclState* s = ctx->mcl.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_create", what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  auto m = std::make_unique<SubMapState>();
  m->cfg = *cfg;
  const int rc = submap_alloc(ctx, s, m.get());
  if (rc == DDDMR_OK) s->submap.reset(m.release());     // (a new store forgets the warm-up; the old one survives a failed create)
  return rc;
}

int dddmr_rollout_submap_add_keyframe(dddmr_rollout_ctx* ctx, const float* corner_xyz, size_t n_corner, size_t corner_stride_bytes,
                                      const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes, const double T_map_base[12],
                                      const double position[3], int32_t* id_out) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "submap_add_keyframe";
  if (!position || !cloud_arg_ok(corner_xyz, n_corner, corner_stride_bytes) || !cloud_arg_ok(ground_xyz, n_ground, ground_stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument or bad cloud pointer / stride", what);
  for (int i = 0; i < 12; ++i)
    if (T_map_base && !std::isfinite(T_map_base[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: T_map_base[%d] is not finite", what, i);
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(position[i]) || !std::isfinite((float)position[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: position[%d] is not finite", what, i);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  SubMapState* m = nullptr;
  if (const int rc = submap_state(ctx, what, false, &s, &m)) return rc;
  const size_t n[2] = {n_corner, n_ground};
  if (m->kf.size() >= m->cfg.max_keyframes || m->used[0] + n[0] > m->cfg.max_store_map_points || m->used[1] + n[1] > m->cfg.max_store_ground_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: keyframe %zu with %zu + %zu points, the store holds %u / %u of %u / %u points and at most %u keyframes", what,
                m->kf.size(), n[0], n[1], m->used[0], m->used[1], m->cfg.max_store_map_points, m->cfg.max_store_ground_points, m->cfg.max_keyframes);
  SubMapKeyframe k{};
  const auto to_map = [T_map_base](float* v) {               // (null: as it is; nothing reads pts or k after a refusal)
    const float x = v[0], y = v[1], z = v[2];
    for (int a = 0; T_map_base && a < 3; ++a) v[a] = submap_transform_row(T_map_base, a, x, y, z);
  };
  std::vector<float4> pts[2] = {std::vector<float4>(n[0]), std::vector<float4>(n[1])};
  if (!stage_cloud(corner_xyz, n[0], corner_stride_bytes, pts[0].data(), k.lo[0], k.hi[0], to_map) ||
      !stage_cloud(ground_xyz, n[1], ground_stride_bytes, pts[1].data(), k.lo[1], k.hi[1], to_map))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a coordinate is not finite (before or after the transform)", what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (int c = 0; c < 2; ++c) {              // (beyond used[]: nothing reads there until the keyframe is recorded below)
    k.ofs[c] = m->used[c];
    k.n[c] = (uint32_t)n[c];
    if (n[c]) HIPCHK(ctx, hipMemcpy(m->store[c] + k.ofs[c], pts[c].data(), n[c] * sizeof(float4), hipMemcpyHostToDevice));
  }
  for (int c = 0; c < 2; ++c) m->used[c] += k.n[c];
  if (id_out) *id_out = (int32_t)m->kf.size();
  m->kf.push_back(k);
  for (int a = 0; a < 3; ++a) m->kf_pos.push_back((float)position[a]);
  return DDDMR_OK;
}

int dddmr_rollout_submap_select(dddmr_rollout_ctx* ctx, const double position[3], double radius, int32_t* ids_out, size_t capacity, size_t* n) {
  if (!ctx || !position || !n) return DDDMR_ERR_BAD_ARG;
  const char* what = "submap_select";
  if (!std::isfinite(position[0]) || !std::isfinite(position[1]) || !std::isfinite(position[2]) || !std::isfinite(radius) || radius < 0)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: the position and the radius must be finite, the radius not negative", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  SubMapState* m = nullptr;
  if (const int rc = submap_state(ctx, what, false, &s, &m)) return rc;
  const size_t cnt = submap_select(m->kf_pos.data(), m->kf.size(), position, radius, ids_out, capacity);
  *n = cnt;
  if (ids_out && cnt > capacity) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu < %zu keyframes", what, capacity, cnt);
  return DDDMR_OK;
}

int dddmr_rollout_submap_warm_up(dddmr_rollout_ctx* ctx, const int32_t* ids, size_t n_ids, dddmr_submap_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "submap_warm_up";
  if (stats) *stats = dddmr_submap_stats{};
  if (n_ids && !ids) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null id list", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  SubMapState* m = nullptr;
  if (const int rc = submap_state(ctx, what, true, &s, &m)) return rc;
  if (n_ids > m->kf.size()) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: %zu ids, the store holds %zu keyframes (a repeated id)", what, n_ids, m->kf.size());
  // the list, the totals and the boxes: host arithmetic over what add_keyframe recorded
  std::vector<uint8_t> seen(m->kf.size(), 0);
  std::vector<uint2> seg[2];
  size_t total[2] = {0, 0};
  float lo[2][3] = {{0, 0, 0}, {0, 0, 0}}, hi[2][3] = {{0, 0, 0}, {0, 0, 0}};
  bool any[2] = {false, false};
  for (size_t q = 0; q < n_ids; ++q) {
    const int32_t id = ids[q];
    if (id < 0 || (size_t)id >= m->kf.size()) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: unknown keyframe id %d", what, id);
    if (seen[id]) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: keyframe id %d is listed twice", what, id);
    seen[id] = 1;
    const SubMapKeyframe& k = m->kf[id];
    for (int c = 0; c < 2; ++c) {
      seg[c].push_back(make_uint2((uint32_t)total[c], k.ofs[c]));
      total[c] += k.n[c];
      if (!k.n[c]) continue;
      for (int a = 0; a < 3; ++a) {
        lo[c][a] = any[c] ? std::min(lo[c][a], k.lo[c][a]) : k.lo[c][a];
        hi[c][a] = any[c] ? std::max(hi[c][a], k.hi[c][a]) : k.hi[c][a];
      }
      any[c] = true;
    }
  }
  if (total[0] > s->cfg.max_map_points || total[1] > s->cfg.max_ground_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu map / %zu ground points, capacity %u / %u", what, total[0], total[1], s->cfg.max_map_points,
                s->cfg.max_ground_points);
  if (!cloud_box_ok(lo[0], hi[0]) || !cloud_box_ok(lo[1], hi[1]))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a map or ground coordinate is beyond 1e6 m, or a cloud is wider than %g m on an axis", what, (double)kMclMaxExtent);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // from here on the earlier warm-up is overwritten: it stops being ready, and an error exit waits for what was enqueued
  m->warm_ready = false;
  MclMap& w = s->warm;
  const uint32_t nm = (uint32_t)total[0], ng = (uint32_t)total[1], k = m->cfg.normal_k;
  const uint32_t seq = next_seq(m->seq);
  hipStream_t st = ctx->stream;
  Drain drain{st};
  uint32_t launches = 0;
  HIPCHK(ctx, hipMemsetAsync(m->counters, 0, sizeof(SubmapCounters), st));
  ++launches;
  float4* dst[2] = {w.map_pts, w.ground_pts};
  GridBuf* grid[2] = {&w.map, &w.ground};
  for (int c = 0; c < 2; ++c) {
    uint2* sh = m->seg_host + (size_t)c * m->cfg.max_keyframes;
    if (n_ids) std::memcpy(sh, seg[c].data(), n_ids * sizeof(uint2));
    if (total[c]) {
      hipLaunchKernelGGL(k_submap_gather, dim3(((uint32_t)total[c] + 255) / 256), dim3(256), 0, st, m->seg_dev + (size_t)c * m->cfg.max_keyframes,
                         (uint32_t)n_ids, (uint32_t)total[c], m->store[c], dst[c]);
      ++launches;
    }
    if (const int rc = mcl_grid(ctx, s, *grid[c], dst[c], lo[c], hi[c], total[c])) return rc;
    launches += total[c] ? 4 : 1;            // grid_build: the memset; count, scan, scatter
  }
  if (ng) {
    const size_t lds = (size_t)k * 64 * sizeof(unsigned long long);
    hipLaunchKernelGGL(k_submap_knn, dim3((ng + 63) / 64), dim3(64), lds, st, w.ground.g, k, m->nb[1], m->far_list, m->counters);
    hipLaunchKernelGGL(k_submap_knn_far, dim3(kSubmapFarBlocks), dim3(64), lds, st, w.ground.g, w.ground_pts, k, m->nb[1], m->far_list, m->counters);
    hipLaunchKernelGGL(k_submap_normals, dim3((ng + 255) / 256), dim3(256), 0, st, w.ground_pts, ng, k, m->nb[1], w.normals, m->counters);
    launches += 3;
  }
  hipLaunchKernelGGL(k_submap_finish, dim3(1), dim3(64), 0, st, m->counters, m->res_dev, seq);
  ++launches;
  uint32_t waits = 0;
  if (const int rc = feed_wait(st, &m->res_host->seq, seq, &waits)) return fail(ctx, DDDMR_ERR_HIP, "%s: launch or wait failed (%d)", what, rc);
  drain.armed = false;
  const SubmapResult r = *m->res_host;
  m->warm_ready = true;
  if (stats) {
    stats->n_keyframes = (uint32_t)n_ids; stats->n_map = nm; stats->n_ground = ng;
    stats->n_nan_normals = r.n_nan; stats->max_rings_searched = r.max_rings; stats->n_brute_force = r.n_far;
    stats->launches = launches; stats->host_waits = waits;
  }
  return DDDMR_OK;
}

int dddmr_rollout_submap_swap(dddmr_rollout_ctx* ctx) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "submap_swap";
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  SubMapState* m = nullptr;
  if (const int rc = submap_state(ctx, what, true, &s, &m)) return rc;
  if (!m->warm_ready) return fail(ctx, DDDMR_ERR_STATE, "%s without a warm-up", what);
  // (the stream is idle: warm_up and every measure end with their wait)
  if (s->cur < 0) s->cur = 0;
  std::swap(s->maps[s->cur], s->warm);
  std::swap(m->nb[0], m->nb[1]);
  m->cur_serial = ++s->serial;
  m->warm_ready = false;
  return DDDMR_OK;
}

int dddmr_rollout_submap_get(dddmr_rollout_ctx* ctx, int32_t which, float* map_xyz_out, size_t map_capacity, size_t* n_map, float* ground_xyz_out,
                             float* normals_out, int32_t* neighbours_out, size_t ground_capacity, size_t* n_ground) {
  if (!ctx || !n_map || !n_ground) return DDDMR_ERR_BAD_ARG;
  const char* what = "submap_get";
  if (which != 0 && which != 1) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: which %d is neither 0 (current) nor 1 (warm-up)", what, which);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  SubMapState* m = nullptr;
  if (const int rc = submap_state(ctx, what, true, &s, &m)) return rc;
  const bool have = which == 0 ? s->cur >= 0 : m->warm_ready;       // (no such generation: zero points)
  const MclMap& g = which == 0 ? s->maps[std::max(s->cur, 0)] : s->warm;
  const size_t nm = have ? g.map.g.n : 0, ng = have ? g.ground.g.n : 0, k = m->cfg.normal_k;
  *n_map = nm;
  *n_ground = ng;
  if ((map_xyz_out && map_capacity < nm) || ((ground_xyz_out || normals_out || neighbours_out) && ground_capacity < ng))
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu / %zu < %zu map / %zu ground points", what, map_capacity, ground_capacity, nm, ng);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<float4> h(std::max(nm, ng));
  const auto read3 = [&](float* out, const float4* dev, size_t n) -> int {
    if (!out || !n) return DDDMR_OK;
    HIPCHK(ctx, hipMemcpy(h.data(), dev, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) { out[3 * i] = h[i].x; out[3 * i + 1] = h[i].y; out[3 * i + 2] = h[i].z; }
    return DDDMR_OK;
  };
  if (const int rc = read3(map_xyz_out, g.map_pts, nm)) return rc;
  if (const int rc = read3(ground_xyz_out, g.ground_pts, ng)) return rc;
  if (const int rc = read3(normals_out, g.normals, ng)) return rc;
  if (neighbours_out && ng) {
    const bool from_warm_up = which == 1 || m->cur_serial == s->serial;
    if (from_warm_up) HIPCHK(ctx, hipMemcpy(neighbours_out, m->nb[which == 0 ? 0 : 1], ng * k * sizeof(int32_t), hipMemcpyDeviceToHost));
    else std::fill(neighbours_out, neighbours_out + ng * k, -1);
  }
  return DDDMR_OK;
}

}  // extern "C"
