// static_layer.hip.h -- the static layer and the no-entry layer on the device: what StaticLayer::selfClear
// (dddmr_perception_3d/plugins/static_layer.cpp:201-231) regenerates whenever the map and ground clouds are republished,
// and what NoEntryLayer inflates around its zones (no_entry_layer.cpp:265-283):
//   generateStaticGraph     :233-285   sGraph (variable degree, CSR here) and the nearest-obstacle part of the dGraph
//   radiusSearchConnection  :287-420   the overhang part of the dGraph (:390-415); RANSAC, the ring probes and
//                                      insertWeight (:350-388, :417) draw random numbers and stay on the host
//   the zones' inflation    no_entry_layer.cpp:265-283, as a gather per ground node
//
// A build goes into the generation that is not current and is swapped in on success, so a refused or failed build leaves
// the previous graph and dGraph as they were:
//   grid_build x 2      a grid over the ground and one over the map (point_grid.hip.h), on the state's own scratch
//   k_sl_degree         a lane per ground node, in the ground grid's sorted order (a wave's lanes share their cells): the
//                       size of the node's neighbourhood, in adaptive mode also its radius index k
//   rocPRIM scan        the degrees into row_start
//   k_sl_finish         the edge count to host-mapped memory: the first host wait, and the capacity decision
//   k_sl_fill           a wave per row: the (index, d2) pairs of the ball into LDS, ranked by index, written in ascending
//                       neighbour index (the std::set's iteration order)
//   k_sl_fill_long      rows longer than DDDMR_STATIC_LAYER_ROW_LDS: a workgroup per listed row, ranking in a slab of
//                       global memory
//   k_sl_dgraph         a lane per ground node: the overhang count and the nearest map point
//   k_sl_finish         the counters and the result word: the second host wait
// The zones' dGraph is one more grid (over the zone points, temporary) and k_sl_zone, a lane per ground node.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_memory.hip.h"        // Owned, dev_alloc, Drain, feed_wait
#include "perception_stack.hip.h"  // StackState: publish_to_stack writes a host slot of the stack
#include "point_grid.hip.h"        // PointGrid and its walks, GridBuf, grid_build; rocPRIM
#include "point_grid_plan.hip.h"   // grid_shape, stage_cloud, HostCloud, cloud_arg_ok, cloud_box_ok
#include "static_layer_plan.hip.h"
#include "wave_ops.hip.h"          // wave_max, wave_sum, lanes_below

#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kSlRowLds = DDDMR_STATIC_LAYER_ROW_LDS;   // entries of a row k_sl_fill ranks in LDS (8 bytes each)
constexpr uint32_t kSlLongBlocks = 32;                        // workgroups of k_sl_fill_long, a slab of max_ground_points entries each
constexpr uint32_t kSlMinNeighbours = 5;                      // :343  nn_pc->points.size() < 5: an orphan, no overhang test
constexpr int kSlOverhangCount = 10;                          // :412  more than 10 points left after the three PassThroughs

struct SlCounters {
  unsigned long long n_edges;
  uint32_t max_degree, n_long, n_overhang, n_near, n_zone_nodes, pad;
};
struct SlResult {              // host-mapped; seq is stored last
  unsigned long long n_edges;
  uint32_t max_degree, n_long, n_overhang, n_near, n_zone_nodes;
  uint32_t seq;
};

// the neighbourhood search of one build
struct SlSearch {
  float r_box, r2;             // fixed mode: float(radius) + kSlPad, float(radius * radius)
  uint32_t number;             // adaptive mode: adaptive_connection_number
  const float* r2_tab;         // adaptive mode: [kSlAdaptiveSteps + 1] float(r_k * r_k), entry 0 unused
  int write_rows;              // generate_static_graph: the degrees become rows
};
__device__ __forceinline__ float sl_adaptive_box(int k) { return (float)sl_adaptive_radius(k) + kSlPad; }

// row_start [n + 1]: the degrees (0 in entry n, and everywhere without write_rows); nb_count [n]: the neighbourhood's size
// whether rows are written or not; kidx [n]: the radius index (0 in fixed mode); long_list: sorted positions of the rows
// k_sl_fill leaves to k_sl_fill_long.
template <bool kAdaptive>
__global__ __launch_bounds__(64) void k_sl_degree(PointGrid g, SlSearch s, uint32_t* __restrict__ row_start, uint32_t* __restrict__ nb_count,
                                                  uint8_t* __restrict__ kidx, uint32_t* __restrict__ long_list, SlCounters* __restrict__ cnt) {
  __shared__ uint8_t hist[(kAdaptive ? kSlAdaptiveSteps + 1 : 1) * 64];
  const uint32_t lane = threadIdx.x;
  const uint32_t t = blockIdx.x * 64 + lane;
  uint32_t deg = 0;
  if (t == 0) row_start[g.n] = 0;
  if (t < g.n) {
    const float4 q = g.sorted[t];
    const uint32_t me = (uint32_t)__float_as_int(q.w);
    float r_box = s.r_box, r2 = s.r2;
    int kk = 0;
    if (kAdaptive) {
      // k = 1 decides for most nodes; the others histogram the ball of r_lim by the first k that holds each point
      // (saturating bytes: only "at least `number`" is asked of the sums, and number <= 32)
      if ((uint32_t)grid_radius_count(g, q.x, q.y, q.z, sl_adaptive_box(1), s.r2_tab[1], (int)s.number) >= s.number) kk = 1;
      const int lims[3] = {8, 32, kSlAdaptiveSteps};
      for (int a = 0; a < 3 && !kk; ++a) {
        const int lim = lims[a];
        for (int k = 1; k <= lim; ++k) hist[k * 64 + lane] = 0;
        const float r2_lim = s.r2_tab[lim];
        grid_for_each(g, q.x, q.y, q.z, sl_adaptive_box(lim), [&](const float4 p) {
          const float d2 = l2_simple(p.x, p.y, p.z, q.x, q.y, q.z);
          if (d2 < r2_lim) {
            int lo = 1, hi = lim;                                // the first k with d2 < r2_tab[k] (the table ascends)
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (d2 < s.r2_tab[mid]) hi = mid; else lo = mid + 1;
            }
            const uint8_t h = hist[lo * 64 + lane];
            if (h < 255) hist[lo * 64 + lane] = h + 1;
          }
          return false;
        });
        uint32_t cum = 0;
        for (int k = 1; k <= lim; ++k) {
          cum += hist[k * 64 + lane];
          if (cum >= s.number) { kk = k; break; }
        }
      }
      if (!kk) kk = kSlAdaptiveSteps;
      r_box = sl_adaptive_box(kk);
      r2 = s.r2_tab[kk];
    }
    deg = (uint32_t)grid_radius_count(g, q.x, q.y, q.z, r_box, r2, 0x7fffffff);
    nb_count[me] = deg;
    kidx[me] = (uint8_t)kk;
    if (!s.write_rows) deg = 0;
    row_start[me] = deg;
    if (deg > kSlRowLds) long_list[atomicAdd(&cnt->n_long, 1u)] = t;
  }
  const uint32_t wmax = wave_max(deg);
  const unsigned long long sum = wave_sum((unsigned long long)deg);
  if (lane == 0 && wmax) {
    atomicMax(&cnt->max_degree, wmax);
    atomicAdd(&cnt->n_edges, sum);
  }
}

__device__ __forceinline__ void sl_row_radius(const SlSearch& s, const uint8_t* kidx, uint32_t me, float& r_box, float& r2) {
  const int kk = kidx[me];
  r_box = kk ? sl_adaptive_box(kk) : s.r_box;
  r2 = kk ? s.r2_tab[kk] : s.r2;
}

// One wave per row (a workgroup is one wave, so the barrier is the wave's own).
__global__ __launch_bounds__(64) void k_sl_fill(PointGrid g, SlSearch s, const uint8_t* __restrict__ kidx, const uint32_t* __restrict__ row_start,
                                                uint32_t* __restrict__ neighbour, float* __restrict__ weight) {
  __shared__ uint32_t s_idx[kSlRowLds];
  __shared__ float s_d2[kSlRowLds];
  const uint32_t lane = threadIdx.x;
  const float4 q = g.sorted[blockIdx.x];                           // (the grid is g.n workgroups)
  const uint32_t me = (uint32_t)__float_as_int(q.w);
  const uint32_t b = row_start[me], deg = row_start[me + 1] - b;
  if (deg == 0 || deg > kSlRowLds) return;                         // (uniform: the whole workgroup leaves)
  float r_box, r2;
  sl_row_radius(s, kidx, me, r_box, r2);
  const int x0 = grid_cx(g, q.x, -r_box), x1 = grid_cx(g, q.x, r_box);
  const int y0 = grid_cy(g, q.y, -r_box), y1 = grid_cy(g, q.y, r_box);
  const int z0 = grid_cz(g, q.z, -r_box), z1 = grid_cz(g, q.z, r_box);
  uint32_t have = 0;
  for (int cz = z0; cz <= z1; ++cz)
    for (int cy = y0; cy <= y1; ++cy) {
      const uint32_t pb = g.cell_start[(cz * g.ny + cy) * g.nx + x0], pe = g.cell_start[(cz * g.ny + cy) * g.nx + x1 + 1];
      for (uint32_t p0 = pb; p0 < pe; p0 += 64) {                  // every lane makes every trip: the ballot is complete
        const uint32_t p = p0 + lane;
        bool hit = false;
        float d2 = 0.f;
        uint32_t idx = 0;
        if (p < pe) {
          const float4 c = g.sorted[p];
          d2 = l2_simple(c.x, c.y, c.z, q.x, q.y, q.z);
          idx = (uint32_t)__float_as_int(c.w);
          hit = d2 < r2;
        }
        const unsigned long long m = __ballot(hit);
        const uint32_t pos = have + lanes_below(m);
        if (hit && pos < kSlRowLds) { s_idx[pos] = idx; s_d2[pos] = d2; }
        have += (uint32_t)__popcll(m);
      }
    }
  __syncthreads();
  const uint32_t n = min(have, deg);                               // (equal: the degree pass made the same tests)
  for (uint32_t e = lane; e < n; e += 64) {
    const uint32_t mine = s_idx[e];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n; ++j) rank += s_idx[j] < mine ? 1u : 0u;   // (a ground index appears once in a row)
    neighbour[b + rank] = mine;
    weight[b + rank] = sqrtf(s_d2[e]);                             // :270  sqrt(pcl::geometry::squaredDistance(...)), the float overload
  }
}

// slab [kSlLongBlocks][slab_stride]: x = neighbour index, y = d2 bits, in the order the lanes found them
__global__ __launch_bounds__(256) void k_sl_fill_long(PointGrid g, SlSearch s, const uint8_t* __restrict__ kidx, const uint32_t* __restrict__ row_start,
                                                      const uint32_t* __restrict__ long_list, const SlCounters* __restrict__ cnt,
                                                      uint2* __restrict__ slab, uint32_t slab_stride, uint32_t* __restrict__ neighbour,
                                                      float* __restrict__ weight) {
  __shared__ uint32_t s_have;
  const uint32_t tid = threadIdx.x;
  const uint32_t n_long = min(cnt->n_long, g.n);
  uint2* mine = slab + (size_t)blockIdx.x * slab_stride;
  for (uint32_t e = blockIdx.x; e < n_long; e += gridDim.x) {
    const float4 q = g.sorted[long_list[e]];
    const uint32_t me = (uint32_t)__float_as_int(q.w);
    const uint32_t b = row_start[me], deg = row_start[me + 1] - b;
    float r_box, r2;
    sl_row_radius(s, kidx, me, r_box, r2);
    if (tid == 0) s_have = 0;
    __syncthreads();
    const int x0 = grid_cx(g, q.x, -r_box), x1 = grid_cx(g, q.x, r_box);
    const int y0 = grid_cy(g, q.y, -r_box), y1 = grid_cy(g, q.y, r_box);
    const int z0 = grid_cz(g, q.z, -r_box), z1 = grid_cz(g, q.z, r_box);
    for (int cz = z0; cz <= z1; ++cz)
      for (int cy = y0; cy <= y1; ++cy) {
        const uint32_t pb = g.cell_start[(cz * g.ny + cy) * g.nx + x0], pe = g.cell_start[(cz * g.ny + cy) * g.nx + x1 + 1];
        for (uint32_t p = pb + tid; p < pe; p += 256) {
          const float4 c = g.sorted[p];
          const float d2 = l2_simple(c.x, c.y, c.z, q.x, q.y, q.z);
          if (d2 < r2) {
            const uint32_t pos = atomicAdd(&s_have, 1u);
            if (pos < slab_stride) mine[pos] = make_uint2((uint32_t)__float_as_int(c.w), __float_as_uint(d2));
          }
        }
      }
    __syncthreads();                                               // (with its fence: the slab's entries are visible to the workgroup)
    const uint32_t n = min(min(s_have, deg), slab_stride);
    for (uint32_t i = tid; i < n; i += 256) {
      const uint2 v = mine[i];
      uint32_t rank = 0;
      for (uint32_t j = 0; j < n; ++j) rank += mine[j].x < v.x ? 1u : 0u;
      neighbour[b + rank] = v.x;
      weight[b + rank] = sqrtf(__uint_as_float(v.y));
    }
    __syncthreads();
  }
}

struct SlDgraphArgs {
  double max_obstacle_distance, inscribed_radius;
  float r_imp_box, r_imp2;     // static_imposing_radius: float(r) + kSlPad, float(r * r)
  float r_ins_box;             // float(inscribed_radius) + kSlPad
  int edge_detection, static_graph;
};

// dgraph [n + 1] by node index; entry n keeps max_obstacle_distance (DynamicGraph::initial fills 0 .. n, no node is n)
__global__ __launch_bounds__(256) void k_sl_dgraph(PointGrid ground, PointGrid map, SlDgraphArgs a, const uint32_t* __restrict__ nb_count,
                                                   double* __restrict__ dgraph, SlCounters* __restrict__ cnt) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  bool overhang = false, near = false;
  if (t == 0) dgraph[ground.n] = a.max_obstacle_distance;
  if (t < ground.n) {
    const float4 q = ground.sorted[t];
    const uint32_t me = (uint32_t)__float_as_int(q.w);
    double v = a.max_obstacle_distance;
    if (a.edge_detection && map.n && nb_count[me] >= kSlMinNeighbours) {
      // :392-415  radiusSearch in the map, then pcl::PassThrough on z, x, y with float limits, both ends inclusive
      const float zlo = (float)((double)q.z + 0.1), zhi = (float)((double)q.z + 1.0);
      const float xlo = (float)((double)q.x - 0.5), xhi = (float)((double)q.x + 0.5);
      const float ylo = (float)((double)q.y - 0.5), yhi = (float)((double)q.y + 0.5);
      // the cells of the ball's box and of the PassThrough box, whichever is narrower
      const int x0 = max(grid_cx(map, q.x, -a.r_imp_box), grid_cx(map, xlo, -kSlPad)), x1 = min(grid_cx(map, q.x, a.r_imp_box), grid_cx(map, xhi, kSlPad));
      const int y0 = max(grid_cy(map, q.y, -a.r_imp_box), grid_cy(map, ylo, -kSlPad)), y1 = min(grid_cy(map, q.y, a.r_imp_box), grid_cy(map, yhi, kSlPad));
      const int z0 = max(grid_cz(map, q.z, -a.r_imp_box), grid_cz(map, zlo, -kSlPad)), z1 = min(grid_cz(map, q.z, a.r_imp_box), grid_cz(map, zhi, kSlPad));
      int count = 0;
      for (int cz = z0; cz <= z1 && count <= kSlOverhangCount; ++cz)
        for (int cy = y0; cy <= y1 && count <= kSlOverhangCount; ++cy) {
          const uint32_t pb = map.cell_start[(cz * map.ny + cy) * map.nx + x0], pe = map.cell_start[(cz * map.ny + cy) * map.nx + x1 + 1];
          for (uint32_t p = pb; p < pe && count <= kSlOverhangCount; ++p) {
            const float4 c = map.sorted[p];
            // (the build refuses a coordinate that is not finite, which PassThrough would drop)
            if (l2_simple(c.x, c.y, c.z, q.x, q.y, q.z) < a.r_imp2 && c.z >= zlo && c.z <= zhi && c.x >= xlo && c.x <= xhi && c.y >= ylo && c.y <= yhi)
              ++count;
          }
        }
      if (count > kSlOverhangCount) {
        overhang = true;
        v = 0.25 < v ? 0.25 : v;                                   // :413  dGraph_.setValue(index_cnt, 0.25): std::min
      }
    }
    if (a.static_graph && map.n) {
      const float best = grid_nearest(map, q.x, q.y, q.z, a.r_ins_box);
      if (best < __int_as_float(0x7F800000)) {
        const double d = (double)sqrtf(best);                      // :278  double distance_to_obstacle = sqrt(float)
        if (d < a.inscribed_radius) {
          near = true;
          v = d < v ? d : v;
        }
      }
    }
    dgraph[me] = v;
  }
  const unsigned long long bo = __ballot(overhang), bn = __ballot(near);
  if ((threadIdx.x & 63) == 0) {
    if (bo) atomicAdd(&cnt->n_overhang, (uint32_t)__popcll(bo));
    if (bn) atomicAdd(&cnt->n_near, (uint32_t)__popcll(bn));
  }
}

// The zones' inflation as a gather: node i takes sqrtf of its nearest zone point's d2 when that is inside the
// inflation ball (l2_simple is symmetric, sqrtf monotone, setValue a minimum).  pts: the ground in its own order.
__global__ __launch_bounds__(256) void k_sl_zone(const float4* __restrict__ pts, uint32_t n, PointGrid zones, float r_box, float r2,
                                                 double max_obstacle_distance, double* __restrict__ dgraph, SlCounters* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool inside = false;
  if (i == 0) dgraph[n] = max_obstacle_distance;
  if (i < n) {
    double v = max_obstacle_distance;
    if (zones.n) {
      const float4 q = pts[i];
      const float best = grid_nearest(zones, q.x, q.y, q.z, r_box);
      if (best < r2) {
        const double d = (double)sqrtf(best);                      // no_entry_layer.cpp:277
        inside = true;
        v = d < v ? d : v;
      }
    }
    dgraph[i] = v;
  }
  const unsigned long long bi = __ballot(inside);
  if ((threadIdx.x & 63) == 0 && bi) atomicAdd(&cnt->n_zone_nodes, (uint32_t)__popcll(bi));
}

__global__ void k_sl_finish(const SlCounters* __restrict__ cnt, SlResult* __restrict__ res, uint32_t seq) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  res->n_edges = cnt->n_edges;
  res->max_degree = cnt->max_degree; res->n_long = cnt->n_long; res->n_overhang = cnt->n_overhang; res->n_near = cnt->n_near;
  res->n_zone_nodes = cnt->n_zone_nodes;
  __threadfence_system();
  __hip_atomic_store(&res->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace dddmr

// ---- host (included by rollout_engine.hip after the context) ---------------------------------------------------------
namespace {

constexpr uint32_t kSlCells = 1u << 21;      // cells of each grid (grid_shape coarsens the cell until the cloud's box fits)

struct SlGeneration {                        // one selfClear regeneration
  uint32_t* row_start = nullptr;             // [max_ground_points + 1]
  uint32_t* neighbour = nullptr;             // [max_edges]
  float* weight = nullptr;                   // [max_edges]
  double* dgraph = nullptr;                  // [max_ground_points + 1]
  float4* ground_pts = nullptr;              // [max_ground_points] the ground in its own order (the zones' gather reads it)
  uint32_t n_ground = 0;
  uint64_t n_edges = 0;
};

struct StaticLayerState {
  dddmr_static_layer_config cfg{};
  SlGeneration gen[2];
  int cur = -1;                              // the generation the getters serve, -1 before the first build
  double* zone_dgraph[2] = {nullptr, nullptr};   // [max_ground_points + 1]; [0] is served while has_zones
  bool has_zones = false;
  bool grid_current = false;                 // `ground` is the grid of gen[cur]'s ground (a refused build leaves another one behind)
  uint32_t ground_epoch = 0;                 // grows when a build's n_ground differs from the one before (the planner's node weights)
  // scratch of one build
  GridBuf ground, map;
  float4* map_pts = nullptr;
  uint2* slot = nullptr;                     // [max(max_ground_points, max_map_points)] grid builder
  char* temp = nullptr;                      // rocPRIM temporary storage
  size_t temp_bytes = 0;
  uint32_t *nb_count = nullptr, *long_list = nullptr;
  uint8_t* kidx = nullptr;
  uint2* slab = nullptr;                     // [kSlLongBlocks][max_ground_points]
  float* r2_tab = nullptr;                   // [kSlAdaptiveSteps + 1]
  SlCounters* counters = nullptr;
  float4 *stage_ground = nullptr, *stage_map = nullptr;     // pinned staging of the caller's clouds
  SlResult *res_host = nullptr, *res_dev = nullptr;
  uint32_t seq = 0;
  Owned mem;
};
static_assert(!std::is_copy_constructible_v<StaticLayerState>);
static_assert(sizeof(dddmr_static_layer_config) == 64 && sizeof(dddmr_static_layer_stats) == 48, "the ctypes mirror (_capi.py) pins these sizes");

int static_layer_alloc(dddmr_rollout_ctx* ctx, StaticLayerState* m) {
  const dddmr_static_layer_config& c = m->cfg;
  const size_t G = c.max_ground_points, M = std::max<size_t>(c.max_map_points, 1), E = std::max<size_t>(c.max_edges, 1);
  DevAllocs& mem = m->mem.dev;
  for (SlGeneration& g : m->gen) {
    HIPCHK(ctx, dev_alloc(mem, &g.row_start, G + 1));
    HIPCHK(ctx, dev_alloc(mem, &g.neighbour, E));
    HIPCHK(ctx, dev_alloc(mem, &g.weight, E));
    HIPCHK(ctx, dev_alloc(mem, &g.dgraph, G + 1));
    HIPCHK(ctx, dev_alloc(mem, &g.ground_pts, G));
  }
  for (double*& z : m->zone_dgraph) HIPCHK(ctx, dev_alloc(mem, &z, G + 1));
  if (grid_alloc(mem, m->ground, kSlCells, (uint32_t)G) != 0 || grid_alloc(mem, m->map, kSlCells, (uint32_t)M) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "static_layer_create: grid storage");
  HIPCHK(ctx, dev_alloc(mem, &m->map_pts, M));
  HIPCHK(ctx, dev_alloc(mem, &m->slot, std::max(G, M)));
  {
    uint32_t* v = nullptr;
    HIPCHK(ctx, rocprim::exclusive_scan(nullptr, m->temp_bytes, v, v, 0u, std::max<size_t>((size_t)kSlCells + 1, G + 1), rocprim::plus<uint32_t>(), ctx->stream));
    m->temp_bytes = std::max<size_t>(m->temp_bytes, 4096) + 256;
  }
  HIPCHK(ctx, dev_alloc(mem, &m->temp, m->temp_bytes));
  HIPCHK(ctx, dev_alloc(mem, &m->nb_count, G));
  HIPCHK(ctx, dev_alloc(mem, &m->long_list, G));
  HIPCHK(ctx, dev_alloc(mem, &m->kidx, G));
  HIPCHK(ctx, dev_alloc(mem, &m->slab, (size_t)kSlLongBlocks * G));
  HIPCHK(ctx, dev_alloc(mem, &m->r2_tab, (size_t)kSlAdaptiveSteps + 1));
  HIPCHK(ctx, dev_alloc_zeroed(mem, &m->counters, 1));
  float tab[kSlAdaptiveSteps + 1] = {0.f};
  for (int k = 1; k <= kSlAdaptiveSteps; ++k) tab[k] = sl_radius2(sl_adaptive_radius(k));
  HIPCHK(ctx, hipMemcpy(m->r2_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
  if (host_alloc(m->mem.host, &m->stage_ground, G * sizeof(float4)) != hipSuccess || host_alloc(m->mem.host, &m->stage_map, M * sizeof(float4)) != hipSuccess ||
      host_mapped_alloc(m->mem.host, &m->res_host, &m->res_dev, sizeof(SlResult)) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "static_layer_create: pinned staging");
  std::memset(m->res_host, 0, sizeof(SlResult));
  return DDDMR_OK;
}

// the checks every static-layer entry starts with; tick_mu held
int static_layer_state(dddmr_rollout_ctx* ctx, const char* what, StaticLayerState** m_out) {
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  if (!ctx->slayer) return fail(ctx, DDDMR_ERR_STATE, "%s before static_layer_create", what);
  *m_out = ctx->slayer.get();
  return DDDMR_OK;
}

bool static_layer_radius_ok(double r) { return std::isfinite(r) && r >= 0.0 && r <= kSlMaxRadius; }

}  // namespace

extern "C" {

int dddmr_rollout_static_layer_create(dddmr_rollout_ctx* ctx, const dddmr_static_layer_config* cfg) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  const char* what = "static_layer_create";
  if (cfg->use_adaptive_connection && (cfg->adaptive_connection_number < 1 || cfg->adaptive_connection_number > kSlMaxAdaptiveNumber))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: adaptive_connection_number %u outside 1 .. %u", what, cfg->adaptive_connection_number, kSlMaxAdaptiveNumber);
  if (!static_layer_radius_ok(cfg->radius_of_ground_connection) || !static_layer_radius_ok(cfg->static_imposing_radius) ||
      !static_layer_radius_ok(cfg->inscribed_radius) || std::isnan(cfg->max_obstacle_distance))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a radius is negative, not finite or above %g m, or max_obstacle_distance is NaN", what, kSlMaxRadius);
  if (cfg->max_ground_points == 0 || cfg->reserved != 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: max_ground_points 0 or the reserved field set", what);
  if (cfg->max_ground_points > (1u << 24) || cfg->max_map_points > (1u << 26) || cfg->max_edges > (1u << 30))
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: at most 2^24 ground points, 2^26 map points and 2^30 edges", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  auto m = std::make_unique<StaticLayerState>();
  m->cfg = *cfg;
  const int rc = static_layer_alloc(ctx, m.get());
  if (rc == DDDMR_OK) ctx->slayer.reset(m.release());       // (the old state survives a failed create)
  return rc;
}

int dddmr_rollout_static_layer_build(dddmr_rollout_ctx* ctx, const float* ground_xyz, size_t n_ground, size_t ground_stride_bytes,
                                     const float* map_xyz, size_t n_map, size_t map_stride_bytes, dddmr_static_layer_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "static_layer_build";
  if (stats) *stats = dddmr_static_layer_stats{};
  if (n_ground == 0 || !cloud_arg_ok(ground_xyz, n_ground, ground_stride_bytes) || !cloud_arg_ok(map_xyz, n_map, map_stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: an empty ground, or a bad cloud pointer / stride", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StaticLayerState* m = nullptr;
  if (const int rc = static_layer_state(ctx, what, &m)) return rc;
  const dddmr_static_layer_config& c = m->cfg;
  if (n_ground > c.max_ground_points || n_map > c.max_map_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu ground / %zu map points, capacity %u / %u", what, n_ground, n_map, c.max_ground_points, c.max_map_points);
  // (the stream is idle: every call of this layer ends with its wait, so the staging buffers are free to be written)
  float lo[2][3], hi[2][3];
  if (!stage_cloud(ground_xyz, n_ground, ground_stride_bytes, m->stage_ground, lo[0], hi[0]) ||
      !stage_cloud(map_xyz, n_map, map_stride_bytes, m->stage_map, lo[1], hi[1]))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a coordinate is not finite", what);
  if (!cloud_box_ok(lo[0], hi[0]) || !cloud_box_ok(lo[1], hi[1]))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a ground or map coordinate is beyond 1e6 m, or a cloud is wider than %g m on an axis", what, (double)kCloudMaxExtent);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  SlGeneration& g = m->gen[m->cur == 0 ? 1 : 0];             // the generation nobody is served from
  const uint32_t ng = (uint32_t)n_ground, nm = (uint32_t)n_map;
  const bool adaptive = c.use_adaptive_connection != 0;
  hipStream_t st = ctx->stream;
  Drain drain{st};
  uint32_t launches = 0, waits = 0;
  HIPCHK(ctx, hipMemsetAsync(m->counters, 0, sizeof(SlCounters), st));
  HIPCHK(ctx, hipMemcpyAsync(g.ground_pts, m->stage_ground, (size_t)ng * sizeof(float4), hipMemcpyHostToDevice, st));
  launches += 2;
  if (nm) {
    HIPCHK(ctx, hipMemcpyAsync(m->map_pts, m->stage_map, (size_t)nm * sizeof(float4), hipMemcpyHostToDevice, st));
    ++launches;
  }
  m->grid_current = false;
  const float gcell = sl_ground_cell(adaptive, c.radius_of_ground_connection), mcell = sl_map_cell(c.inscribed_radius);
  grid_shape(m->ground.g, lo[0], hi[0], gcell, gcell, m->ground.cap_cells);
  if (const int rc = grid_build(ctx, m->temp, m->temp_bytes, m->ground, g.ground_pts, ng, m->slot, st)) return rc;
  grid_shape(m->map.g, lo[1], hi[1], mcell, mcell, m->map.cap_cells);
  if (const int rc = grid_build(ctx, m->temp, m->temp_bytes, m->map, m->map_pts, nm, m->slot, st)) return rc;
  launches += 4 + (nm ? 4 : 1);                              // grid_build: the memset; count, scan, scatter
  SlSearch s{};
  s.r_box = (float)c.radius_of_ground_connection + kSlPad;
  s.r2 = sl_radius2(c.radius_of_ground_connection);
  s.number = c.adaptive_connection_number;
  s.r2_tab = m->r2_tab;
  s.write_rows = c.generate_static_graph != 0;
  if (adaptive) hipLaunchKernelGGL(k_sl_degree<true>, dim3((ng + 63) / 64), dim3(64), 0, st, m->ground.g, s, g.row_start, m->nb_count, m->kidx, m->long_list, m->counters);
  else hipLaunchKernelGGL(k_sl_degree<false>, dim3((ng + 63) / 64), dim3(64), 0, st, m->ground.g, s, g.row_start, m->nb_count, m->kidx, m->long_list, m->counters);
  HIPCHK(ctx, rocprim::exclusive_scan(m->temp, m->temp_bytes, g.row_start, g.row_start, 0u, (size_t)ng + 1, rocprim::plus<uint32_t>(), st));
  uint32_t seq = next_seq(m->seq);
  hipLaunchKernelGGL(k_sl_finish, dim3(1), dim3(64), 0, st, m->counters, m->res_dev, seq);
  launches += 3;
  if (const int rc = feed_wait(st, &m->res_host->seq, seq, &waits)) return fail(ctx, DDDMR_ERR_HIP, "%s: launch or wait failed (%d)", what, rc);
  const uint64_t n_edges = m->res_host->n_edges;
  if (stats) {
    stats->n_edges = n_edges; stats->n_ground = ng; stats->n_map = nm;
    stats->max_degree = m->res_host->max_degree; stats->n_long_rows = m->res_host->n_long;
    stats->launches = launches; stats->host_waits = waits;
  }
  if (!sl_edges_fit(n_edges, c.max_edges)) {
    drain.armed = false;                                     // (the wait above left the stream idle)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %llu edges, max_edges %u", what, (unsigned long long)n_edges, c.max_edges);
  }
  if (n_edges) {
    hipLaunchKernelGGL(k_sl_fill, dim3(ng), dim3(64), 0, st, m->ground.g, s, m->kidx, g.row_start, g.neighbour, g.weight);
    hipLaunchKernelGGL(k_sl_fill_long, dim3(kSlLongBlocks), dim3(256), 0, st, m->ground.g, s, m->kidx, g.row_start, m->long_list, m->counters, m->slab,
                       c.max_ground_points, g.neighbour, g.weight);
    launches += 2;
  }
  SlDgraphArgs a{};
  a.max_obstacle_distance = c.max_obstacle_distance;
  a.inscribed_radius = c.inscribed_radius;
  a.r_imp_box = (float)c.static_imposing_radius + kSlPad;
  a.r_imp2 = sl_radius2(c.static_imposing_radius);
  a.r_ins_box = (float)c.inscribed_radius + kSlPad;
  a.edge_detection = c.enable_edge_detection != 0;
  a.static_graph = c.generate_static_graph != 0;
  hipLaunchKernelGGL(k_sl_dgraph, dim3((ng + 255) / 256), dim3(256), 0, st, m->ground.g, m->map.g, a, m->nb_count, g.dgraph, m->counters);
  seq = next_seq(m->seq);
  hipLaunchKernelGGL(k_sl_finish, dim3(1), dim3(64), 0, st, m->counters, m->res_dev, seq);
  launches += 2;
  if (const int rc = feed_wait(st, &m->res_host->seq, seq, &waits)) return fail(ctx, DDDMR_ERR_HIP, "%s: launch or wait failed (%d)", what, rc);
  drain.armed = false;
  if (m->cur < 0 || m->gen[m->cur].n_ground != ng) ++m->ground_epoch;
  g.n_ground = ng;
  g.n_edges = n_edges;
  m->cur = m->cur == 0 ? 1 : 0;
  m->grid_current = true;
  m->has_zones = false;                                      // (requestAllLayersToResetDGraph, :207: the zones are inflated again)
  if (stats) {
    stats->n_overhang = m->res_host->n_overhang; stats->n_near_obstacle = m->res_host->n_near;
    stats->launches = launches; stats->host_waits = waits;
  }
  return DDDMR_OK;
}

int dddmr_rollout_static_layer_get_graph(dddmr_rollout_ctx* ctx, uint32_t* row_start_out, uint32_t* neighbour_out, float* weight_out,
                                         size_t edge_capacity, size_t* n_edges) {
  if (!ctx || !n_edges) return DDDMR_ERR_BAD_ARG;
  const char* what = "static_layer_get_graph";
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StaticLayerState* m = nullptr;
  if (const int rc = static_layer_state(ctx, what, &m)) return rc;
  if (m->cur < 0) return fail(ctx, DDDMR_ERR_STATE, "%s before the first build", what);
  const SlGeneration& g = m->gen[m->cur];
  *n_edges = (size_t)g.n_edges;
  if ((neighbour_out || weight_out) && edge_capacity < g.n_edges)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu < %llu edges", what, edge_capacity, (unsigned long long)g.n_edges);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (row_start_out) HIPCHK(ctx, hipMemcpy(row_start_out, g.row_start, ((size_t)g.n_ground + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (neighbour_out && g.n_edges) HIPCHK(ctx, hipMemcpy(neighbour_out, g.neighbour, (size_t)g.n_edges * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (weight_out && g.n_edges) HIPCHK(ctx, hipMemcpy(weight_out, g.weight, (size_t)g.n_edges * sizeof(float), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

namespace {
int static_layer_read_dgraph(dddmr_rollout_ctx* ctx, const char* what, bool zones, double* values_out, size_t capacity) {
  if (!ctx || !values_out) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StaticLayerState* m = nullptr;
  if (const int rc = static_layer_state(ctx, what, &m)) return rc;
  if (m->cur < 0 || (zones && !m->has_zones)) return fail(ctx, DDDMR_ERR_STATE, "%s before the first %s", what, zones && m->cur >= 0 ? "set_zones of this build" : "build");
  const size_t n = (size_t)m->gen[m->cur].n_ground + 1;
  if (capacity < n) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu < %zu", what, capacity, n);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpy(values_out, zones ? m->zone_dgraph[0] : m->gen[m->cur].dgraph, n * sizeof(double), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}
}  // namespace

int dddmr_rollout_static_layer_get_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity) {
  return static_layer_read_dgraph(ctx, "static_layer_get_dgraph", false, values_out, capacity);
}

int dddmr_rollout_static_layer_get_zone_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity) {
  return static_layer_read_dgraph(ctx, "static_layer_get_zone_dgraph", true, values_out, capacity);
}

int dddmr_rollout_static_layer_set_zones(dddmr_rollout_ctx* ctx, const float* zone_xyz, size_t n_points, size_t stride_bytes,
                                         double inflation_distance, dddmr_static_layer_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "static_layer_set_zones";
  if (stats) *stats = dddmr_static_layer_stats{};
  if (!cloud_arg_ok(zone_xyz, n_points, stride_bytes) || !static_layer_radius_ok(inflation_distance))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a bad cloud pointer / stride, or an inflation distance that is negative, not finite or above %g m", what, kSlMaxRadius);
  if (n_points > (1u << 26)) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: at most 2^26 zone points", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StaticLayerState* m = nullptr;
  if (const int rc = static_layer_state(ctx, what, &m)) return rc;
  if (m->cur < 0) return fail(ctx, DDDMR_ERR_STATE, "%s before the first build", what);
  const SlGeneration& g = m->gen[m->cur];
  const uint32_t nz = (uint32_t)n_points;
  const HostCloud zones(zone_xyz, n_points, stride_bytes);
  if (!zones.finite) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a coordinate is not finite", what);
  if (!cloud_box_ok(zones.lo, zones.hi))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a zone coordinate is beyond 1e6 m, or the zones are wider than %g m on an axis", what, (double)kCloudMaxExtent);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the zones' points and grid live for this call (zones change when an operator switches one)
  DevScope scope;
  GridBuf zg;
  float4* zpts = nullptr;
  uint2* zslot = nullptr;
  const float cell = sl_zone_cell(inflation_distance);
  grid_shape(zg.g, zones.lo, zones.hi, cell, cell, kSlCells);
  if (grid_alloc(scope.mem, zg, (uint32_t)((size_t)zg.g.nx * zg.g.ny * zg.g.nz), nz) != 0) return fail(ctx, DDDMR_ERR_HIP, "%s: grid storage", what);
  HIPCHK(ctx, dev_alloc(scope.mem, &zpts, zones.pts.size()));
  HIPCHK(ctx, dev_alloc(scope.mem, &zslot, zones.pts.size()));
  hipStream_t st = ctx->stream;
  Drain drain{st};                                           // behind `scope`: an error exit waits before the scratch is freed
  uint32_t launches = 0, waits = 0;
  HIPCHK(ctx, hipMemsetAsync(m->counters, 0, sizeof(SlCounters), st));
  HIPCHK(ctx, hipMemcpyAsync(zpts, zones.pts.data(), zones.pts.size() * sizeof(float4), hipMemcpyHostToDevice, st));
  if (const int rc = grid_build(ctx, m->temp, m->temp_bytes, zg, zpts, nz, zslot, st)) return rc;
  launches += 2 + (nz ? 4 : 1);
  hipLaunchKernelGGL(k_sl_zone, dim3((g.n_ground + 255) / 256), dim3(256), 0, st, g.ground_pts, g.n_ground, zg.g, (float)inflation_distance + kSlPad,
                     sl_radius2(inflation_distance), m->cfg.max_obstacle_distance, m->zone_dgraph[1], m->counters);
  const uint32_t seq = next_seq(m->seq);
  hipLaunchKernelGGL(k_sl_finish, dim3(1), dim3(64), 0, st, m->counters, m->res_dev, seq);
  launches += 2;
  if (const int rc = feed_wait(st, &m->res_host->seq, seq, &waits)) return fail(ctx, DDDMR_ERR_HIP, "%s: launch or wait failed (%d)", what, rc);
  // (the spin saw the result word; the stream itself must be idle before the scratch goes)
  HIPCHK(ctx, hipStreamSynchronize(st));
  drain.armed = false;
  std::swap(m->zone_dgraph[0], m->zone_dgraph[1]);
  m->has_zones = true;
  if (stats) {
    stats->n_ground = g.n_ground; stats->n_zone_points = nz; stats->n_zone_nodes = m->res_host->n_zone_nodes;
    stats->launches = launches; stats->host_waits = waits;
  }
  return DDDMR_OK;
}

int dddmr_rollout_static_layer_bind(dddmr_rollout_ctx* ctx, int32_t which, int32_t slot) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "static_layer_bind";
  if (which != 0 && which != 1) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: which %d is neither 0 (static) nor 1 (no-entry)", what, which);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StaticLayerState* m = nullptr;
  if (const int rc = static_layer_state(ctx, what, &m)) return rc;
  StackState* s = stack_of(ctx, what);
  if (!s) return DDDMR_ERR_STATE;
  if (m->cur < 0 || (which == 1 && !m->has_zones)) return fail(ctx, DDDMR_ERR_STATE, "%s: that dGraph has not been computed (build, then set_zones)", what);
  const SlGeneration& g = m->gen[m->cur];
  double* dst = stack_host_slot(s, slot);
  if (!dst) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: slot %d of %d", what, slot, s->cfg.n_host_layers);
  if (g.n_ground + 1 != s->n_nodes) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: the build has %u ground nodes, the stack %u", what, g.n_ground, s->n_nodes - 1);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Drain drain{ctx->stream};
  HIPCHK(ctx, hipMemcpyAsync(dst, which == 0 ? g.dgraph : m->zone_dgraph[0], (size_t)s->n_nodes * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  drain.armed = false;
  stack_host_slot_set(s, slot);
  return DDDMR_OK;
}

}  // extern "C"
