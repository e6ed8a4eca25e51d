// global_plan.hip.h -- the pre-graph global planner's A* on the device graph: A_Star_on_PreGraph::getPath
// (dddmr_global_planner/src/a_star_on_pre_graph.cpp:191-289) over the static layer's CSR rows and a dGraph that is already
// on the device (the stack's stacked minimum, or the static layer's own), GlobalPlanner::getStartGoalID's nearest-node
// search (global_planner.cpp:407, :451) and determineDWAPlan's goal test (dynamic_window_aware_global_planner.cpp:248-270).
// The arithmetic is global_plan_plan.hip.h's; DESIGN.md 4d-4 restates it and says what differs on purpose.
//
//   k_gp_plan      one workgroup per query, no synchronisation between workgroups.  The search is the reference's serial
//                  loop; the parallelism is inside one expansion (a lane per successor of the row) and inside one pop (the
//                  lanes min-reduce the frontier).
//   k_gp_nearest   a lane per point: the nearest ground node inside radiusSearch(p, 0.5), lowest index among equals
//   k_gp_probe     a lane per point: the size of radiusSearch(p, 0.25) and whether a node of it is below inscribed_radius
//   k_gp_finish    the result word: the call's one host wait
//
// The frontier of a query is a dense array of keys (gp_key: f, then index) in global memory.  A pop is the minimum over the
// whole array, so it is exactly *f_priority_set_.begin(); the taken key's place is filled with the array's last key, so
// the array stays dense and as long as the set is large.  Equal pairs never enter twice (gp_file).  Nothing here orders
// the array, so the order in which a row's lanes append does not show.
//
// Termination: every turn of the search loop either removes a key or closes a node (at most max_expansions of those), keys
// are appended only by an expansion and at most max_open_entries are ever held, and every inner loop runs over a row, the
// key array or a parent chain whose length the closed nodes bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_memory.hip.h"        // Owned, dev_alloc, Drain, feed_wait
#include "global_plan_plan.hip.h"
#include "perception_stack.hip.h"  // StackState: the stacked minimum dGraph (dgraph_source 0)
#include "point_grid.hip.h"        // PointGrid, grid_for_each, grid_nearest_id
#include "point_grid_plan.hip.h"   // HostCloud
#include "static_layer.hip.h"      // StaticLayerState: the rows, the ground grid and the layer's own dGraph; kSlPad, sl_radius2
#include "wave_ops.hip.h"          // wave_min, wave_append

#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kGpThreads = 256;
static_assert(kGpThreads % 64 == 0, "whole waves: the searches run the wave primitives");
constexpr float kGpNearestRadius = 0.5f, kGpProbeRadius = 0.25f;       // global_planner.cpp:407, dynamic_window_...cpp:248

struct GpGraph {
  const uint32_t* row_start;     // [n + 1]
  const uint32_t* neighbour;     // ascending in a row: std::set<edge_t>'s iteration order (:220)
  const float* weight;
  const float4* pts;             // the ground in its own order
  const double* dgraph;          // [n + 1] get_min_dGraphValue
  const float* intensity;        // [n] or null: all zero
  uint32_t n;
};
struct GpParams {
  double turning_weight, expanding_radius, inscribed_radius, rate;
  uint32_t max_open, max_expansions, path_stride;
  uint32_t stamp_open;           // 2 * serial; + 1: closed.  A record of another plan has neither.
};
struct GpQueries { uint32_t start[DDDMR_GLOBAL_PLAN_MAX_QUERIES], goal[DDDMR_GLOBAL_PLAN_MAX_QUERIES]; };

// per node and query slot: x = stamp, y = g bits, z = f bits, w = parent
__device__ __forceinline__ uint4 gp_record(uint32_t stamp, float g, float f, uint32_t parent) { return make_uint4(stamp, __float_as_uint(g), __float_as_uint(f), parent); }

// rec [queries][rec_stride], keys [queries][max_open], path [queries][path_stride] (host-mapped), res [queries] (host-mapped)
__global__ __launch_bounds__(kGpThreads) void k_gp_plan(GpGraph G, GpParams P, GpQueries Q, uint4* __restrict__ rec_all, size_t rec_stride,
                                                        unsigned long long* __restrict__ keys_all, uint32_t* __restrict__ path_all,
                                                        dddmr_global_plan_result* __restrict__ res_all) {
  __shared__ unsigned long long s_wmin[kGpThreads / 64];
  __shared__ uint32_t s_count, s_full;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t qi = blockIdx.x;
  uint4* rec = rec_all + (size_t)qi * rec_stride;
  unsigned long long* keys = keys_all + (size_t)qi * P.max_open;
  const uint32_t start = Q.start[qi], goal = Q.goal[qi];
  const uint32_t closed_stamp = P.stamp_open + 1u;
  const float4 pg = G.pts[goal];
  // The search's state is held by every lane alike: each value below is computed from LDS read behind a barrier or from
  // global memory that no lane writes between two barriers, so every branch that leaves or repeats the loop is uniform.
  uint32_t n_expanded = 0, n_pushed = 1, n_discarded = 0, status = kGpNoPath;
  bool behind = false;                                                               // this pop has discarded an entry already
  if (tid == 0) {
    const float4 ps = G.pts[start];
    const float f0 = gp_dist(ps.x, ps.y, ps.z, pg.x, pg.y, pg.z);                   // :203
    rec[start] = gp_record(P.stamp_open, 0.f, f0, start);                            // :204  parent_index = start
    keys[0] = gp_key(f0, start);
    s_count = 1;
    s_full = 0;
  }
  __syncthreads();
  for (;;) {
    // ---- pop: getNode_wi_MinimumF (:74-92) ----
    const uint32_t cnt = s_count;
    if (cnt == 0) { status = kGpNoPath; break; }                                     // :213  the frontier is exhausted
    if (n_expanded >= P.max_expansions) { status = kGpBudget; break; }
    unsigned long long best = ~0ull;                                                 // (no key: an index of UINT32_MAX is no node)
    uint32_t best_at = 0;
    for (uint32_t i = tid; i < cnt; i += kGpThreads) {
      const unsigned long long k = keys[i];
      if (k < best) { best = k; best_at = i; }
    }
    const unsigned long long wmin = wave_min(best);
    if (lane == 0) s_wmin[wave] = wmin;
    __syncthreads();
    unsigned long long kmin = s_wmin[0];
#pragma unroll
    for (uint32_t w = 1; w < kGpThreads / 64; ++w) kmin = s_wmin[w] < kmin ? s_wmin[w] : kmin;
    // one round trip for all the pop and the row's head need: the node's record, its row, its point, the array's last key
    const uint32_t cur = gp_key_index(kmin);
    if (cur >= G.n) { status = kGpNoPath; break; }                                   // (cannot happen: every key names a node)
    const uint4 r = rec[cur];
    const unsigned long long last_key = keys[cnt - 1];
    const uint32_t rb = G.row_start[cur], re = G.row_start[cur + 1];
    const float4 pc = G.pts[cur];
    const float inten = G.intensity ? G.intensity[cur] : 0.f;                        // :246  points[current].intensity
    const bool is_closed = r.x == closed_stamp;
    // :77-79 erases the entry of an open node only when it is the first one looked at; behind discarded entries
    // (:85-91) the entry stays and is discarded by a later pop, its node being closed by then
    const bool remove = is_closed || !behind;
    if (remove && best == kmin) {                                                    // (a key is held once: one lane)
      keys[best_at] = last_key;
      s_count = cnt - 1;
    }
    const uint32_t held = remove ? cnt - 1 : cnt;
    __syncthreads();                                                                 // the array is dense again before anybody appends or scans
    if (is_closed) {
      ++n_discarded;
      behind = true;                                                                 // (until this pop ends)
      continue;
    }
    behind = false;
    // ---- the row of current_node (:218-268), a lane per successor; current_node is the record read above ----
    const uint32_t parent = r.w < G.n ? r.w : cur;
    const float g_cur = __uint_as_float(r.y);
    const float4 pp = G.pts[parent];
    for (uint32_t base = rb; base < re; base += kGpThreads) {                        // (uniform trip count)
      const uint32_t j = base + tid;
      bool file = false;
      unsigned long long key = 0;
      if (j < re) {
        const uint32_t nb = G.neighbour[j];
        const float w = G.weight[j];
        if (nb < G.n) {
          // (the three loads go out together, also for an edge the filter drops: the row's latency is what counts)
          const double d = G.dgraph[nb];
          const float4 pe = G.pts[nb];
          const uint4 rn = rec[nb];
          if (!gp_edge_skipped(w, P.expanding_radius, d, P.inscribed_radius)) {      // :222, :229
            const double factor = gp_factor(P.rate, d, P.inscribed_radius);          // :240
            const double theta = gp_theta(pp.x, pp.y, pc.x, pc.y, pe.x, pe.y);       // :243
            const float new_g = gp_new_g(g_cur, w, factor, theta, P.turning_weight, inten);   // :245
            const float new_h = gp_dist(pe.x, pe.y, pe.z, pg.x, pg.y, pg.z);         // :248
            const float new_f = new_g + new_h;                                       // :249
            const bool opened = rn.x == P.stamp_open, nb_closed = rn.x == closed_stamp;
            const int what = gp_file(nb_closed, opened, __uint_as_float(rn.y), __uint_as_float(rn.z), new_g, new_f);   // :254-265
            if (what) rec[nb] = gp_record(P.stamp_open, new_g, new_f, cur);
            file = what == 2;
            key = gp_key(new_f, nb);
          }
        }
      }
      // one atomic per wave for its entries
      const uint32_t at = wave_append(file, &s_count);
      if (file) {
        if (at < P.max_open) keys[at] = key;
        else s_full = 1;                                                             // (every writer stores the same)
      }
    }
    __syncthreads();
    n_pushed += s_count - held;                                                      // the set's growth (:70)
    if (s_full) { status = kGpOpenFull; break; }
    if (tid == 0) rec[cur].x = closed_stamp;                                         // :271 (read again only behind the next pop's barrier)
    ++n_expanded;
    if (cur == goal) { status = kGpFound; break; }                                   // :274
  }
  // ---- the path (:276-282), by one lane ----
  if (tid == 0) {
    dddmr_global_plan_result out;
    out.status = status;
    out.path_offset = 0;
    out.path_len = 0;
    out.n_expanded = n_expanded;
    out.n_pushed = n_pushed;
    out.n_discarded_closed = n_discarded;
    out.g_goal = 0.f;
    out.host_waits = 0;
    if (status == kGpFound) {
      uint32_t len = 1, at = goal;
      // (a chain of closed nodes' parents: at most n_expanded long; the bound holds whatever the records say)
      for (uint32_t step = 0; step < n_expanded; ++step) {
        const uint32_t p = rec[at].w;
        if (p == at || p >= G.n) break;
        at = p;
        ++len;
      }
      if (len <= P.path_stride) {
        uint32_t* path = path_all + (size_t)qi * P.path_stride;
        at = goal;
        for (uint32_t i = 0; i < len; ++i) {
          path[len - 1 - i] = at;
          at = rec[at].w;
        }
        out.path_len = len;
      }
      out.g_goal = __uint_as_float(rec[goal].y);
    }
    res_all[qi] = out;
    __threadfence_system();
  }
}

__global__ __launch_bounds__(256) void k_gp_nearest(PointGrid g, const float4* __restrict__ q, uint32_t n, float r_box, float r2, uint32_t* __restrict__ ids) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = q[i];
  static_assert(kGpNone == kGridNone, "ids_out's \"no node\" is the grid's");
  ids[i] = grid_nearest_id(g, p.x, p.y, p.z, r_box, r2).id;
}

__global__ __launch_bounds__(256) void k_gp_probe(PointGrid g, const float4* __restrict__ q, uint32_t n, float r_box, float r2, const double* __restrict__ dgraph,
                                                  double inscribed_radius, uint32_t* __restrict__ n_near, uint8_t* __restrict__ blocked) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = q[i];
  uint32_t cnt = 0;
  bool hit = false;
  grid_for_each(g, p.x, p.y, p.z, r_box, [&](const float4 c) {
    if (l2_simple(c.x, c.y, c.z, p.x, p.y, p.z) < r2) {
      ++cnt;
      const uint32_t id = (uint32_t)__float_as_int(c.w);
      if (id < g.n && dgraph[id] < inscribed_radius) hit = true;                     // :261
    }
    return false;
  });
  n_near[i] = cnt;
  blocked[i] = hit ? 1 : 0;
}

__global__ void k_gp_finish(uint32_t* __restrict__ word, uint32_t seq) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  __threadfence_system();
  __hip_atomic_store(word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace dddmr

// ---- host (included by rollout_engine.hip after the context) ---------------------------------------------------------
namespace {

struct GpOut {                               // host-mapped; seq is stored last, by k_gp_finish
  dddmr_global_plan_result res[DDDMR_GLOBAL_PLAN_MAX_QUERIES];
  uint32_t seq;
};

struct GlobalPlanState {
  dddmr_global_plan_config cfg{};
  uint32_t max_nodes = 0;                    // the static layer's max_ground_points at create: records per query slot
  uint4* rec = nullptr;                      // [max_queries][max_nodes], zeroed: no plan has stamp 0 or 1
  unsigned long long* keys = nullptr;        // [max_queries][max_open_entries]
  float* weights = nullptr;                  // [max_nodes] the ground cloud's intensity
  uint32_t weights_n = 0, weights_epoch = 0; // valid while weights_n != 0 and the static layer's ground_epoch is weights_epoch
  uint32_t serial = 0;                       // of the last plan call: the stamps are 2 * serial and 2 * serial + 1
  GpOut *out_host = nullptr, *out_dev = nullptr;
  uint32_t *path_host = nullptr, *path_dev = nullptr;        // [max_queries][max_nodes], host-mapped
  uint32_t seq = 0;
  Owned mem;
};
static_assert(!std::is_copy_constructible_v<GlobalPlanState>);
static_assert(sizeof(dddmr_global_plan_config) == 48 && sizeof(dddmr_global_plan_result) == 32, "the ctypes mirror (_capi.py) pins these sizes");

// the checks every entry but create starts with; tick_mu held.  *dgraph: the array cfg.dgraph_source names.
int global_plan_state(dddmr_rollout_ctx* ctx, const char* what, bool need_graph, GlobalPlanState** p_out, StaticLayerState** m_out, const double** dgraph) {
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  if (!ctx->gplan) return fail(ctx, DDDMR_ERR_STATE, "%s before global_plan_create", what);
  if (!ctx->slayer) return fail(ctx, DDDMR_ERR_STATE, "%s before static_layer_create", what);
  GlobalPlanState* p = ctx->gplan.get();
  StaticLayerState* m = ctx->slayer.get();
  if (m->cfg.max_ground_points > p->max_nodes)
    return fail(ctx, DDDMR_ERR_STATE, "%s: the static layer was created again with more ground points (%u) than the planner was sized for (%u)", what,
                m->cfg.max_ground_points, p->max_nodes);
  if (m->cur < 0) return fail(ctx, DDDMR_ERR_STATE, "%s before the first static_layer_build", what);
  if (need_graph && !m->cfg.generate_static_graph) return fail(ctx, DDDMR_ERR_STATE, "%s: the static layer was built without generate_static_graph", what);
  if (!need_graph && !m->grid_current) return fail(ctx, DDDMR_ERR_STATE, "%s: a static_layer_build was refused since the last good one; build again", what);
  const SlGeneration& g = m->gen[m->cur];
  if (dgraph) {
    if (p->cfg.dgraph_source == 0) {
      StackState* s = ctx->stack.get();
      if (!s) return fail(ctx, DDDMR_ERR_STATE, "%s: dgraph_source 0 before stack_create", what);
      if (s->n_nodes != g.n_ground + 1) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: the build has %u ground nodes, the stack %u", what, g.n_ground, s->n_nodes - 1);
      *dgraph = s->min_pub;
    } else {
      *dgraph = g.dgraph;
    }
  }
  *p_out = p;
  *m_out = m;
  return DDDMR_OK;
}

}  // namespace

extern "C" {

int dddmr_rollout_global_plan_create(dddmr_rollout_ctx* ctx, const dddmr_global_plan_config* cfg) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  const char* what = "global_plan_create";
  if (!std::isfinite(cfg->turning_weight) || !std::isfinite(cfg->a_star_expanding_radius) || !std::isfinite(cfg->inscribed_radius) ||
      !std::isfinite(cfg->inflation_descending_rate))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a parameter is not finite", what);
  if ((cfg->dgraph_source != 0 && cfg->dgraph_source != 1) || cfg->max_queries < 1 || cfg->max_queries > DDDMR_GLOBAL_PLAN_MAX_QUERIES ||
      cfg->max_open_entries < 1 || cfg->max_expansions < 1)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: dgraph_source %d (0 or 1), max_queries %u (1 .. %d), max_open_entries %u, max_expansions %u (at least 1)", what,
                cfg->dgraph_source, cfg->max_queries, DDDMR_GLOBAL_PLAN_MAX_QUERIES, cfg->max_open_entries, cfg->max_expansions);
  if (cfg->max_open_entries > (1u << 26)) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: at most 2^26 open entries per query", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  if (!ctx->slayer) return fail(ctx, DDDMR_ERR_STATE, "%s before static_layer_create", what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  auto p = std::make_unique<GlobalPlanState>();
  p->cfg = *cfg;
  p->max_nodes = ctx->slayer->cfg.max_ground_points;
  const size_t Q = cfg->max_queries, N = p->max_nodes;
  HIPCHK(ctx, dev_alloc_zeroed(p->mem.dev, &p->rec, Q * N));
  HIPCHK(ctx, dev_alloc(p->mem.dev, &p->keys, Q * (size_t)cfg->max_open_entries));
  HIPCHK(ctx, dev_alloc_zeroed(p->mem.dev, &p->weights, N));
  if (host_mapped_alloc(p->mem.host, &p->out_host, &p->out_dev, sizeof(GpOut)) != 0 ||
      host_mapped_alloc(p->mem.host, &p->path_host, &p->path_dev, Q * N * sizeof(uint32_t)) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "%s: pinned results", what);
  std::memset(p->out_host, 0, sizeof(GpOut));
  ctx->gplan.reset(p.release());                             // (the old state survives a failed create)
  return DDDMR_OK;
}

int dddmr_rollout_global_plan_set_node_weights(dddmr_rollout_ctx* ctx, const float* weights, size_t n) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "global_plan_set_node_weights";
  if (n && !weights) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null weights", what);
  // a negative weight would let the self edge update the node being expanded: refused
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(weights[i]) || weights[i] < 0.f) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: weight %zu is negative or not finite", what, i);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  GlobalPlanState* p = nullptr;
  StaticLayerState* m = nullptr;
  if (const int rc = global_plan_state(ctx, what, false, &p, &m, nullptr)) return rc;
  const uint32_t ng = m->gen[m->cur].n_ground;
  if (n != 0 && n != ng) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: %zu weights for %u ground nodes", what, n, ng);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (n) HIPCHK(ctx, hipMemcpy(p->weights, weights, n * sizeof(float), hipMemcpyHostToDevice));
  p->weights_n = (uint32_t)n;                                // (0: back to all zero)
  p->weights_epoch = m->ground_epoch;
  return DDDMR_OK;
}

int dddmr_rollout_global_plan_nearest(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, uint32_t* ids_out) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "global_plan_nearest";
  if (n && (!xyz || !ids_out)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument", what);
  if (n > (1u << 24)) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: at most 2^24 points", what);
  const HostCloud pts(xyz, n, 12);                           // packed points; their box goes unused
  if (!pts.finite) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a coordinate is not finite", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  GlobalPlanState* p = nullptr;
  StaticLayerState* m = nullptr;
  if (const int rc = global_plan_state(ctx, what, false, &p, &m, nullptr)) return rc;
  if (!n) return DDDMR_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevScope scope;
  float4* q = nullptr;
  uint32_t* ids = nullptr;
  HIPCHK(ctx, dev_alloc(scope.mem, &q, n));
  HIPCHK(ctx, dev_alloc(scope.mem, &ids, n));
  hipStream_t st = ctx->stream;
  Drain drain{st};                                           // behind `scope`: an error exit waits before the scratch is freed
  HIPCHK(ctx, hipMemcpyAsync(q, pts.pts.data(), n * sizeof(float4), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_gp_nearest, dim3(((uint32_t)n + 255) / 256), dim3(256), 0, st, m->ground.g, q, (uint32_t)n, kGpNearestRadius + kSlPad,
                     sl_radius2(0.5), ids);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(ids_out, ids, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  drain.armed = false;
  return DDDMR_OK;
}

int dddmr_rollout_global_plan_probe(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, uint32_t* n_ground_near_out, uint8_t* blocked_out) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "global_plan_probe";
  if (n && (!xyz || !n_ground_near_out || !blocked_out)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument", what);
  if (n > (1u << 24)) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: at most 2^24 points", what);
  const HostCloud pts(xyz, n, 12);                           // packed points; their box goes unused
  if (!pts.finite) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a coordinate is not finite", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  GlobalPlanState* p = nullptr;
  StaticLayerState* m = nullptr;
  const double* dgraph = nullptr;
  if (const int rc = global_plan_state(ctx, what, false, &p, &m, &dgraph)) return rc;
  if (!n) return DDDMR_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevScope scope;
  float4* q = nullptr;
  uint32_t* cnt = nullptr;
  uint8_t* blocked = nullptr;
  HIPCHK(ctx, dev_alloc(scope.mem, &q, n));
  HIPCHK(ctx, dev_alloc(scope.mem, &cnt, n));
  HIPCHK(ctx, dev_alloc(scope.mem, &blocked, n));
  hipStream_t st = ctx->stream;
  Drain drain{st};
  HIPCHK(ctx, hipMemcpyAsync(q, pts.pts.data(), n * sizeof(float4), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_gp_probe, dim3(((uint32_t)n + 255) / 256), dim3(256), 0, st, m->ground.g, q, (uint32_t)n, kGpProbeRadius + kSlPad, sl_radius2(0.25),
                     dgraph, p->cfg.inscribed_radius, cnt, blocked);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(n_ground_near_out, cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(blocked_out, blocked, n, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  drain.armed = false;
  return DDDMR_OK;
}

int dddmr_rollout_global_plan_plan(dddmr_rollout_ctx* ctx, const uint32_t* start_id, const uint32_t* goal_id, size_t n_queries, uint32_t* path_out,
                                   size_t path_capacity, dddmr_global_plan_result* results) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "global_plan_plan";
  if (!start_id || !goal_id || !results || n_queries == 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument or no query", what);
  if (path_capacity && !path_out) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null path_out", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  GlobalPlanState* p = nullptr;
  StaticLayerState* m = nullptr;
  const double* dgraph = nullptr;
  if (const int rc = global_plan_state(ctx, what, true, &p, &m, &dgraph)) return rc;
  if (n_queries > p->cfg.max_queries) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu queries, max_queries %u", what, n_queries, p->cfg.max_queries);
  const SlGeneration& g = m->gen[m->cur];
  GpQueries Q{};
  for (size_t i = 0; i < n_queries; ++i) {
    if (start_id[i] >= g.n_ground || goal_id[i] >= g.n_ground)
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: query %zu names node %u / %u of %u", what, i, start_id[i], goal_id[i], g.n_ground);
    Q.start[i] = start_id[i];
    Q.goal[i] = goal_id[i];
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Drain drain{st};
  if (p->serial >= 0x7FFFFFF0u) {                            // the stamps would wrap: the records start over
    HIPCHK(ctx, hipMemsetAsync(p->rec, 0, (size_t)p->cfg.max_queries * p->max_nodes * sizeof(uint4), st));
    p->serial = 0;
  }
  ++p->serial;
  if (p->weights_n && (p->weights_epoch != m->ground_epoch || p->weights_n != g.n_ground)) p->weights_n = 0;   // another ground: dropped
  GpGraph G{};
  G.row_start = g.row_start; G.neighbour = g.neighbour; G.weight = g.weight; G.pts = g.ground_pts; G.dgraph = dgraph;
  G.intensity = p->weights_n ? p->weights : nullptr;
  G.n = g.n_ground;
  GpParams P{};
  P.turning_weight = p->cfg.turning_weight; P.expanding_radius = p->cfg.a_star_expanding_radius;
  P.inscribed_radius = p->cfg.inscribed_radius; P.rate = p->cfg.inflation_descending_rate;
  P.max_open = p->cfg.max_open_entries; P.max_expansions = p->cfg.max_expansions; P.path_stride = p->max_nodes;
  P.stamp_open = 2u * p->serial;
  hipLaunchKernelGGL(k_gp_plan, dim3((uint32_t)n_queries), dim3(kGpThreads), 0, st, G, P, Q, p->rec, (size_t)p->max_nodes, p->keys, p->path_dev, p->out_dev->res);
  const uint32_t seq = next_seq(p->seq);
  hipLaunchKernelGGL(k_gp_finish, dim3(1), dim3(64), 0, st, &p->out_dev->seq, seq);
  uint32_t waits = 0;
  if (const int rc = feed_wait(st, &p->out_host->seq, seq, &waits)) return fail(ctx, DDDMR_ERR_HIP, "%s: launch or wait failed (%d)", what, rc);
  drain.armed = false;
  // the paths one after the other; a query that is not FOUND has none
  size_t at = 0;
  bool full = false, fits = true;
  for (size_t i = 0; i < n_queries; ++i) {
    dddmr_global_plan_result r = p->out_host->res[i];
    full = full || r.status == DDDMR_GLOBAL_PLAN_OPEN_FULL;
    r.path_offset = (uint32_t)at;
    r.host_waits = waits;
    if (fits && at + r.path_len <= path_capacity) {
      if (r.path_len) std::memcpy(path_out + at, p->path_host + i * (size_t)p->max_nodes, (size_t)r.path_len * sizeof(uint32_t));
    } else {
      fits = false;
    }
    at += r.path_len;
    results[i] = r;
  }
  if (full) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: a query's frontier outgrew max_open_entries %u", what, p->cfg.max_open_entries);
  if (!fits) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: the paths hold %zu nodes, path_capacity %zu", what, at, path_capacity);
  return DDDMR_OK;
}

}  // extern "C"
