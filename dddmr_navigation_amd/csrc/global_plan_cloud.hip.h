// global_plan_cloud.hip.h -- the global planner's default A* on the device: A_Star_on_Graph::getPath
// (dddmr_global_planner/src/a_star_on_pc.cpp:200-329, use_pre_graph: false) with isLineOfSightClear (:168-198), over what is
// resident already: the static layer's ground and its grid, the stack's stacked minimum dGraph and lethal masks, and the
// records, key array and stamps of the planner state that k_gp_plan searches (global_plan.hip.h).  It needs no sGraph.
// The arithmetic is global_plan_cloud_plan.hip.h's and global_plan_plan.hip.h's; DESIGN.md 4d-5 restates it with its
// lines, says what differs on purpose and that the restatement it is tested against is not pinned to compiled reference
// code yet.
//
//   k_gp_plan_cloud   one workgroup per query, 256 lanes, no synchronisation between workgroups.  The search is the
//                     reference's serial loop; the parallelism is inside one expansion:
//     pop             the lanes min-reduce the key array, as k_gp_plan does (getNode_wi_MinimumF :70-88, `behind` included)
//     successors      radiusSearch(pcl_now, a_star_expanding_radius_) on the ground (:240): the waves walk the rows of cells
//                     of the ball's box and append (d2, id) to an LDS list, one LDS add per wave and row segment
//     8 nearest       fewer than 8 (:243): boxes of doubling half width until 8 points lie inside the ball the box is sure
//                     to contain (gp_cloud_shell_d2), then eight min-reductions over (d2, id), each above the one before
//     avg_intensity   (:248-252) only with node intensities: the list ranked by (d2, id) by counting, summed by one lane
//     per successor   a lane each (256 at a time): dGraph value, point, record; the lethal skip (:263); the number of
//                     line-of-sight samples by the float recurrence of :181
//     line of sight   the (edge, sample) pairs of the 256 successors dealt across the lanes; a lane counts the lethal points
//                     in radiusSearch(sample, 2 * inscribed_radius) up to 2: ground nodes weighted by popcount(mask), plus
//                     the points of the host layers' lethal cloud.  More than one blocks the edge (:193); the verdict is an
//                     OR, so no order among the samples shows
//     cost and filing :278-306 as k_gp_plan's (gp_factor, gp_theta, gp_file), new_g by gp_cloud_new_g
//
// The aggregate lethal cloud (stacked_perception.cpp:142-155) is the plugins' lethal clouds appended: a ground node that
// is lethal in two device layers is two points, hence the popcount; a layer left on the host hands its lethal points in
// through global_plan_set_lethal_points, which get a grid of their own.
//
// Equal distances are taken in ascending index (the project's rule; nanoflann orders them by its tree walk).  It shows
// only in which nodes make the 8 nearest and in the float sum of avg_intensity.
//
// Termination: every turn of the search loop either removes a key or closes a node (at most max_expansions of those);
// keys are appended only by an expansion and at most max_open_entries are held.  Inside an expansion every loop runs over
// the rows and points of a bounded box of cells (at most the whole grid), at most kGpcMaxDoublings doublings of the box,
// eight reductions, at most kGpCloudMaxSuccessors successors, at most kGpLosMaxSamples samples per edge (an edge that
// would take more is blocked without a march), the key array, or a parent chain that the closed nodes bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_memory.hip.h"              // dev_alloc, Drain, feed_wait
#include "global_plan.hip.h"             // GpParams, GpQueries, gp_record, GlobalPlanState, global_plan_state
#include "global_plan_cloud_plan.hip.h"
#include "wave_ops.hip.h"                // wave_min, wave_append, block_excl_scan

#pragma clang fp contract(off)

namespace dddmr {

constexpr int kGpcMaxDoublings = 40;     // 2^40 times the radius: beyond any grid a build accepts (4096 m)

struct GpcArgs {
  PointGrid ground;              // the static layer's ground grid
  PointGrid extra;               // the host layers' lethal points; n == 0: none
  const float4* pts;             // the ground in its own order
  const double* dgraph;          // [n + 1] get_min_dGraphValue
  const uint8_t* mask;           // [n + 1] lethal bits of the device layers; null: no device layer (dgraph_source 1)
  const float* intensity;        // [n] or null: all zero
  const float* node_weight;      // [n] or null: all zero (sGraph_ptr_->getNodeWeight, static_graph.cpp:62)
  uint32_t n;
  float r_box, r2;               // a_star_expanding_radius: float(r) + kSlPad, gp_cloud_radius2
  float los_box, los_r2;         // 2 * inscribed_radius, likewise
};

struct GpcBox { int x0, x1, y0, y1, z0, z1; };
__device__ __forceinline__ GpcBox gpc_box(const PointGrid& g, float qx, float qy, float qz, float h) {
  return GpcBox{grid_cx(g, qx, -h), grid_cx(g, qx, h), grid_cy(g, qy, -h), grid_cy(g, qy, h), grid_cz(g, qz, -h), grid_cz(g, qz, h)};
}
__device__ __forceinline__ bool gpc_box_is_grid(const PointGrid& g, const GpcBox& b) {
  return b.x0 == 0 && b.y0 == 0 && b.z0 == 0 && b.x1 == g.nx - 1 && b.y1 == g.ny - 1 && b.z1 == g.nz - 1;
}

// The workgroup walks the points of a box of cells (all: every point of the grid).  The bounds of up to 256 rows of cells
// go to LDS in one round of loads; a wave then takes every fourth row and its lanes stride the row's run.  f(in, p) is
// called by all lanes of a wave together (in: this lane has a point), so f may ballot.  Call from uniform control flow.
template <class F>
__device__ __forceinline__ void gpc_walk(const PointGrid& g, const GpcBox& b, bool all, uint2* s_rows, uint32_t tid, F&& f) {
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
  if (all) {
    for (uint32_t k0 = wave * 64u; k0 < g.n; k0 += kGpThreads) {
      const uint32_t k = k0 + lane;
      const bool in = k < g.n;
      f(in, in ? g.sorted[k] : none);
    }
    return;
  }
  const int nys = b.y1 - b.y0 + 1, nrows = nys * (b.z1 - b.z0 + 1);
  for (int base = 0; base < nrows; base += (int)kGpThreads) {
    const int row = base + (int)tid;
    __syncthreads();                                                                 // (s_rows is free)
    if (row < nrows) {
      const int cell = ((b.z0 + row / nys) * g.ny + (b.y0 + row % nys)) * g.nx;
      s_rows[tid] = make_uint2(g.cell_start[cell + b.x0], g.cell_start[cell + b.x1 + 1]);
    }
    __syncthreads();
    const uint32_t m = (uint32_t)min((int)kGpThreads, nrows - base);
    for (uint32_t r = wave; r < m; r += kGpThreads / 64u) {
      const uint2 be = s_rows[r];
      for (uint32_t k0 = be.x; k0 < be.y; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const bool in = k < be.y;
        f(in, in ? g.sorted[k] : none);
      }
    }
  }
}

__device__ __forceinline__ unsigned long long gpc_key(float d2, uint32_t id) { return ((unsigned long long)__float_as_uint(d2) << 32) | id; }   // d2 >= 0: its bits order

// the lethal points of radiusSearch(sample, 2 * inscribed_radius) on the aggregate lethal cloud, counted up to 2
__device__ __forceinline__ uint32_t gpc_lethal_count(const GpcArgs& A, float sx, float sy, float sz) {
  uint32_t cnt = 0;
  if (A.mask) {
    grid_for_each(A.ground, sx, sy, sz, A.los_box, [&](const float4 c) {
      if (l2_simple(c.x, c.y, c.z, sx, sy, sz) < A.los_r2) {
        const uint32_t id = (uint32_t)__float_as_int(c.w);
        if (id < A.n) cnt += (uint32_t)__popc((uint32_t)A.mask[id]);                 // a point per layer that holds the node lethal
      }
      return cnt >= 2u;
    });
  }
  if (cnt < 2u && A.extra.n) cnt += (uint32_t)grid_radius_count(A.extra, sx, sy, sz, A.los_box, A.los_r2, (int)(2u - cnt));
  return cnt;
}

// rec [queries][rec_stride], keys [queries][max_open], path [queries][path_stride] (host-mapped), res [queries] (host-mapped)
__global__ __launch_bounds__(kGpThreads) void k_gp_plan_cloud(GpcArgs A_in, GpParams P_in, GpQueries Q, uint4* __restrict__ rec_all, size_t rec_stride,
                                                              unsigned long long* __restrict__ keys_all, uint32_t* __restrict__ path_all,
                                                              dddmr_global_plan_cloud_result* __restrict__ res_all) {
  __shared__ unsigned long long s_wmin[kGpThreads / 64];
  __shared__ unsigned long long s_list[kGpCloudMaxSuccessors];      // (d2 bits, id) of the successors
  __shared__ float s_inten[kGpCloudMaxSuccessors];                  // their intensities in list order
  __shared__ uint2 s_rows[kGpThreads];
  __shared__ float4 s_pe[kGpThreads];                               // of the 256 successors in hand: point, dt, samples before, verdict
  __shared__ float s_dt[kGpThreads];
  __shared__ uint32_t s_prefix[kGpThreads + 1];
  __shared__ uint32_t s_flag[kGpThreads];
  __shared__ uint32_t s_wsum[kGpThreads / 64];
  __shared__ uint32_t s_count, s_full, s_n, s_tmp;
  __shared__ float s_avg;
  __shared__ uint32_t s_ctr[4];
  // The two argument structs are read from LDS, not held in scalar registers: with 60 dwords of them live across the
  // whole search the scalar file overflowed into vector lanes by more than a hundred registers (profiles/r29_*_resources.json).
  __shared__ __attribute__((aligned(16))) unsigned char s_args[sizeof(GpcArgs)], s_params[sizeof(GpParams)];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) {
    *reinterpret_cast<GpcArgs*>(s_args) = A_in;
    *reinterpret_cast<GpParams*>(s_params) = P_in;
  }
  __syncthreads();
  const GpcArgs& A = *reinterpret_cast<const GpcArgs*>(s_args);
  const GpParams& P = *reinterpret_cast<const GpParams*>(s_params);
  const uint32_t qi = blockIdx.x;
  uint4* rec = rec_all + (size_t)qi * rec_stride;
  unsigned long long* keys = keys_all + (size_t)qi * P.max_open;
  const uint32_t start = Q.start[qi], goal = Q.goal[qi];
  const uint32_t closed_stamp = P.stamp_open + 1u;
  const float4 pg = A.pts[goal];
  // (as in k_gp_plan: every lane holds the search's state alike, every branch that leaves or repeats a loop is uniform)
  uint32_t n_expanded = 0, n_pushed = 1, n_discarded = 0, status = kGpNoPath;
  uint32_t n_knn = 0, max_succ = 0;
  uint32_t c_lethal = 0, c_tested = 0, c_blocked = 0, c_capped = 0;                  // this lane's share
  bool behind = false;
  if (tid == 0) {
    const float4 ps = A.pts[start];
    const float f0 = gp_dist(ps.x, ps.y, ps.z, pg.x, pg.y, pg.z);                   // :212
    rec[start] = gp_record(P.stamp_open, 0.f, f0, start);                            // :213  parent_index = start
    keys[0] = gp_key(f0, start);
    s_count = 1;
    s_full = 0;
    s_ctr[0] = s_ctr[1] = s_ctr[2] = s_ctr[3] = 0;
  }
  __syncthreads();
  for (;;) {
    // ---- pop: getNode_wi_MinimumF (:70-88), k_gp_plan's ----
    const uint32_t cnt_keys = s_count;
    if (cnt_keys == 0) { status = kGpNoPath; break; }                                // :231  the frontier is exhausted
    if (n_expanded >= P.max_expansions) { status = kGpBudget; break; }
    unsigned long long best = ~0ull;
    uint32_t best_at = 0;
    for (uint32_t i = tid; i < cnt_keys; i += kGpThreads) {
      const unsigned long long k = keys[i];
      if (k < best) { best = k; best_at = i; }
    }
    const unsigned long long wmin = wave_min(best);
    if (lane == 0) s_wmin[wave] = wmin;
    __syncthreads();
    unsigned long long kmin = s_wmin[0];
#pragma unroll
    for (uint32_t w = 1; w < kGpThreads / 64; ++w) kmin = s_wmin[w] < kmin ? s_wmin[w] : kmin;
    const uint32_t cur = gp_key_index(kmin);
    if (cur >= A.n) { status = kGpNoPath; break; }                                   // (cannot happen: every key names a node)
    const uint4 r = rec[cur];
    const unsigned long long last_key = keys[cnt_keys - 1];
    const float4 pc = A.pts[cur];                                                    // :237  pcl_now
    const bool is_closed = r.x == closed_stamp;
    const bool remove = is_closed || !behind;                                        // :73-75 against :81-86, as k_gp_plan
    if (remove && best == kmin) {
      keys[best_at] = last_key;
      s_count = cnt_keys - 1;
    }
    if (tid == 0) { s_n = 0; s_tmp = 0; }
    const uint32_t held = remove ? cnt_keys - 1 : cnt_keys;
    __syncthreads();
    if (is_closed) {
      ++n_discarded;
      behind = true;
      continue;
    }
    behind = false;
    const uint32_t parent = r.w < A.n ? r.w : cur;
    const float g_cur = __uint_as_float(r.y);
    const float4 pp = A.pts[parent];

    // ---- the successors: radiusSearch(pcl_now, a_star_expanding_radius_) (:240) ----
    gpc_walk(A.ground, gpc_box(A.ground, pc.x, pc.y, pc.z, A.r_box), false, s_rows, tid, [&](bool in, const float4 c) {
      const float d2 = l2_simple(c.x, c.y, c.z, pc.x, pc.y, pc.z);
      const bool hit = in && d2 < A.r2;                                              // RadiusResultSet::addPoint: strictly
      const uint32_t at = wave_append(hit, &s_n);
      if (hit && at < kGpCloudMaxSuccessors) s_list[at] = gpc_key(d2, (uint32_t)__float_as_int(c.w));
    });
    __syncthreads();
    uint32_t cnt = s_n;
    if (cnt < kGpCloudKnn) {
      // ---- nearestKSearch(pcl_now, 8) replaces the list (:243-245) ----
      ++n_knn;
      float h = A.r_box;
      GpcBox bx{};
      bool all = false;
      for (int it = 0;; ++it) {
        h = h * 2.0f;
        bx = gpc_box(A.ground, pc.x, pc.y, pc.z, h);
        all = it >= kGpcMaxDoublings || gpc_box_is_grid(A.ground, bx);
        if (all) break;
        const float d2_max = gp_cloud_shell_d2(h);
        uint32_t mine = 0;
        gpc_walk(A.ground, bx, false, s_rows, tid, [&](bool in, const float4 c) {
          if (in && l2_simple(c.x, c.y, c.z, pc.x, pc.y, pc.z) <= d2_max) ++mine;
        });
        if (mine) atomicAdd(&s_tmp, mine);
        __syncthreads();
        const uint32_t inside = s_tmp;
        __syncthreads();
        if (tid == 0) s_tmp = 0;                                                     // (read again only behind the next walk's barriers)
        if (gp_cloud_shell_accepts(inside, false)) break;
      }
      unsigned long long prev = 0;
      cnt = 0;
      for (uint32_t j = 0; j < kGpCloudKnn; ++j) {
        unsigned long long lo = ~0ull;
        gpc_walk(A.ground, bx, all, s_rows, tid, [&](bool in, const float4 c) {
          const unsigned long long k = gpc_key(l2_simple(c.x, c.y, c.z, pc.x, pc.y, pc.z), (uint32_t)__float_as_int(c.w));
          if (in && (j == 0 || k > prev) && k < lo) lo = k;
        });
        const unsigned long long wlo = wave_min(lo);
        if (lane == 0) s_wmin[wave] = wlo;
        __syncthreads();
        unsigned long long k8 = s_wmin[0];
#pragma unroll
        for (uint32_t w = 1; w < kGpThreads / 64; ++w) k8 = s_wmin[w] < k8 ? s_wmin[w] : k8;
        if (tid == 0 && k8 != ~0ull) s_list[j] = k8;
        __syncthreads();                                                             // s_wmin is free, s_list[j] stands
        if (k8 == ~0ull) break;                                                      // (cannot happen: the ground has 8 nodes)
        prev = k8;
        cnt = j + 1;
      }
    }
    max_succ = cnt > max_succ ? cnt : max_succ;
    if (cnt > kGpCloudMaxSuccessors) { status = kGpRowFull; break; }

    // ---- avg_intensity (:248-252): a float sum in list order, the list ascending in (d2, id) ----
    float avg = 0.f;
    if (A.intensity) {
      for (uint32_t i = tid; i < cnt; i += kGpThreads) {
        const unsigned long long k = s_list[i];
        const float w = A.intensity[(uint32_t)k];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < cnt; ++j) rank += s_list[j] < k ? 1u : 0u;
        s_inten[rank] = w;                                                           // (the ids differ, so the ranks do)
      }
      __syncthreads();
      if (tid == 0) {
        float sum = 0.f;
        for (uint32_t i = 0; i < cnt; ++i) sum += s_inten[i];
        s_avg = gp_cloud_avg_intensity(sum, cnt);
      }
      __syncthreads();
      avg = s_avg;
    }

    // ---- the successors, 256 at a time (:254-306); a successor occurs once, so no lane's record is another's ----
    for (uint32_t base = 0; base < cnt; base += kGpThreads) {
      const uint32_t j = base + tid;
      bool live = false;
      uint32_t nb = 0, ns = 0;
      float d2 = 0.f, dt = 0.f, nw = 0.f;
      double d = 0.0;
      float4 pe = make_float4(0.f, 0.f, 0.f, 0.f);
      uint4 rn = make_uint4(0, 0, 0, 0);
      if (j < cnt) {
        const unsigned long long k = s_list[j];
        nb = (uint32_t)k;
        d2 = __uint_as_float((uint32_t)(k >> 32));
        d = A.dgraph[nb];                                                            // :260
        pe = A.pts[nb];
        rn = rec[nb];
        nw = A.node_weight ? A.node_weight[nb] : 0.f;                                // :287
        if (d < P.inscribed_radius) {                                                // :263
          ++c_lethal;
        } else {
          live = true;
          if (gp_cloud_los_needed(d2, P.inscribed_radius)) {                         // :273
            ++c_tested;
            dt = gp_cloud_los_dt(pe.x - pc.x, pe.y - pc.y, pe.z - pc.z, P.inscribed_radius);   // :171-180
            ns = gp_cloud_los_samples(dt);
          }
        }
      }
      const bool capped = ns > kGpLosMaxSamples;                                     // blocked without a march
      s_pe[tid] = pe;
      s_dt[tid] = dt;
      s_flag[tid] = capped ? 1u : 0u;
      const uint32_t steps = capped ? 0u : ns;
      uint32_t total;
      s_prefix[tid + 1] = block_excl_scan<kGpThreads / 64>(steps, s_wsum, &total) + steps;
      if (tid == 0) s_prefix[0] = 0;
      __syncthreads();
      // ---- isLineOfSightClear (:168-198): a lane per (edge, sample) ----
      for (uint32_t p = tid; p < total; p += kGpThreads) {
        uint32_t lo = 0, hi = kGpThreads;                                            // the last e with s_prefix[e] <= p: p's edge
        while (hi - lo > 1u) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_prefix[mid] <= p) lo = mid;
          else hi = mid;
        }
        if (((volatile uint32_t*)s_flag)[lo]) continue;                              // blocked already: an OR over the samples
        const float4 e = s_pe[lo];
        const float rr = gp_cloud_los_r(gp_cloud_los_t(s_dt[lo], p - s_prefix[lo]));
        const float sx = gp_cloud_los_coord(pc.x, e.x - pc.x, rr), sy = gp_cloud_los_coord(pc.y, e.y - pc.y, rr),
                    sz = gp_cloud_los_coord(pc.z, e.z - pc.z, rr);                   // :187-189
        if (gpc_lethal_count(A, sx, sy, sz) > 1u) ((volatile uint32_t*)s_flag)[lo] = 1u;   // :193  pidx.size() > 1
      }
      __syncthreads();
      // ---- cost and filing (:278-306), as k_gp_plan ----
      bool file = false;
      unsigned long long key = 0;
      if (live) {
        if (s_flag[tid]) {
          ++c_blocked;
          if (capped) ++c_capped;
        } else {
          const double factor = gp_factor(P.rate, d, P.inscribed_radius);            // :278
          const double theta = gp_theta(pp.x, pp.y, pc.x, pc.y, pe.x, pe.y);         // :281
          const float new_g = gp_cloud_new_g(g_cur, sqrtf(d2), factor, nw, theta, P.turning_weight, avg);   // :288
          const float new_h = gp_dist(pe.x, pe.y, pe.z, pg.x, pg.y, pg.z);           // :289
          const float new_f = new_g + new_h;                                         // :290
          const bool opened = rn.x == P.stamp_open, nb_closed = rn.x == closed_stamp;
          const int what = gp_file(nb_closed, opened, __uint_as_float(rn.y), __uint_as_float(rn.z), new_g, new_f);   // :295-306
          if (what) rec[nb] = gp_record(P.stamp_open, new_g, new_f, cur);
          file = what == 2;
          key = gp_key(new_f, nb);
        }
      }
      const uint32_t at = wave_append(file, &s_count);
      if (file) {
        if (at < P.max_open) keys[at] = key;
        else s_full = 1;
      }
      __syncthreads();                                                               // the 256 slots are free for the next round
    }
    n_pushed += s_count - held;
    if (s_full) { status = kGpOpenFull; break; }
    if (tid == 0) rec[cur].x = closed_stamp;                                         // :312 (read again only behind the next pop's barrier)
    ++n_expanded;
    if (cur == goal) { status = kGpFound; break; }                                   // :315
  }
  // ---- the counters, then the path (:316-322) by one lane ----
  if (c_lethal) atomicAdd(&s_ctr[0], c_lethal);
  if (c_tested) atomicAdd(&s_ctr[1], c_tested);
  if (c_blocked) atomicAdd(&s_ctr[2], c_blocked);
  if (c_capped) atomicAdd(&s_ctr[3], c_capped);
  __syncthreads();
  if (tid == 0) {
    dddmr_global_plan_cloud_result out;
    out.plan.status = status;
    out.plan.path_offset = 0;
    out.plan.path_len = 0;
    out.plan.n_expanded = n_expanded;
    out.plan.n_pushed = n_pushed;
    out.plan.n_discarded_closed = n_discarded;
    out.plan.g_goal = 0.f;
    out.plan.host_waits = 0;
    out.n_knn_fallbacks = n_knn;
    out.n_lethal_skipped = s_ctr[0];
    out.n_los_tested = s_ctr[1];
    out.n_los_blocked = s_ctr[2];
    out.n_los_capped = s_ctr[3];
    out.max_successors = max_succ;
    if (status == kGpFound) {
      uint32_t len = 1, at = goal;
      for (uint32_t step = 0; step < n_expanded; ++step) {                           // (a chain of closed nodes' parents)
        const uint32_t p = rec[at].w;
        if (p == at || p >= A.n) break;
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
        out.plan.path_len = len;
      }
      out.plan.g_goal = __uint_as_float(rec[goal].y);
    }
    res_all[qi] = out;
    __threadfence_system();
  }
}

}  // namespace dddmr

// ---- host (included by rollout_engine.hip after global_plan.hip.h) ----------------------------------------------------
namespace {

struct GpcOut {                              // host-mapped; seq is stored last, by k_gp_finish
  dddmr_global_plan_cloud_result res[DDDMR_GLOBAL_PLAN_MAX_QUERIES];
  uint32_t seq;
};

// What the cloud search keeps beside GlobalPlanState: it belongs to the context, is made by the first of its three entries
// and outlives a global_plan_create unless the planner's node capacity changes (both arrays are then dropped).
struct GpCloudState {
  uint32_t max_nodes = 0;                    // the planner's max_nodes when this was made
  float* node_weights = nullptr;             // [max_nodes] sGraph's node weights
  uint32_t weights_n = 0, weights_epoch = 0; // as GlobalPlanState's intensity: valid for one ground
  GridBuf extra;                             // the host layers' lethal points
  float4* extra_pts = nullptr;               // [max_nodes]
  uint2* extra_slot = nullptr;               // [max_nodes] grid builder
  GpcOut *out_host = nullptr, *out_dev = nullptr;
  uint32_t seq = 0;
  Owned mem;
};
static_assert(!std::is_copy_constructible_v<GpCloudState>);
static_assert(sizeof(dddmr_global_plan_cloud_result) == 56, "the ctypes mirror (_capi.py) pins this size");
static_assert(kGpRowFull == DDDMR_GLOBAL_PLAN_ROW_FULL && kGpCloudMaxSuccessors == DDDMR_GLOBAL_PLAN_CLOUD_MAX_SUCCESSORS &&
              kGpLosMaxSamples == DDDMR_GLOBAL_PLAN_LOS_MAX_SAMPLES, "the header's constants are the kernel's");

// the cloud state sized for planner p; tick_mu held, the device current
int global_plan_cloud_state(dddmr_rollout_ctx* ctx, const char* what, const GlobalPlanState* p, GpCloudState** c_out) {
  if (ctx->gcloud && ctx->gcloud->max_nodes == p->max_nodes) {
    *c_out = ctx->gcloud.get();
    return DDDMR_OK;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  auto c = std::make_unique<GpCloudState>();
  c->max_nodes = p->max_nodes;
  const size_t N = std::max<size_t>(p->max_nodes, 1);
  HIPCHK(ctx, dev_alloc_zeroed(c->mem.dev, &c->node_weights, N));
  HIPCHK(ctx, dev_alloc(c->mem.dev, &c->extra_pts, N));
  HIPCHK(ctx, dev_alloc(c->mem.dev, &c->extra_slot, N));
  if (grid_alloc(c->mem.dev, c->extra, kSlCells, (uint32_t)N) != 0) return fail(ctx, DDDMR_ERR_HIP, "%s: grid storage", what);
  if (host_mapped_alloc(c->mem.host, &c->out_host, &c->out_dev, sizeof(GpcOut)) != 0) return fail(ctx, DDDMR_ERR_HIP, "%s: pinned results", what);
  std::memset(c->out_host, 0, sizeof(GpcOut));
  ctx->gcloud.reset(c.release());
  *c_out = ctx->gcloud.get();
  return DDDMR_OK;
}

}  // namespace

extern "C" {

int dddmr_rollout_global_plan_set_graph_node_weights(dddmr_rollout_ctx* ctx, const float* weights, size_t n) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "global_plan_set_graph_node_weights";
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
  GpCloudState* c = nullptr;
  if (const int rc = global_plan_cloud_state(ctx, what, p, &c)) return rc;
  if (n) HIPCHK(ctx, hipMemcpy(c->node_weights, weights, n * sizeof(float), hipMemcpyHostToDevice));
  c->weights_n = (uint32_t)n;                                // (0: back to all zero)
  c->weights_epoch = m->ground_epoch;
  return DDDMR_OK;
}

int dddmr_rollout_global_plan_set_lethal_points(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "global_plan_set_lethal_points";
  if (!cloud_arg_ok(xyz, n, stride_bytes)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a bad cloud pointer / stride", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  GlobalPlanState* p = nullptr;
  StaticLayerState* m = nullptr;
  if (const int rc = global_plan_state(ctx, what, false, &p, &m, nullptr)) return rc;
  if (n > m->cfg.max_ground_points) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu points, the static layer's max_ground_points %u", what, n, m->cfg.max_ground_points);
  const HostCloud pts(xyz, n, n ? stride_bytes : 12);
  if (!pts.finite) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a coordinate is not finite", what);
  if (!cloud_box_ok(pts.lo, pts.hi))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a coordinate is beyond 1e6 m, or the cloud is wider than %g m on an axis", what, (double)kCloudMaxExtent);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GpCloudState* c = nullptr;
  if (const int rc = global_plan_cloud_state(ctx, what, p, &c)) return rc;
  c->extra.g.n = 0;                                          // (a failure below leaves no cloud behind)
  if (!n) return DDDMR_OK;
  hipStream_t st = ctx->stream;
  Drain drain{st};
  // cells as wide as the line of sight's ball (2 * inscribed_radius), like the zones' grid
  const float cell = sl_zone_cell(2.0 * p->cfg.inscribed_radius);
  PointGrid g = c->extra.g;
  grid_shape(g, pts.lo, pts.hi, cell, cell, c->extra.cap_cells);
  c->extra.g = g;
  HIPCHK(ctx, hipMemcpyAsync(c->extra_pts, pts.pts.data(), n * sizeof(float4), hipMemcpyHostToDevice, st));
  if (const int rc = grid_build(ctx, m->temp, m->temp_bytes, c->extra, c->extra_pts, (uint32_t)n, c->extra_slot, st)) {
    c->extra.g.n = 0;
    return rc;
  }
  const hipError_t e = hipStreamSynchronize(st);             // (pts is this call's: the copy has to be over)
  if (e != hipSuccess) {
    c->extra.g.n = 0;
    HIPCHK(ctx, e);
  }
  drain.armed = false;
  return DDDMR_OK;
}

int dddmr_rollout_global_plan_plan_on_cloud(dddmr_rollout_ctx* ctx, const uint32_t* start_id, const uint32_t* goal_id, size_t n_queries,
                                            uint32_t* path_out, size_t path_capacity, dddmr_global_plan_cloud_result* results) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "global_plan_plan_on_cloud";
  if (!start_id || !goal_id || !results || n_queries == 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument or no query", what);
  if (path_capacity && !path_out) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null path_out", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  GlobalPlanState* p = nullptr;
  StaticLayerState* m = nullptr;
  const double* dgraph = nullptr;
  if (const int rc = global_plan_state(ctx, what, false, &p, &m, &dgraph)) return rc;
  // isLineOfSightClear's dt is 0 for inscribed_radius 0 and its loop does not end (:180-181): refused here, and with it
  // radii the search boxes are not made for
  if (!(p->cfg.inscribed_radius > 0.0) || p->cfg.inscribed_radius > kSlMaxRadius || !(p->cfg.a_star_expanding_radius >= 0.0) ||
      p->cfg.a_star_expanding_radius > kSlMaxRadius)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: inscribed_radius %g (above 0, at most %g), a_star_expanding_radius %g (0 .. %g)", what, p->cfg.inscribed_radius,
                kSlMaxRadius, p->cfg.a_star_expanding_radius, kSlMaxRadius);
  if (n_queries > p->cfg.max_queries) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu queries, max_queries %u", what, n_queries, p->cfg.max_queries);
  const SlGeneration& g = m->gen[m->cur];
  // nearestKSearch resizes its result to 8 and the caller walks entries the search never filled: refused
  if (g.n_ground < kGpCloudKnn) return fail(ctx, DDDMR_ERR_STATE, "%s: the ground has %u nodes, the search needs %u", what, g.n_ground, kGpCloudKnn);
  GpQueries Q{};
  for (size_t i = 0; i < n_queries; ++i) {
    if (start_id[i] >= g.n_ground || goal_id[i] >= g.n_ground)
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: query %zu names node %u / %u of %u", what, i, start_id[i], goal_id[i], g.n_ground);
    Q.start[i] = start_id[i];
    Q.goal[i] = goal_id[i];
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  GpCloudState* c = nullptr;
  if (const int rc = global_plan_cloud_state(ctx, what, p, &c)) return rc;
  hipStream_t st = ctx->stream;
  Drain drain{st};
  if (p->serial >= 0x7FFFFFF0u) {                            // the stamps would wrap: the records start over
    HIPCHK(ctx, hipMemsetAsync(p->rec, 0, (size_t)p->cfg.max_queries * p->max_nodes * sizeof(uint4), st));
    p->serial = 0;
  }
  ++p->serial;                                               // one serial for both searches: neither sees the other's records
  if (p->weights_n && (p->weights_epoch != m->ground_epoch || p->weights_n != g.n_ground)) p->weights_n = 0;   // another ground: dropped
  if (c->weights_n && (c->weights_epoch != m->ground_epoch || c->weights_n != g.n_ground)) c->weights_n = 0;
  GpcArgs A{};
  A.ground = m->ground.g;
  A.extra = c->extra.g;
  A.pts = g.ground_pts;
  A.dgraph = dgraph;
  A.mask = p->cfg.dgraph_source == 0 ? ctx->stack->mask_pub : nullptr;   // (global_plan_state has checked the stack)
  A.intensity = p->weights_n ? p->weights : nullptr;
  A.node_weight = c->weights_n ? c->node_weights : nullptr;
  A.n = g.n_ground;
  A.r_box = (float)p->cfg.a_star_expanding_radius + kSlPad;
  A.r2 = gp_cloud_radius2(p->cfg.a_star_expanding_radius);
  A.los_box = (float)(2.0 * p->cfg.inscribed_radius) + kSlPad;
  A.los_r2 = gp_cloud_radius2(2.0 * p->cfg.inscribed_radius);
  GpParams P{};
  P.turning_weight = p->cfg.turning_weight; P.expanding_radius = p->cfg.a_star_expanding_radius;
  P.inscribed_radius = p->cfg.inscribed_radius; P.rate = p->cfg.inflation_descending_rate;
  P.max_open = p->cfg.max_open_entries; P.max_expansions = p->cfg.max_expansions; P.path_stride = p->max_nodes;
  P.stamp_open = 2u * p->serial;
  hipLaunchKernelGGL(k_gp_plan_cloud, dim3((uint32_t)n_queries), dim3(kGpThreads), 0, st, A, P, Q, p->rec, (size_t)p->max_nodes, p->keys, p->path_dev, c->out_dev->res);
  const uint32_t seq = next_seq(c->seq);
  hipLaunchKernelGGL(k_gp_finish, dim3(1), dim3(64), 0, st, &c->out_dev->seq, seq);
  uint32_t waits = 0;
  if (const int rc = feed_wait(st, &c->out_host->seq, seq, &waits)) return fail(ctx, DDDMR_ERR_HIP, "%s: launch or wait failed (%d)", what, rc);
  drain.armed = false;
  size_t at = 0;
  bool full = false, row_full = false, fits = true;
  for (size_t i = 0; i < n_queries; ++i) {
    dddmr_global_plan_cloud_result r = c->out_host->res[i];
    full = full || r.plan.status == DDDMR_GLOBAL_PLAN_OPEN_FULL;
    row_full = row_full || r.plan.status == DDDMR_GLOBAL_PLAN_ROW_FULL;
    r.plan.path_offset = (uint32_t)at;
    r.plan.host_waits = waits;
    if (fits && at + r.plan.path_len <= path_capacity) {
      if (r.plan.path_len) std::memcpy(path_out + at, p->path_host + i * (size_t)p->max_nodes, (size_t)r.plan.path_len * sizeof(uint32_t));
    } else {
      fits = false;
    }
    at += r.plan.path_len;
    results[i] = r;
  }
  if (full) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: a query's frontier outgrew max_open_entries %u", what, p->cfg.max_open_entries);
  if (row_full) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: a radius search found more than %u successors", what, kGpCloudMaxSuccessors);
  if (!fits) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: the paths hold %zu nodes, path_capacity %zu", what, at, path_capacity);
  return DDDMR_OK;
}

}  // extern "C"
