// mcl_observation.hip.h -- the localiser's observation on the device: what MCL3dlNode::cbLeGoFeatureCloud
// (dddmr_mcl_3dl/src/mcl_3dl.cpp:263-464) makes of one sweep's flat and less-sharp feature lists before measure() sees
// them:
//   pcl::transformPointCloud x 2            :295-296   a second rounding to float after the feature emitter's T_out
//   VoxelGrid, leaf (1.0f, 1.0f, 0.1f)      :306-309   flat: oracle/ASSUMPTIONS.md rows 7-8 with a per-axis inverse leaf
//   NormalEstimation, setKSearch(5)         :320-329   less sharp: DESIGN 4e lists what is recalled of PCL 1.15
//   the two sums and the dominance rule     :340-360   one lane, index order, double
//   the dominant branch's weights           :362-403
//   EuclideanClusterExtraction + weights    :404-443   rows 9-10; a cluster below the minimum is dropped WITH its points
//
// At most 2000 points: one workgroup stages them in LDS once and answers everything by brute force over all pairs -- the
// flat points' voxel order by counting, the 5 nearest by a per-lane insertion of (d2, index), the clusters by a
// lock-free union-find whose root is the lowest index.  The order of the kept clusters is libstdc++'s std::sort over
// their sizes, which only the host can replay (mcl_observation_plan.hip.h): k_mclobs_prepare hands it the sizes with the
// stats, the host waits once, sorts, and k_mclobs_pack writes the less-sharp output.  In a dominant branch the first
// kernel writes the output itself.  2 launches at most and 1 host wait per prepare; no memset.
//
// The result has k_mcl_match's layout (x y z w, the flat points first with w = 1) and stays in device memory:
// dddmr_rollout_mcl_measure_prepared runs the measure's three kernels on it.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "dev_memory.hip.h"        // Owned, dev_alloc, Drain
#include "mcl_measure.hip.h"       // MclState, mcl_run: the prepared observation is measured there
#include "mcl_normal.hip.h"
#include "mcl_observation_plan.hip.h"
#include "point_grid_plan.hip.h"   // cloud_arg_ok
#include "sensor_sources.hip.h"    // sweep_features_of: the features of a sweep source, on the device
#include "wave_ops.hip.h"          // block_excl_scan

#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kMclObsThreads = 1024;
static_assert(kMclObsThreads % 64 == 0, "whole waves: the scans run the wave primitives");
static_assert(kMclMaxObs <= 2 * kMclObsThreads, "two elements per lane in the scans and the root pass");
constexpr uint32_t kMclObsNone = 0xFFFFFFFFu;

struct MclObsParams {
  double R[9], t[3];             // trans_b2s_af3
  float inv_leaf[3];             // 1 / leaf per axis, in float
  float tol2;                    // static_cast<float>(tol * tol)
  int32_t min_size;
  uint32_t n_flat, n_ls;
  uint32_t seq;
};

struct MclObsResult {            // host-mapped; seq is stored last
  double sum_x, sum_y;
  uint32_t n_flat_out, n_ls_out, branch, n_kept, n_small, n_nan;
  uint32_t seq;
};

// exclusive scan of a[0 .. n) in place, n <= 2 * kMclObsThreads; every lane of the workgroup calls it; returns the total
__device__ inline uint32_t mclobs_scan(uint32_t* a, uint32_t n, uint32_t* s_w) {
  const uint32_t i0 = 2 * threadIdx.x, i1 = i0 + 1;
  const uint32_t v0 = i0 < n ? a[i0] : 0u, v1 = i1 < n ? a[i1] : 0u;
  uint32_t total;
  const uint32_t base = block_excl_scan<kMclObsThreads / 64>(v0 + v1, s_w, &total);   // (ends with a barrier: a[] has been read)
  if (i0 < n) a[i0] = base;
  if (i1 < n) a[i1] = base + v0;
  __syncthreads();
  return total;
}

// find with path halving: a node that has a parent other than itself is never a root again and its ancestors only get
// smaller, so pointing it at its grandparent is safe beside the hooks (which only ever CAS a root)
__device__ __forceinline__ uint32_t mclobs_find(uint32_t* parent, uint32_t i) {
  uint32_t p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (p != i) {
    const uint32_t g = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (g != p) __hip_atomic_store(&parent[i], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    i = p;
    p = g;
  }
  return i;
}
// the larger root is hooked under the smaller one (marking_fused.hip.h's cc_union_pair): whatever the interleaving,
// the components are those of the graph and a component's root is its lowest index
__device__ __forceinline__ void mclobs_union(uint32_t* parent, uint32_t i, uint32_t j) {
  uint32_t u = mclobs_find(parent, i), v = mclobs_find(parent, j);
  while (u != v) {
    if (u < v) { const uint32_t t = u; u = v; v = t; }
    const uint32_t old = atomicCAS(&parent[u], u, v);
    if (old == u) break;
    u = mclobs_find(parent, old);
    v = mclobs_find(parent, v);
  }
}

// Everything of one prepare but the order of the clusters.  One workgroup of kMclObsThreads lanes.
//   flat_in, ls_in   x y z (w is ignored): the host's staging, or a sweep source's feature lists where they lie
//   obs_out          [n_flat_out] flat x y z 1, then -- in a dominant branch -- the less-sharp x y z intensity
//   normals_out      [n_ls] normal x y z, input order
//   pts_out          [n_ls] the transformed less-sharp points              | cluster branch: what k_mclobs_pack reads
//   slot_rank        [n_ls] (kept cluster in creation order or none, rank inside it) |
//   kept_size        [n_kept] host-mapped: the kept clusters' sizes in creation order
__global__ __launch_bounds__(kMclObsThreads) void k_mclobs_prepare(MclObsParams k, const float4* __restrict__ flat_in,
                                                                   const float4* __restrict__ ls_in, float4* __restrict__ obs_out,
                                                                   float4* __restrict__ normals_out, float4* __restrict__ pts_out,
                                                                   uint2* __restrict__ slot_rank, uint32_t* __restrict__ kept_size,
                                                                   MclObsResult* __restrict__ res) {
  // 64 000 bytes of the arrays below: under the 64 KiB a workgroup gets without asking for more
  __shared__ float4 s_p[kMclMaxObs];                     // flat [0, n_flat), less sharp after them
  __shared__ unsigned long long s_key[kMclMaxObs];       // flat: voxel index; less sharp: normal x, y, then (clusters) s_c
  __shared__ uint32_t s_a[kMclMaxObs];                   // flat: point by rank; less sharp: union-find parent
  __shared__ uint32_t s_b[kMclMaxObs];                   // flat: first of its voxel, scanned; less sharp: cluster size
  __shared__ uint32_t s_w[kMclObsThreads / 64];
  __shared__ int s_lo[3], s_hi[3];
  __shared__ double s_sum[2];
  __shared__ uint32_t s_cnt[4];                          // branch, NaN normals, kept points, small clusters
  const uint32_t t = threadIdx.x, T = kMclObsThreads;
  const uint32_t nf = min(k.n_flat, kMclMaxObs), nl = min(k.n_ls, kMclMaxObs - nf);

  for (uint32_t i = t; i < nf + nl; i += T) {
    const float4 q = i < nf ? flat_in[i] : ls_in[i - nf];
    const float3 g = affine_to_float(k.R, k.t, q.x, q.y, q.z);
    s_p[i] = make_float4(g.x, g.y, g.z, 0.f);
  }
  if (t < 3) { s_lo[t] = INT_MAX; s_hi[t] = INT_MIN; }
  if (t < 4) s_cnt[t] = 0;
  __syncthreads();

  // ---- flat: VoxelGrid ------------------------------------------------------------------------------------------
  for (uint32_t i = t; i < nf; i += T) {
    const float4 p = s_p[i];
    const int v[3] = {(int)floorf(p.x * k.inv_leaf[0]), (int)floorf(p.y * k.inv_leaf[1]), (int)floorf(p.z * k.inv_leaf[2])};
    for (int a = 0; a < 3; ++a) { atomicMin(&s_lo[a], v[a]); atomicMax(&s_hi[a], v[a]); }
  }
  __syncthreads();
  if (nf) {
    const long long lo0 = s_lo[0], lo1 = s_lo[1], lo2 = s_lo[2];
    const unsigned long long dx = (unsigned long long)(s_hi[0] - lo0 + 1), dy = (unsigned long long)(s_hi[1] - lo1 + 1);
    for (uint32_t i = t; i < nf; i += T) {
      const float4 p = s_p[i];
      const unsigned long long i0 = (unsigned long long)((long long)floorf(p.x * k.inv_leaf[0]) - lo0);
      const unsigned long long i1 = (unsigned long long)((long long)floorf(p.y * k.inv_leaf[1]) - lo1);
      const unsigned long long i2 = (unsigned long long)((long long)floorf(p.z * k.inv_leaf[2]) - lo2);
      s_key[i] = i0 + i1 * dx + i2 * dx * dy;
    }
  }
  __syncthreads();
  for (uint32_t i = t; i < nf; i += T) {                 // rank by (voxel, input index)
    const unsigned long long ki = s_key[i];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < nf; ++j) {
      const unsigned long long kj = s_key[j];
      rank += (kj < ki || (kj == ki && j < i)) ? 1u : 0u;
    }
    s_a[rank] = i;
  }
  __syncthreads();
  for (uint32_t r = t; r < nf; r += T) s_b[r] = (r == 0 || s_key[s_a[r]] != s_key[s_a[r - 1]]) ? 1u : 0u;
  __syncthreads();
  const uint32_t n_flat_out = mclobs_scan(s_b, nf, s_w);
  for (uint32_t r = t; r < nf; r += T) {
    const unsigned long long key = s_key[s_a[r]];
    if (r != 0 && s_key[s_a[r - 1]] == key) continue;
    float sx = 0.f, sy = 0.f, sz = 0.f;                  // CentroidPoint: float running sums in input order
    uint32_t q = r;
    for (; q < nf && s_key[s_a[q]] == key; ++q) {
      const float4 p = s_p[s_a[q]];
      sx += p.x; sy += p.y; sz += p.z;
    }
    const float c = (float)(q - r);
    obs_out[s_b[r]] = make_float4(sx / c, sy / c, sz / c, 1.0f);
  }
  __syncthreads();

  // ---- less sharp: 5 nearest, normal -------------------------------------------------------------------------------
  const float4* P = s_p + nf;
  float2* s_nxy = reinterpret_cast<float2*>(s_key);
  const uint32_t kn = min(nl, 5u);
  for (uint32_t i = t; i < nl; i += T) {
    const float4 p = P[i];
    const float inf = __int_as_float(0x7F800000);
    float b0 = inf, b1 = inf, b2 = inf, b3 = inf, b4 = inf;
    uint32_t i0 = kMclObsNone, i1 = kMclObsNone, i2 = kMclObsNone, i3 = kMclObsNone, i4 = kMclObsNone;
#pragma unroll 4
    for (uint32_t j = 0; j < nl; ++j) {                  // ascending j and strict <: ties keep the lower index first
      const float4 g = P[j];
      const float d = l2_simple(g.x, g.y, g.z, p.x, p.y, p.z);
      if (d < b4) {
        b4 = d; i4 = j;
        if (b4 < b3) { const float f = b3; b3 = b4; b4 = f; const uint32_t u = i3; i3 = i4; i4 = u; }
        if (b3 < b2) { const float f = b2; b2 = b3; b3 = f; const uint32_t u = i2; i2 = i3; i3 = u; }
        if (b2 < b1) { const float f = b1; b1 = b2; b2 = f; const uint32_t u = i1; i1 = i2; i2 = u; }
        if (b1 < b0) { const float f = b0; b0 = b1; b1 = f; const uint32_t u = i0; i0 = i1; i1 = u; }
      }
    }
    const uint32_t nb[5] = {i0, i1, i2, i3, i4};
    uint32_t have = 0;
    for (uint32_t q = 0; q < kn; ++q) have += nb[q] != kMclObsNone ? 1u : 0u;
    // (a neighbour slot stays empty only when distances are not finite: such a point gets a NaN normal)
    const float3 nrm = mclobs_normal(P, nb, have == kn ? kn : 0u, p);
    normals_out[i] = make_float4(nrm.x, nrm.y, nrm.z, 0.f);
    s_nxy[i] = make_float2(nrm.x, nrm.y);
  }
  __syncthreads();
  if (t == 0) {                                          // :340-360, index order
    double sum_y = 0, sum_x = 0;
    uint32_t n_nan = 0;
    const float nan = __int_as_float(0x7FC00000);
    for (uint32_t i0 = 0; i0 < nl; i0 += 8) {              // eight loads in flight, then the adds in index order
      float2 n[8];
#pragma unroll
      for (uint32_t q = 0; q < 8; ++q) n[q] = i0 + q < nl ? s_nxy[i0 + q] : make_float2(nan, nan);
#pragma unroll
      for (uint32_t q = 0; q < 8; ++q) {
        if (!(n[q].y != n[q].y)) sum_y += (double)fabsf(n[q].y);
        if (!(n[q].x != n[q].x)) sum_x += (double)fabsf(n[q].x);
        n_nan += (i0 + q < nl && n[q].x != n[q].x) ? 1u : 0u;
      }
    }
    s_sum[0] = sum_x; s_sum[1] = sum_y;
    s_cnt[0] = mclobs_branch(sum_x, sum_y);
    s_cnt[1] = n_nan;
  }
  __syncthreads();
  const uint32_t branch = s_cnt[0];
  const double sum_x = s_sum[0], sum_y = s_sum[1];
  uint32_t n_ls_out = 0, n_kept = 0;

  if (branch != kMclObsClusters) {
    // ---- dominant: every point, input order ----------------------------------------------------------------------
    for (uint32_t i = t; i < nl; i += T) {
      const float4 p = P[i];
      const float2 n = s_nxy[i];
      obs_out[n_flat_out + i] = make_float4(p.x, p.y, p.z, mclobs_dominant_intensity(branch, n.x, n.y, sum_x, sum_y));
    }
    n_ls_out = nl;
  } else {
    // ---- clusters ------------------------------------------------------------------------------------------------
    uint32_t* parent = s_a;
    uint32_t* csize = s_b;
    uint32_t* s_c = reinterpret_cast<uint32_t*>(s_key);  // kept root flag, scanned (the normals are not read any more)
    for (uint32_t i = t; i < nl; i += T) { parent[i] = i; csize[i] = 0; }
    __syncthreads();
    for (uint32_t i = t; i < nl; i += T) {
      const float4 p = P[i];
#pragma unroll 4
      for (uint32_t j = (i & ~63u) + 1; j < nl; ++j) {   // (a wave's lanes read the same P[j])
        const float4 g = P[j];
        if (j > i && l2_simple(g.x, g.y, g.z, p.x, p.y, p.z) < k.tol2) mclobs_union(parent, i, j);
      }
    }
    __syncthreads();
    uint32_t root[2] = {0, 0};
    for (uint32_t i = t, q = 0; i < nl; i += T, ++q) root[q] = mclobs_find(parent, i);
    __syncthreads();
    for (uint32_t i = t, q = 0; i < nl; i += T, ++q) {
      parent[i] = root[q];
      atomicAdd(&csize[root[q]], 1u);
    }
    __syncthreads();
    for (uint32_t i = t; i < nl; i += T) {
      const bool kept = parent[i] == i && (int64_t)csize[i] >= (int64_t)k.min_size;
      s_c[i] = kept ? 1u : 0u;
      if (kept) {
        atomicAdd(&s_cnt[2], csize[i]);
        if ((int64_t)csize[i] < (int64_t)k.min_size + 1) atomicAdd(&s_cnt[3], 1u);
      }
    }
    __syncthreads();
    n_kept = mclobs_scan(s_c, nl, s_w);
    for (uint32_t i = t; i < nl; i += T) {
      const uint32_t r = parent[i];
      const bool kept = (int64_t)csize[r] >= (int64_t)k.min_size;
      if (kept && r == i) kept_size[s_c[i]] = csize[i];
      uint32_t rank = 0;
#pragma unroll 8
      for (uint32_t j = r; j < i; ++j) rank += parent[j] == r ? 1u : 0u;     // (the root is the lowest member)
      slot_rank[i] = make_uint2(kept ? s_c[r] : kMclObsNone, rank);
      const float4 p = P[i];
      pts_out[i] = make_float4(p.x, p.y, p.z, 0.f);
    }
    n_ls_out = s_cnt[2];
  }
  __syncthreads();
  if (t == 0) {
    res->sum_x = sum_x; res->sum_y = sum_y;
    res->n_flat_out = n_flat_out; res->n_ls_out = n_ls_out; res->branch = branch;
    res->n_kept = n_kept; res->n_small = s_cnt[3]; res->n_nan = s_cnt[1];
    __threadfence_system();
    __hip_atomic_store(&res->seq, k.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// The cluster branch's output once the host has ordered the kept clusters.
//   plan  [n_kept] host-mapped, by kept cluster in creation order: (first output index, intensity bits)
__global__ __launch_bounds__(256) void k_mclobs_pack(uint32_t n_ls, uint32_t n_ls_out, const float4* __restrict__ pts,
                                                     const uint2* __restrict__ slot_rank, const uint2* __restrict__ plan,
                                                     float4* __restrict__ ls_out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_ls) return;
  const uint2 sr = slot_rank[i];
  if (sr.x == kMclObsNone) return;
  const uint2 pl = plan[sr.x];
  const uint32_t o = pl.x + sr.y;
  if (o >= n_ls_out) return;
  const float4 p = pts[i];
  ls_out[o] = make_float4(p.x, p.y, p.z, __uint_as_float(pl.y));
}

}  // namespace dddmr

// ---- host (included by rollout_engine.hip after the context) ---------------------------------------------------------
namespace {

struct MclObs {
  dddmr_mcl_observation_config cfg{};
  uint32_t cap = 0;                         // max_flat_points + max_less_sharp_points
  float4* obs[2] = {nullptr, nullptr};      // [cap] the prepared observation, k_mcl_match's layout
  float4* normals[2] = {nullptr, nullptr};  // [max_less_sharp_points]
  uint32_t n_flat[2] = {0, 0}, n_ls[2] = {0, 0}, n_ls_in[2] = {0, 0};
  int cur = 0;                              // obs[cur] answers the getter and the measure
  float4* pts = nullptr;
  uint2* slot_rank = nullptr;
  Owned mem;
  // host-mapped: the host entry's input, the kept clusters' sizes, their plan, the result
  float4 *in_host = nullptr, *in_dev = nullptr;
  uint32_t *kept_host = nullptr, *kept_dev = nullptr;
  uint2 *plan_host = nullptr, *plan_dev = nullptr;
  MclObsResult *res_host = nullptr, *res_dev = nullptr;
  uint32_t seq = 0;
};

static_assert(!std::is_copy_constructible_v<MclObs>);

int mclobs_alloc(dddmr_rollout_ctx* ctx, MclObs* o) {
  const size_t cap = std::max<uint32_t>(o->cap, 1), nl = std::max<uint32_t>(o->cfg.max_less_sharp_points, 1);
  for (int b = 0; b < 2; ++b) {
    HIPCHK(ctx, dev_alloc(o->mem.dev, &o->obs[b], cap));
    HIPCHK(ctx, dev_alloc(o->mem.dev, &o->normals[b], nl));
  }
  HIPCHK(ctx, dev_alloc(o->mem.dev, &o->pts, nl));
  HIPCHK(ctx, dev_alloc(o->mem.dev, &o->slot_rank, nl));
  if (host_mapped_alloc(o->mem.host, &o->in_host, &o->in_dev, cap * sizeof(float4)) != 0 ||
      host_mapped_alloc(o->mem.host, &o->kept_host, &o->kept_dev, nl * sizeof(uint32_t)) != 0 ||
      host_mapped_alloc(o->mem.host, &o->plan_host, &o->plan_dev, nl * sizeof(uint2)) != 0 ||
      host_mapped_alloc(o->mem.host, &o->res_host, &o->res_dev, sizeof(MclObsResult)) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "mcl_set_observation_config: host-mapped staging");
  std::memset(o->res_host, 0, sizeof(MclObsResult));
  return DDDMR_OK;
}

// The launches and the one wait of a prepare; flat_dev / ls_dev are device-readable.  tick_mu held.
int mclobs_run(dddmr_rollout_ctx* ctx, const char* what, MclObs* o, const float4* flat_dev, uint32_t n_flat, const float4* ls_dev,
               uint32_t n_ls, const double T_b2s[12], dddmr_mcl_observation_stats* stats) {
  MclObsParams k{};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) k.R[3 * r + c] = T_b2s[4 * r + c];
    k.t[r] = T_b2s[4 * r + 3];
  }
  k.inv_leaf[0] = 1.0f / 1.0f; k.inv_leaf[1] = 1.0f / 1.0f; k.inv_leaf[2] = 1.0f / 0.1f;     // setLeafSize(1.0f, 1.0f, 0.1f)
  k.tol2 = static_cast<float>(o->cfg.euc_cluster_distance * o->cfg.euc_cluster_distance);
  k.min_size = o->cfg.euc_cluster_min_size;
  k.n_flat = n_flat;
  k.n_ls = n_ls;
  k.seq = next_seq(o->seq);
  const int b = o->cur ^ 1;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(k_mclobs_prepare, dim3(1), dim3(kMclObsThreads), 0, st, k, flat_dev, ls_dev, o->obs[b], o->normals[b], o->pts, o->slot_rank,
                     o->kept_dev, o->res_dev);
  uint32_t launches = 1, waits = 0;
  if (const int rc = feed_wait(st, &o->res_host->seq, k.seq, &waits)) return fail(ctx, DDDMR_ERR_HIP, "%s: launch or wait failed (%d)", what, rc);
  const MclObsResult r = *o->res_host;
  if (r.n_flat_out > n_flat || r.n_ls_out > n_ls || r.n_kept > n_ls) return fail(ctx, DDDMR_ERR_HIP, "%s: inconsistent counts from the device", what);
  if (r.branch == kMclObsClusters && r.n_kept) {
    std::vector<uint32_t> order;
    mclobs_order_clusters(o->kept_host, r.n_kept, order);
    uint32_t at = 0;
    for (uint32_t q = 0; q < r.n_kept; ++q) {
      const uint32_t c = order[q], size = o->kept_host[c];
      const float w = mclobs_cluster_intensity(size, n_ls, k.min_size);
      uint32_t bits;
      std::memcpy(&bits, &w, 4);
      o->plan_host[c] = make_uint2(at, bits);
      at += size;
    }
    if (at != r.n_ls_out) return fail(ctx, DDDMR_ERR_HIP, "%s: the kept clusters hold %u points, the device counted %u", what, at, r.n_ls_out);
    Drain drain{st};                                     // (the prepare does not wait for this launch; an error exit does)
    hipLaunchKernelGGL(k_mclobs_pack, dim3((n_ls + 255) / 256), dim3(256), 0, st, n_ls, r.n_ls_out, o->pts, o->slot_rank, o->plan_dev,
                       o->obs[b] + r.n_flat_out);
    HIPCHK(ctx, hipGetLastError());
    drain.armed = false;
    ++launches;
  }
  o->n_flat[b] = r.n_flat_out;
  o->n_ls[b] = r.n_ls_out;
  o->n_ls_in[b] = n_ls;
  o->cur = b;
  if (stats) {
    stats->n_flat_in = n_flat; stats->n_flat_out = r.n_flat_out;
    stats->n_less_sharp_in = n_ls; stats->n_less_sharp_out = r.n_ls_out;
    stats->branch = r.branch;
    stats->n_clusters = r.n_kept; stats->n_small_clusters = r.n_small; stats->n_nan_normals = r.n_nan;
    stats->sum_normal_x = r.sum_x; stats->sum_normal_y = r.sum_y;
    stats->launches = launches; stats->host_waits = waits;
  }
  return DDDMR_OK;
}

// the checks every observation entry starts with; tick_mu held
int mclobs_state(dddmr_rollout_ctx* ctx, const char* what, bool need_config, MclState** out) {
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  MclState* s = ctx->mcl.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_create", what);
  if (need_config && !s->obs) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_set_observation_config", what);
  *out = s;
  return DDDMR_OK;
}

}  // namespace

extern "C" {

int dddmr_rollout_mcl_set_observation_config(dddmr_rollout_ctx* ctx, const dddmr_mcl_observation_config* cfg) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_set_observation_config";
  if (cfg) {
    if (!std::isfinite(cfg->euc_cluster_distance) || !(cfg->euc_cluster_distance > 0) || !((float)cfg->euc_cluster_distance > 0.f))
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: euc_cluster_distance %g must be positive and finite", what, cfg->euc_cluster_distance);
    if (cfg->euc_cluster_min_size < 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: negative euc_cluster_min_size", what);
    if (cfg->flags != 0 || cfg->reserved != 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: flags %#x, reserved %#x", what, cfg->flags, cfg->reserved);
  }
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  if (const int rc = mclobs_state(ctx, what, false, &s)) return rc;
  if (cfg && (uint64_t)cfg->max_flat_points + cfg->max_less_sharp_points > s->cfg.max_observation_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %u flat + %u less-sharp points, mcl_create's max_observation_points is %u", what, cfg->max_flat_points,
                cfg->max_less_sharp_points, s->cfg.max_observation_points);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (!cfg) {
    s->obs.reset();
    return DDDMR_OK;
  }
  auto o = std::make_unique<MclObs>();
  o->cfg = *cfg;
  o->cap = cfg->max_flat_points + cfg->max_less_sharp_points;
  const int rc = mclobs_alloc(ctx, o.get());
  if (rc == DDDMR_OK) s->obs.reset(o.release());         // (a new configuration forgets the prepared observation; the old one survives a failed create)
  return rc;
}

int dddmr_rollout_mcl_prepare(dddmr_rollout_ctx* ctx, const float* flat_xyz, size_t n_flat, size_t flat_stride_bytes,
                              const float* less_sharp_xyz, size_t n_less_sharp, size_t less_sharp_stride_bytes, const double T_b2s[12],
                              dddmr_mcl_observation_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_prepare";
  if (stats) *stats = dddmr_mcl_observation_stats{};
  if (!T_b2s || !cloud_arg_ok(flat_xyz, n_flat, flat_stride_bytes) || !cloud_arg_ok(less_sharp_xyz, n_less_sharp, less_sharp_stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument or bad stride", what);
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(T_b2s[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: T_b2s[%d] is not finite", what, i);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  if (const int rc = mclobs_state(ctx, what, true, &s)) return rc;
  MclObs* o = s->obs.get();
  if (n_flat > o->cfg.max_flat_points || n_less_sharp > o->cfg.max_less_sharp_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu flat / %zu less-sharp points, configured for %u / %u", what, n_flat, n_less_sharp,
                o->cfg.max_flat_points, o->cfg.max_less_sharp_points);
  const size_t sf = flat_stride_bytes / sizeof(float), sl = less_sharp_stride_bytes / sizeof(float);
  for (size_t i = 0; i < n_flat + n_less_sharp; ++i) {
    const float* p = i < n_flat ? flat_xyz + i * sf : less_sharp_xyz + (i - n_flat) * sl;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: %s point %zu is not finite", what, i < n_flat ? "flat" : "less-sharp", i < n_flat ? i : i - n_flat);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (size_t i = 0; i < n_flat + n_less_sharp; ++i) {
    const float* p = i < n_flat ? flat_xyz + i * sf : less_sharp_xyz + (i - n_flat) * sl;
    o->in_host[i] = make_float4(p[0], p[1], p[2], 0.f);
  }
  return mclobs_run(ctx, what, o, o->in_dev, (uint32_t)n_flat, o->in_dev + n_flat, (uint32_t)n_less_sharp, T_b2s, stats);
}

int dddmr_rollout_mcl_prepare_from_sweep(dddmr_rollout_ctx* ctx, int32_t source_id, const double T_b2s[12], dddmr_mcl_observation_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_prepare_from_sweep";
  if (stats) *stats = dddmr_mcl_observation_stats{};
  if (!T_b2s) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument", what);
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(T_b2s[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: T_b2s[%d] is not finite", what, i);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  if (const int rc = mclobs_state(ctx, what, true, &s)) return rc;
  MclObs* o = s->obs.get();
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the source's current buffers are complete (set_lidar_sweep waits for its result before it commits) and stay as they
  // are while producer_mu is held: the next sweep builds beside them
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  LidarSweep* sw = nullptr;
  if (const int rc = sweep_features_of(ctx, source_id, what, &sw)) return rc;
  const LidarFeatures& lf = *sw->features;
  const int b = sw->cur;
  const uint32_t n_ls = lf.n_feat[b][1], n_flat = lf.n_feat[b][2];
  if (n_flat > o->cfg.max_flat_points || n_ls > o->cfg.max_less_sharp_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %u flat / %u less-sharp points, configured for %u / %u", what, n_flat, n_ls, o->cfg.max_flat_points,
                o->cfg.max_less_sharp_points);
  return mclobs_run(ctx, what, o, lf.feat[b] + feat_offset(sw->p.V, 2), n_flat, lf.feat[b] + feat_offset(sw->p.V, 1), n_ls, T_b2s, stats);
}

int dddmr_rollout_mcl_get_observation(dddmr_rollout_ctx* ctx, float* flat_xyz_out, size_t flat_capacity, size_t* n_flat,
                                      float* less_sharp_xyzi_out, size_t less_sharp_capacity, size_t* n_less_sharp, float* normals_out,
                                      size_t normals_capacity) {
  if (!ctx || !n_flat || !n_less_sharp) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_get_observation";
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  if (const int rc = mclobs_state(ctx, what, true, &s)) return rc;
  const MclObs* o = s->obs.get();
  const int b = o->cur;
  const size_t nf = o->n_flat[b], nl = o->n_ls[b], nn = o->n_ls_in[b];
  if ((flat_xyz_out && flat_capacity < nf) || (less_sharp_xyzi_out && less_sharp_capacity < nl) || (normals_out && normals_capacity < nn))
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu / %zu / %zu < %zu flat / %zu less-sharp points / %zu normals", what, flat_capacity,
                less_sharp_capacity, normals_capacity, nf, nl, nn);
  *n_flat = nf;
  *n_less_sharp = nl;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));          // (the pack kernel is not waited for by the prepare)
  std::vector<float4> h(std::max(nf, nn));
  if (flat_xyz_out && nf) {
    HIPCHK(ctx, hipMemcpy(h.data(), o->obs[b], nf * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nf; ++i) { flat_xyz_out[3 * i] = h[i].x; flat_xyz_out[3 * i + 1] = h[i].y; flat_xyz_out[3 * i + 2] = h[i].z; }
  }
  if (less_sharp_xyzi_out && nl) HIPCHK(ctx, hipMemcpy(less_sharp_xyzi_out, o->obs[b] + nf, nl * sizeof(float4), hipMemcpyDeviceToHost));
  if (normals_out && nn) {
    HIPCHK(ctx, hipMemcpy(h.data(), o->normals[b], nn * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nn; ++i) { normals_out[3 * i] = h[i].x; normals_out[3 * i + 1] = h[i].y; normals_out[3 * i + 2] = h[i].z; }
  }
  return DDDMR_OK;
}

int dddmr_rollout_mcl_measure_prepared(dddmr_rollout_ctx* ctx, const float* states, size_t n_states, float* likelihood_out, float* quality_out,
                                       dddmr_mcl_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_measure_prepared";
  if (stats) *stats = dddmr_mcl_stats{};
  if (n_states && (!states || !likelihood_out || !quality_out)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s = nullptr;
  if (const int rc = mclobs_state(ctx, what, true, &s)) return rc;
  const MclObs* o = s->obs.get();
  const int b = o->cur;
  if (o->n_flat[b] + o->n_ls[b] == 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: no observation point (the reference divides 0 by 0)", what);
  return mcl_run(ctx, what, s, o->obs[b], o->n_flat[b], o->n_ls[b], states, n_states, likelihood_out, quality_out, stats);
}

}  // extern "C"
