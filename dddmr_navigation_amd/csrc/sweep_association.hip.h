// sweep_association.hip.h -- what the host FeatureAssociation and mapOptimization need of a sweep beyond the three
// feature lists (lidar_features.hip.h): the rest of the front half of LeGO-LOAM's feature node, off unless asked for.
//
//   ImageProjection::findStartEndAngle       dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp:391-406
//   FeatureAssociation::adjustDistortion     src/featureAssociation.cpp:281-314: relTime, the part lidar_features leaves out
//   extractFeatures' cloudLabel loop         :486-490, and its VoxelGrid (downSizeFilter, leaf 0.2: :124, :510-514)
//   cloudSegmentation's outlier cloud        imageProjection.cpp:548-558, the intensity of :376
//   the four clouds as extractFeatures holds them (association frame) and as publishCloud publishes them (:1401-1404)
//
// Types as the reference has them: the three orientations are float32 message fields, `ori` and relTime are floats, M_PI
// and _scan_period are doubles; a float compared with or added to a double expression is promoted and the sum is stored
// back into the float.  Nothing is fused.
//
// halfPassed is a serial flag over the segmented cloud.  It flips once, after the first index i0 whose first-branch `ori`
// gives ori - start > M_PI; i0 itself still takes the first branch, everything behind it the second.  Here: every point
// computes the first-branch value and the flipping ones take an integer atomicMin on i0 (order-independent), then a
// second pass redoes the points behind i0 by the second branch.  No serial walk.
//
// cloudLabel follows the features' convention: every sweep is the first sweep of a fresh node, so a label is 2 or 1
// exactly for the ring's sharp / less-sharp picks, -1 for its flat picks and 0 otherwise.  A sixth's picks all lie inside
// that sixth (or are index 0, which no sixth covers), so the labels the loop of :486 reads are the final ones.
//
// VoxelGrid as oracle/ASSUMPTIONS.md rows 7 and 8 state it (float inverse leaf, floor, min_b from the ring's own
// candidates, output in voxel-index order, equal-voxel points summed in input order, in float), on the association-frame
// point (y, z, x).  ASSUMED here and nowhere pinned: downsample_all_data averages the intensity the same way, a float
// running sum in input order divided by the count.  PCL's overflow rule: with d = int64((max - min) * inverse_leaf) + 1
// per axis (a float product), dx * dy * dz above INT32_MAX hands the input through unchanged.  (Where the reference's
// int64 product itself overflows its behaviour is undefined; here that is an overflow too.)
//
// Seven launches behind k_feat_emit on the sweep's stream, none of them when the association is off, no host wait:
//   k_assoc_ends     one lane per raw record: the first and last record the ingest keeps as finite (one atomic per wave)
//   k_assoc_orient   one lane: the three orientations from those two pitch-removed points; zeros for an empty sweep
//   k_assoc_first    one lane per segmented point: the first-branch `ori`, atomicMin on i0 (one atomic per wave)
//   k_assoc_times    one lane per segmented point: its branch by i <= i0, relTime, the intensity
//   k_assoc_ring     one workgroup per ring: candidate flags in LDS, compacted in ascending index; (voxel, rank) keys
//                    sorted by the features' LDS bitonic sort (a ring has at most 4096 candidates: 78 compare-exchange
//                    rounds of 8 pairs per lane, where ranking by counting would read 4096 keys per candidate); the
//                    first lane of a voxel's run sums it in input order.  Also the ring's outlier count.
//   k_assoc_emit     one workgroup per ring: the rings' less-flat results concatenated in ring order, the three feature
//                    lists with their point times, every cloud in both frames
//   k_assoc_outliers one workgroup per row: the outlier cloud in raster order behind the rows' counts (a kernel of its
//                    own: with its three pointers k_assoc_emit spilled twelve scalar registers)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#include "dev_memory.hip.h"    // Owned, dev_alloc
#include "lidar_features.hip.h"
#include "lidar_sweep.hip.h"
#include "wave_ops.hip.h"      // block_rank, wave_min, wave_max, wave_sum

#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kAssocRingMax = kSweepMaxCols;     // a ring's candidates lie inside [start, end]: fewer than its columns
constexpr uint32_t kAssocNone = 0xFFFFFFFFu;
constexpr double kAssocPi = 3.14159265358979323846;   // M_PI

struct AssocResult {           // host-mapped; written by k_assoc_orient, k_assoc_times, k_assoc_emit and k_assoc_outliers
  uint32_t n_less_flat, n_outliers, i0, pad;
  float orient[4];             // start, end, diff
};

struct SweepAssoc {
  double scan_period = 0.1;
  float inv_leaf = 0.f;                // 1 / 0.2f in float
  uint32_t* ends = nullptr;            // [2] max of ~index and of index + 1 over the finite records; zero between sweeps
  uint32_t* i0 = nullptr;              // [1]
  float* orient = nullptr;             // [4] start, end, diff of the sweep being built
  uint32_t* ring_cnt = nullptr;        // [2 V] less-flat points, outliers per ring
  float4* stage = nullptr;             // [V H] a ring's less-flat points at row * H
  uint32_t* stage_idx = nullptr;       // [V H]
  // part of the sweep's double-buffered result, as the features are
  float* times[2] = {nullptr, nullptr};            // [V H] intensity per segmented point
  float4* list[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};        // [b][frame][V x kFeatPerRing], feat_offset() as the features
  float4* less_flat[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [b][frame][V H]
  uint32_t* less_flat_idx[2] = {nullptr, nullptr};
  float4* outliers[2] = {nullptr, nullptr};        // [V H]
  uint32_t n_less_flat[2] = {0, 0}, n_outliers[2] = {0, 0}, half_index[2] = {0, 0};
  float orientation[2][3] = {{0, 0, 0}, {0, 0, 0}};
  bool have[2] = {false, false};       // the buffer holds a sweep that was accepted with the association on
  AssocResult* res_host = nullptr;
  AssocResult* res_dev = nullptr;
  Owned mem;
};

__global__ __launch_bounds__(256) void k_assoc_ends(SweepParams k, const float* __restrict__ raw, uint32_t* __restrict__ ends) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  uint32_t first = 0u, last = 0u;
  if (i < k.n) {
    const float* sp = raw + (size_t)i * k.stride_floats;
    if (isfinite(sp[0]) && isfinite(sp[1]) && isfinite(sp[2])) {       // k_sweep_project's test
      first = kAssocNone - i;
      last = i + 1u;
    }
  }
  first = wave_max(first);
  last = wave_max(last);
  if ((threadIdx.x & 63) == 0 && last) {
    atomicMax(&ends[0], first);
    atomicMax(&ends[1], last);
  }
}

// imageProjection.cpp:391-406
__global__ __launch_bounds__(64) void k_assoc_orient(const float4* __restrict__ moved, uint32_t* __restrict__ ends, float* __restrict__ orient,
                                                     uint32_t* __restrict__ i0, AssocResult* __restrict__ res) {
  if (threadIdx.x != 0) return;
  float start = 0.f, end = 0.f, diff = 0.f;
  if (ends[1]) {
    const float4 a = moved[kAssocNone - ends[0]], b = moved[ends[1] - 1u];
    start = -atan2f(a.y, a.x);
    end = (float)((double)(-atan2f(b.y, b.x)) + 2 * kAssocPi);
    if ((double)(end - start) > 3 * kAssocPi) {
      end = (float)((double)end - 2 * kAssocPi);
    } else if ((double)(end - start) < kAssocPi) {
      end = (float)((double)end + 2 * kAssocPi);
    }
    diff = end - start;
  }
  ends[0] = 0u;
  ends[1] = 0u;
  orient[0] = start;
  orient[1] = end;
  orient[2] = diff;
  *i0 = kAssocNone;
  res->orient[0] = start;
  res->orient[1] = end;
  res->orient[2] = diff;
  __threadfence_system();
}

// featureAssociation.cpp:292-298
__device__ __forceinline__ float assoc_ori_first(float x, float y, float start) {
  float ori = -atan2f(y, x);
  if ((double)ori < (double)start - kAssocPi / 2) {
    ori = (float)((double)ori + 2 * kAssocPi);
  } else if ((double)ori > (double)start + kAssocPi * 3 / 2) {
    ori = (float)((double)ori - 2 * kAssocPi);
  }
  return ori;
}

// :301-306
__device__ __forceinline__ float assoc_ori_second(float x, float y, float end) {
  float ori = -atan2f(y, x);
  ori = (float)((double)ori + 2 * kAssocPi);
  if ((double)ori < (double)end - kAssocPi * 3 / 2) {
    ori = (float)((double)ori + 2 * kAssocPi);
  } else if ((double)ori > (double)end + kAssocPi / 2) {
    ori = (float)((double)ori - 2 * kAssocPi);
  }
  return ori;
}

__global__ __launch_bounds__(256) void k_assoc_first(const float4* __restrict__ seg_pt, const uint32_t* __restrict__ n_dev,
                                                     const float* __restrict__ orient, uint32_t* __restrict__ i0) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  uint32_t flip = kAssocNone;
  if (i < *n_dev) {
    const float4 q = seg_pt[i];
    const float start = orient[0];
    const float ori = assoc_ori_first(q.x, q.y, start);
    if ((double)(ori - start) > kAssocPi) flip = i;          // :299
  }
  flip = wave_min(flip);
  if ((threadIdx.x & 63) == 0 && flip != kAssocNone) atomicMin(i0, flip);
}

// :309-311
__global__ __launch_bounds__(256) void k_assoc_times(double scan_period, const float4* __restrict__ seg_pt, const uint32_t* __restrict__ seg_cr,
                                                     const uint32_t* __restrict__ n_dev, const float* __restrict__ orient,
                                                     const uint32_t* __restrict__ i0, float* __restrict__ times, AssocResult* __restrict__ res) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, n = *n_dev, half = min(*i0, n);
  if (i == 0) {
    res->i0 = half;
    __threadfence_system();
  }
  if (i >= n) return;
  const float4 q = seg_pt[i];
  const float start = orient[0];
  const float ori = i <= half ? assoc_ori_first(q.x, q.y, start) : assoc_ori_second(q.x, q.y, orient[1]);
  const float rel = (ori - start) / orient[2];
  const int ring = (int)((seg_cr[i] >> 16) & 0x7FFFu);     // int(row + col / 10000.0)
  times[i] = (float)((double)ring + scan_period * (double)rel);
}

__device__ __forceinline__ float3 assoc_frame(float4 q) { return make_float3(q.y, q.z, q.x); }   // :288-290

// One workgroup per ring.  flag[k - s]: segment index k is a less-flat candidate; cand[c]: the c-th candidate, ascending;
// key[]: (voxel << 12 | c), sorted.  The ring's result goes to stage[row * H ..], its size and the row's outlier count to
// ring_cnt.
__global__ __launch_bounds__(256) void k_assoc_ring(FeatParams k, uint32_t gsi, float inv_leaf, const int32_t* __restrict__ ring,
                                                    const uint32_t* __restrict__ slots, const uint32_t* __restrict__ slot_cnt,
                                                    const float4* __restrict__ seg_pt, const float* __restrict__ times,
                                                    const int32_t* __restrict__ label_img, float4* __restrict__ stage,
                                                    uint32_t* __restrict__ stage_idx, uint32_t* __restrict__ ring_cnt) {
  __shared__ unsigned long long key[kAssocRingMax];
  __shared__ uint16_t cand[kAssocRingMax];
  __shared__ uint8_t flag[kAssocRingMax];
  __shared__ uint32_t lds[4];
  __shared__ float s_mn[4][3], s_mx[4][3];
  __shared__ uint32_t s_outl;
  const uint32_t row = blockIdx.x, t = threadIdx.x;
  const int s = ring[row], e = ring[k.V + row];
  const uint32_t span = e >= s && (uint32_t)(e - s) < kAssocRingMax ? (uint32_t)(e - s + 1) : 0u;
  float4* out = stage + (size_t)row * k.H;
  uint32_t* out_idx = stage_idx + (size_t)row * k.H;

  // imageProjection.cpp:550-551: the row's outliers, counted here and written by k_assoc_outliers
  if (t == 0) s_outl = 0u;
  for (uint32_t i = t; i < span; i += 256) flag[i] = 0;
  __syncthreads();
  if (row > gsi) {
    uint32_t c = 0;
    for (uint32_t col = 5 * t; col < k.H; col += 5 * 256) c += label_img[(size_t)row * k.H + col] == kSweepInvalidLabel ? 1u : 0u;
    if (c) atomicAdd(&s_outl, c);
  }
  if (span) {
    for (int j = 0; j < 6; ++j) {                                  // :486: k = sp .. ep of the sixths that were not skipped
      int sp, ep;
      if (!feat_sixth(s, e, j, &sp, &ep)) continue;
      for (int q = sp + (int)t; q <= ep; q += 256) flag[q - s] = 1;
    }
  }
  __syncthreads();
  if (t == 0) ring_cnt[k.V + row] = s_outl;
  if (span) {                                                      // :487: cloudLabel > 0 are the ring's less-sharp picks
    const uint32_t n_less = slot_cnt[3 * row + 1];
    for (uint32_t i = t; i < n_less; i += 256) {
      const int ind = (int)slots[(size_t)row * kFeatPerRing + kFeatSharp + i] - s;
      if (ind >= 0 && (uint32_t)ind < span) flag[ind] = 0;
    }
  }
  __syncthreads();
  uint32_t n = 0;
  for (uint32_t base = 0; base < span; base += 256) {
    const uint32_t i = base + t;
    const bool f = i < span && flag[i];
    uint32_t total;
    const uint32_t r = block_rank<4>(f, lds, &total);
    if (f) cand[n + r] = (uint16_t)i;
    n += total;
  }
  __syncthreads();
  if (n == 0) {
    if (t == 0) ring_cnt[row] = 0u;
    return;
  }

  // getMinMax3D over the candidates
  const float inf = __int_as_float(0x7F800000);
  float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
  for (uint32_t c = t; c < n; c += 256) {
    const float3 p = assoc_frame(seg_pt[s + (int)cand[c]]);
    mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
    mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = wave_min(mn[a]);
    mx[a] = wave_max(mx[a]);
    if ((t & 63) == 0) {
      s_mn[t >> 6][a] = mn[a];
      s_mx[t >> 6][a] = mx[a];
    }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mn[a] = fminf(fminf(s_mn[0][a], s_mn[1][a]), fminf(s_mn[2][a], s_mn[3][a]));
    mx[a] = fmaxf(fmaxf(s_mx[0][a], s_mx[1][a]), fmaxf(s_mx[2][a], s_mx[3][a]));
  }
  // the leaf-size check: dx * dy * dz above INT32_MAX hands the input through
  bool over = false;
  long long prod = 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ext = (mx[a] - mn[a]) * inv_leaf;
    if (!(ext < 2147483648.f)) {
      over = true;
    } else if (!over) {
      prod *= (long long)ext + 1;
      if (prod > 2147483647ll) over = true;
    }
  }
  if (over) {
    for (uint32_t c = t; c < n; c += 256) {
      const int ind = s + (int)cand[c];
      const float3 p = assoc_frame(seg_pt[ind]);
      out[c] = make_float4(p.x, p.y, p.z, times[ind]);
      out_idx[c] = (uint32_t)ind;
    }
    if (t == 0) ring_cnt[row] = n;
    return;
  }
  const long long lo[3] = {(long long)floorf(mn[0] * inv_leaf), (long long)floorf(mn[1] * inv_leaf), (long long)floorf(mn[2] * inv_leaf)};
  const unsigned long long dx = (unsigned long long)((long long)floorf(mx[0] * inv_leaf) - lo[0] + 1);
  const unsigned long long dy = (unsigned long long)((long long)floorf(mx[1] * inv_leaf) - lo[1] + 1);
  uint32_t n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (uint32_t c = t; c < n2; c += 256) {
    unsigned long long v = ~0ull;
    if (c < n) {
      const float3 p = assoc_frame(seg_pt[s + (int)cand[c]]);
      const unsigned long long i0 = (unsigned long long)((long long)floorf(p.x * inv_leaf) - lo[0]);
      const unsigned long long i1 = (unsigned long long)((long long)floorf(p.y * inv_leaf) - lo[1]);
      const unsigned long long i2 = (unsigned long long)((long long)floorf(p.z * inv_leaf) - lo[2]);
      v = ((i0 + i1 * dx + i2 * dx * dy) << 12) | c;           // (below 2^34 voxels: the check above)
    }
    key[c] = v;
  }
  __syncthreads();
  feat_sort(key, n2);
  uint32_t n_out = 0;
  for (uint32_t base = 0; base < n; base += 256) {
    const uint32_t i = base + t;
    const bool head = i < n && (i == 0 || (key[i] >> 12) != (key[i - 1] >> 12));
    uint32_t total;
    const uint32_t r = block_rank<4>(head, lds, &total);
    if (head) {
      const unsigned long long voxel = key[i] >> 12;
      float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;              // float running sums in input order
      uint32_t q = i;
      for (; q < n && (key[q] >> 12) == voxel; ++q) {
        const int ind = s + (int)cand[key[q] & 4095u];
        const float3 p = assoc_frame(seg_pt[ind]);
        sx += p.x; sy += p.y; sz += p.z; si += times[ind];
      }
      const float c = (float)(q - i);
      out[n_out + r] = make_float4(sx / c, sy / c, sz / c, si / c);
      out_idx[n_out + r] = (uint32_t)(s + (int)cand[key[i] & 4095u]);
    }
    n_out += total;
  }
  if (t == 0) ring_cnt[row] = n_out;
}

// One workgroup per ring: waves 0 .. 3 sum what the rings before it hold of sharp, less sharp, flat and less flat.
// frame 0: the association frame, (y, z, x) of the segmented point; frame 1: through T_out.
__global__ __launch_bounds__(256) void k_assoc_emit(FeatParams k, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ slot_cnt,
                                                    const uint32_t* __restrict__ ring_cnt, const float4* __restrict__ seg_pt,
                                                    const float* __restrict__ times, const float4* __restrict__ stage,
                                                    const uint32_t* __restrict__ stage_idx, float4* __restrict__ list0,
                                                    float4* __restrict__ list1, float4* __restrict__ lf0, float4* __restrict__ lf1,
                                                    uint32_t* __restrict__ lf_idx, AssocResult* __restrict__ res) {
  __shared__ uint32_t before[4];
  const uint32_t row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, t = threadIdx.x;
  {
    uint32_t acc = 0;
    for (uint32_t r = lane; r < row; r += 64) acc += wave < 3 ? slot_cnt[3 * r + wave] : ring_cnt[r];
    acc = wave_sum(acc);
    if (lane == 0) {
      before[wave] = acc;
      if (row == k.V - 1 && wave == 3) {
        res->n_less_flat = acc + ring_cnt[row];
        __threadfence_system();
      }
    }
  }
  __syncthreads();
  // the three lists: k_feat_emit's slots, with the point times
  if (t < kFeatPerRing) {
    const int which = t < kFeatSharp ? 0 : t < kFeatSharp + kFeatLess ? 1 : 2;
    const uint32_t kth = t - (which == 0 ? 0u : which == 1 ? kFeatSharp : kFeatSharp + kFeatLess);
    if (kth < slot_cnt[3 * row + which]) {
      const uint32_t idx = slots[(size_t)row * kFeatPerRing + t], o = feat_offset(k.V, which) + before[which] + kth;
      const float4 q = seg_pt[idx];
      const float w = times[idx];
      const float3 g = affine_to_float(k.R, k.t, q.y, q.z, q.x);
      list0[o] = make_float4(q.y, q.z, q.x, w);
      list1[o] = make_float4(g.x, g.y, g.z, w);
    }
  }
  // :514: the rings' less-flat clouds in ring order
  const uint32_t n_lf = ring_cnt[row];
  for (uint32_t i = t; i < n_lf; i += 256) {
    const float4 q = stage[(size_t)row * k.H + i];
    const float3 g = affine_to_float(k.R, k.t, q.x, q.y, q.z);
    lf0[before[3] + i] = q;
    lf1[before[3] + i] = make_float4(g.x, g.y, g.z, q.w);
    lf_idx[before[3] + i] = stage_idx[(size_t)row * k.H + i];
  }
}

// imageProjection.cpp:550-553 in raster order, the intensity of :376: one workgroup per row, behind the rows' counts
__global__ __launch_bounds__(256) void k_assoc_outliers(uint32_t V, uint32_t H, uint32_t gsi, const uint32_t* __restrict__ ring_cnt,
                                                        const int32_t* __restrict__ label_img, const float4* __restrict__ pts,
                                                        float4* __restrict__ outl, AssocResult* __restrict__ res) {
  __shared__ uint32_t lds[4];
  __shared__ uint32_t s_before;
  const uint32_t row = blockIdx.x, t = threadIdx.x;
  if (t < 64) {
    uint32_t acc = 0;
    for (uint32_t r = t; r < row; r += 64) acc += ring_cnt[V + r];
    acc = wave_sum(acc);
    if (t == 0) {
      s_before = acc;
      if (row == V - 1) {
        res->n_outliers = acc + ring_cnt[V + row];
        __threadfence_system();
      }
    }
  }
  __syncthreads();
  if (row <= gsi || ring_cnt[V + row] == 0) return;
  uint32_t done = s_before;
  for (uint32_t base = 0; base < H; base += 5 * 256) {
    const uint32_t col = base + 5 * t;
    const size_t p = (size_t)row * H + col;
    const bool f = col < H && label_img[p] == kSweepInvalidLabel;
    uint32_t total;
    const uint32_t r = block_rank<4>(f, lds, &total);
    if (f) {
      const float4 q = pts[p];
      outl[done + r] = make_float4(q.x, q.y, q.z, (float)((double)(float)row + (double)(float)col / 10000.0));
    }
    done += total;
  }
}

inline int association_alloc(SweepAssoc& a, uint32_t V, uint32_t H) {
  const size_t px = (size_t)V * H;
  auto dev = [&a](auto** ptr, size_t count) { return dev_alloc_zeroed(a.mem.dev, ptr, count) == hipSuccess; };
  bool ok = dev(&a.ends, 2) && dev(&a.i0, 1) && dev(&a.orient, 4) && dev(&a.ring_cnt, 2 * (size_t)V) && dev(&a.stage, px) &&
            dev(&a.stage_idx, px);
  for (int b = 0; b < 2 && ok; ++b) {
    ok = dev(&a.times[b], px) && dev(&a.less_flat_idx[b], px) && dev(&a.outliers[b], px);
    for (int f = 0; f < 2 && ok; ++f) ok = dev(&a.list[b][f], (size_t)V * kFeatPerRing) && dev(&a.less_flat[b][f], px);
  }
  if (!ok) return -1;
  if (host_mapped_alloc(a.mem.host, &a.res_host, &a.res_dev, sizeof(AssocResult)) != 0) return -1;
  std::memset(a.res_host, 0, sizeof(AssocResult));
  a.inv_leaf = 1.0f / 0.2f;            // Eigen::Array4f::Ones() / leaf_size_.array()
  return 0;
}

// The association's launches of one sweep, behind features_launch on the same stream; nothing when it is off.  The counts
// are in res_host once the sweep's own wait has returned, as the features' are.
inline void association_launch(LidarFeatures& f, int b, const SweepParams& sweep, const float* raw, const float4* moved,
                               const int32_t* label_img, const float4* pts, hipStream_t stream) {
  SweepAssoc* a = f.assoc.get();
  if (!a) return;
  const FeatParams& k = f.p;
  const dim3 block(256), per_pixel((k.V * k.H + 255) / 256);
  if (sweep.n) hipLaunchKernelGGL(k_assoc_ends, dim3((sweep.n + 255) / 256), block, 0, stream, sweep, raw, a->ends);
  hipLaunchKernelGGL(k_assoc_orient, dim3(1), dim3(64), 0, stream, moved, a->ends, a->orient, a->i0, a->res_dev);
  hipLaunchKernelGGL(k_assoc_first, per_pixel, block, 0, stream, f.seg_pt[b], f.n_dev, a->orient, a->i0);
  hipLaunchKernelGGL(k_assoc_times, per_pixel, block, 0, stream, a->scan_period, f.seg_pt[b], f.seg_cr[b], f.n_dev, a->orient, a->i0,
                     a->times[b], a->res_dev);
  hipLaunchKernelGGL(k_assoc_ring, dim3(k.V), block, 0, stream, k, sweep.gsi, a->inv_leaf, f.ring[b], f.slots, f.slot_cnt, f.seg_pt[b],
                     a->times[b], label_img, a->stage, a->stage_idx, a->ring_cnt);
  hipLaunchKernelGGL(k_assoc_emit, dim3(k.V), block, 0, stream, k, f.slots, f.slot_cnt, a->ring_cnt, f.seg_pt[b], a->times[b], a->stage,
                     a->stage_idx, a->list[b][0], a->list[b][1], a->less_flat[b][0], a->less_flat[b][1], a->less_flat_idx[b], a->res_dev);
  hipLaunchKernelGGL(k_assoc_outliers, dim3(k.V), block, 0, stream, k.V, k.H, sweep.gsi, a->ring_cnt, label_img, pts, a->outliers[b],
                     a->res_dev);
}

}  // namespace dddmr
