// lidar_features.hip.h -- the feature half of the reference's mcl_feature_node on a sweep source: what lies between the
// sweep ingest (lidar_sweep.hip.h) and the particle filter's likelihood (mcl_measure.hip.h).
//
// ImageProjection::cloudSegmentation's segmented_cloud and seg_msg (dddmr_lego_loam/lego_loam_bor/src/imageProjection.cpp
// :542-580), then FeatureAssociation::calculateSmoothness (src/featureAssociation.cpp:318-341), markOccludedPoints
// (:343-379), extractFeatures (:381-491, without the cloudLabel / less-flat loop and its VoxelGrid), adjustDistortion's
// axis change (:281-314, without relTime) and publishCloud's transform (:1384-1405).  What is left out here is in
// sweep_association.hip.h, off unless asked for.  Types as featureAssociation.h
// :62-63, :100-103 has them: the thresholds, ranges and curvatures are floats; the literals 0.3 and 0.02 are doubles.
//
// Every sweep behaves like the FIRST sweep of a freshly constructed FeatureAssociation (std::vector::resize leaves
// zeros): slot 4 of cloudSmoothness, ring 0's sp, lies below calculateSmoothness's range and is never rewritten by the
// reference, which carries its sorted leftover from sweep to sweep; here it is {0.0f, ind 0} every time.  Equal
// curvatures sort by ascending index (std::sort leaves their order undefined).
//
// Six launches behind k_sweep_output on the sweep's stream, none of them when features are off, no host wait between:
//   k_feat_blocks    one lane per pixel: per-workgroup counts of kept pixels (k_sweep_blocks' scheme, own kernels so
//   k_feat_segment   the sweep's stay what they are); ranks -> the segmented cloud in raster order, per-row start / end
//   k_feat_curv      one lane per segmented point: curvature; the occlusion mark as a GATHER over the neighbours whose
//                    conditions would mark this point (no store races with calculateSmoothness's reset); how far a pick
//                    at this point suppresses forward and backward (the column-jump test of :423-442, precomputed)
//   k_feat_sort      one workgroup per sixth of a ring: a bitonic sort of (curvature bits, index) in LDS, written back
//                    over cloudSmoothness's slots [sp, ep); the sorts depend on nothing the walks change
//   k_feat_extract   one wave per ring: the ring's meta bytes (ground, picked, reaches) in LDS with a one-entry halo in
//                    front (suppression reaches one index before the ring's first point and never into what another
//                    ring reads, so the rings are independent); per sixth the sorted keys into LDS, then the two
//                    walks in BALLOT form: the wave tests 64 sorted candidates at once, takes the first passing lane,
//                    applies its suppression and tests again -- the serial result, in rounds = picks instead of steps =
//                    candidates; a sorted walk stops at the first key beyond its threshold.  std::sort covers [sp, ep)
//                    and the walks include ep: slot ep is always {curvature[ep], ep} and is tested on its own.
//   k_feat_emit      the per-ring slots (12 sharp, 120 less sharp, 24 flat) compacted in ring order, (y, z, x) through
//                    T_out as pcl::transformPointCloud(Affine3d) does it, ring as the fourth float
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_memory.hip.h"    // Owned, dev_alloc
#include "lidar_sweep.hip.h"
#include "wave_ops.hip.h"      // block_rank, wave_sum

#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kFeatSharp = 12, kFeatLess = 120, kFeatFlat = 24, kFeatPerRing = kFeatSharp + kFeatLess + kFeatFlat;
constexpr uint32_t kFeatSortMax = 1024;          // a sixth of a 4096-column ring is at most 682 slots
// meta word of a segmented point
constexpr uint32_t kMetaGround = 1u, kMetaPicked = 2u;     // bits 2-4: forward reach, bits 5-7: backward reach: one byte

struct FeatParams {
  double R[9], t[3];           // T_out
  float edge_threshold, surf_threshold;
  uint32_t V, H;
};

struct FeatResult {            // host-mapped; written by k_feat_segment's last workgroup and by k_feat_emit
  uint32_t n_seg;
  uint32_t n_feat[3];
};

struct SweepAssoc;              // sweep_association.hip.h, included at the end of this file

struct LidarFeatures {
  FeatParams p;
  std::unique_ptr<SweepAssoc, LateDelete<SweepAssoc>> assoc;   // not null: the sweep association is on
  uint32_t* block_cnt = nullptr;       // [workgroups]
  uint32_t* n_dev = nullptr;           // [1] segmented points of the sweep being built
  float* curv = nullptr;               // [V H]
  uint32_t* meta = nullptr;            // [V H]
  unsigned long long* smooth = nullptr;   // [V H] cloudSmoothness, each sixth sorted
  uint32_t* slots = nullptr;           // [V x kFeatPerRing] segment indices
  uint32_t* slot_cnt = nullptr;        // [V x 3]
  // part of the sweep's double-buffered result: [cur] belongs to the latest accepted sweep
  float4* seg_pt[2] = {nullptr, nullptr};      // x y z range
  uint32_t* seg_cr[2] = {nullptr, nullptr};    // column | row << 16 | ground << 31
  int32_t* ring[2] = {nullptr, nullptr};       // [2 V] start_ring_index, end_ring_index
  float4* feat[2] = {nullptr, nullptr};        // [V x kFeatPerRing] sharp at 0, less sharp at 12 V, flat at 132 V: x y z ring
  uint32_t* feat_idx[2] = {nullptr, nullptr};
  uint32_t n_seg[2] = {0, 0}, n_feat[2][3] = {{0, 0, 0}, {0, 0, 0}};
  bool have_sweep = false;             // a sweep has been accepted since the features were switched on
  FeatResult* res_host = nullptr;
  FeatResult* res_dev = nullptr;
  Owned mem;
};

__host__ __device__ __forceinline__ uint32_t feat_offset(uint32_t V, int which) {
  return which == 0 ? 0u : which == 1 ? kFeatSharp * V : (kFeatSharp + kFeatLess) * V;
}

// :548-562
__device__ __forceinline__ bool feat_keep(const FeatParams& k, uint32_t p, const int32_t* __restrict__ label_img,
                                          const uint8_t* __restrict__ ground_img, bool* ground) {
  if (p >= k.V * k.H) return false;
  const int32_t label = label_img[p];
  const bool g = ground_img[p] == 1;
  *ground = g;
  if (!(label > 0 || g)) return false;
  if (label == kSweepInvalidLabel) return false;
  const int j = (int)(p % k.H);
  if (g && j % 5 != 0 && j > 5 && j < (int)k.H - 5) return false;
  return true;
}

__global__ __launch_bounds__(256) void k_feat_blocks(FeatParams k, const int32_t* __restrict__ label_img, const uint8_t* __restrict__ ground_img,
                                                     uint32_t* __restrict__ block_cnt) {
  __shared__ uint32_t lds[4];
  bool g;
  const bool keep = feat_keep(k, blockIdx.x * 256 + threadIdx.x, label_img, ground_img, &g);
  uint32_t total;
  block_rank<4>(keep, lds, &total);
  if (threadIdx.x == 0) block_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_feat_segment(FeatParams k, const int32_t* __restrict__ label_img, const uint8_t* __restrict__ ground_img,
                                                      const float* __restrict__ range_img, const float4* __restrict__ pts,
                                                      const uint32_t* __restrict__ block_cnt, float4* __restrict__ seg_pt,
                                                      uint32_t* __restrict__ seg_cr, int32_t* __restrict__ ring, uint32_t* __restrict__ n_dev,
                                                      FeatResult* __restrict__ res) {
  __shared__ uint32_t lds[4];
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  bool g = false;
  const bool keep = feat_keep(k, p, label_img, ground_img, &g);
  uint32_t before = 0;
  for (uint32_t i = threadIdx.x; i < blockIdx.x; i += 256) before += block_cnt[i];
  before = wave_sum(before);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = before;
  __syncthreads();
  before = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  uint32_t total;
  const uint32_t rank = before + block_rank<4>(keep, lds, &total);
  if (keep) {
    const float4 q = pts[p];
    seg_pt[rank] = make_float4(q.x, q.y, q.z, range_img[p]);
    seg_cr[rank] = (p % k.H) | ((p / k.H) << 16) | (g ? 0x80000000u : 0u);
  }
  if (p < k.V * k.H && p % k.H == 0) {               // :545, :579: the count before the row and after the row before it
    const uint32_t row = p / k.H;
    ring[row] = (int32_t)rank - 1 + 5;
    if (row) ring[k.V + row - 1] = (int32_t)rank - 1 - 5;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    ring[2 * k.V - 1] = (int32_t)(before + total) - 1 - 5;
    *n_dev = before + total;
    res->n_seg = before + total;
    __threadfence_system();
  }
}

__device__ __forceinline__ int feat_col(uint32_t cr) { return (int)(cr & 0xFFFFu); }
__device__ __forceinline__ int feat_abs(int v) { return v < 0 ? -v : v; }

// :346-367 for loop index i: 1 = marks i - 5 .. i, 2 = marks i + 1 .. i + 6, 0 = neither
__device__ __forceinline__ int feat_occluder(const float4* __restrict__ seg_pt, const uint32_t* __restrict__ seg_cr, int i, int n) {
  if (i < 5 || i >= n - 6) return 0;
  if (feat_abs(feat_col(seg_cr[i + 1]) - feat_col(seg_cr[i])) >= 10) return 0;
  const float d1 = seg_pt[i].w, d2 = seg_pt[i + 1].w;
  if ((double)(d1 - d2) > 0.3) return 1;
  if ((double)(d2 - d1) > 0.3) return 2;
  return 0;
}

__global__ __launch_bounds__(256) void k_feat_curv(const float4* __restrict__ seg_pt, const uint32_t* __restrict__ seg_cr,
                                                   const uint32_t* __restrict__ n_dev, float* __restrict__ curv, uint32_t* __restrict__ meta) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x), n = (int)*n_dev;
  if (i >= n) return;
  float c = 0.f;                                       // a fresh node's cloudCurvature outside the loop's range
  if (i >= 5 && i < n - 5) {                           // :320-333, left to right
    const float d = seg_pt[i - 5].w + seg_pt[i - 4].w + seg_pt[i - 3].w + seg_pt[i - 2].w + seg_pt[i - 1].w - seg_pt[i].w * 10 +
                    seg_pt[i + 1].w + seg_pt[i + 2].w + seg_pt[i + 3].w + seg_pt[i + 4].w + seg_pt[i + 5].w;
    c = d * d;
  }
  curv[i] = c;
  const uint32_t cr = seg_cr[i];
  bool marked = false;
  for (int j = i; j <= i + 5; ++j) marked |= feat_occluder(seg_pt, seg_cr, j, n) == 1;        // i is in j - 5 .. j
  for (int j = i - 6; j <= i - 1; ++j) marked |= feat_occluder(seg_pt, seg_cr, j, n) == 2;    // i is in j + 1 .. j + 6
  if (i >= 5 && i < n - 6) {                           // :370-377
    const float r = seg_pt[i].w;
    const float diff1 = fabsf(seg_pt[i - 1].w - r), diff2 = fabsf(seg_pt[i + 1].w - r);
    marked |= (double)diff1 > 0.02 * (double)r && (double)diff2 > 0.02 * (double)r;
  }
  // :423-442: how many of ind + 1 .. ind + 5 / ind - 1 .. ind - 5 a pick at this point marks
  int fwd = 0, bwd = 0;
  for (int l = 1; l <= 5 && i + l < n; ++l) {
    if (feat_abs(feat_col(seg_cr[i + l]) - feat_col(seg_cr[i + l - 1])) > 10) break;
    fwd = l;
  }
  for (int l = -1; l >= -5 && i + l >= 0; --l) {       // `ind + l < 0` is skipped, and so is everything after it
    if (feat_abs(feat_col(seg_cr[i + l]) - feat_col(seg_cr[i + l + 1])) > 10) break;
    bwd = -l;
  }
  meta[i] = (cr >> 31) | (marked ? kMetaPicked : 0u) | ((uint32_t)fwd << 2) | ((uint32_t)bwd << 5);
}

// ascending bitonic sort of n (a power of two) keys in the caller's LDS array by the whole workgroup, whatever its size:
// k_feat_sort has at most kFeatSortMax keys, k_assoc_ring (sweep_association.hip.h) up to 4096
__device__ __forceinline__ void feat_sort(unsigned long long* key, uint32_t n) {
  for (uint32_t size = 2; size <= n; size <<= 1)
    for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (uint32_t t = threadIdx.x; t < n / 2; t += blockDim.x) {
        const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const unsigned long long a = key[lo], b = key[hi];
        const bool up = (lo & size) == 0;
        if ((a > b) == up) {
          key[lo] = b;
          key[hi] = a;
        }
      }
      __syncthreads();
    }
}

// the sixth j of a ring (:391-397, int division): false when it is skipped
__device__ __forceinline__ bool feat_sixth(int s, int e, int j, int* sp, int* ep) {
  *sp = (s * (6 - j) + e * j) / 6;
  *ep = (s * (5 - j) + e * (j + 1)) / 6 - 1;
  return *sp < *ep && (uint32_t)(*ep - *sp) <= kFeatSortMax;   // (a sixth of a ring of <= 4096 points is below 683 slots)
}

// std::sort of cloudSmoothness over [sp, ep) for every sixth of every ring: one workgroup each.  smooth[] is
// cloudSmoothness itself, (curvature bits << 32 | ind) per slot; the sorts depend on nothing the walks change, so all of
// them run side by side before the serial part.
__global__ __launch_bounds__(256) void k_feat_sort(FeatParams k, const int32_t* __restrict__ ring, const float* __restrict__ curv,
                                                   unsigned long long* __restrict__ smooth) {
  __shared__ unsigned long long key[kFeatSortMax];
  const uint32_t row = blockIdx.x / 6;
  int sp, ep;
  if (!feat_sixth(ring[row], ring[k.V + row], (int)(blockIdx.x % 6), &sp, &ep)) return;
  const uint32_t len = (uint32_t)(ep - sp);
  uint32_t n = 2;
  while (n < len) n <<= 1;
  for (uint32_t t = threadIdx.x; t < n; t += 256) {
    const int slot = sp + (int)t;
    unsigned long long v = ~0ull;
    // a slot below calculateSmoothness's range is a fresh node's {0.0f, 0}
    if (t < len) v = slot < 5 ? 0ull : ((unsigned long long)__float_as_uint(curv[slot]) << 32) | (uint32_t)slot;
    key[t] = v;
  }
  __syncthreads();
  feat_sort(key, n);
  for (uint32_t t = threadIdx.x; t < len; t += 256) smooth[sp + t] = key[t];
}

// One wave per ring.  flag[1 + (index - first)] is the point's meta byte, its picked bit the walk's cloudNeighborPicked;
// flag[0] is the halo.
__global__ __launch_bounds__(64) void k_feat_extract(FeatParams k, const int32_t* __restrict__ ring, const float* __restrict__ curv,
                                                     const uint32_t* __restrict__ meta, const unsigned long long* __restrict__ smooth,
                                                     uint32_t* __restrict__ slots, uint32_t* __restrict__ slot_cnt) {
  __shared__ unsigned long long key[kFeatSortMax];
  __shared__ uint8_t flag[kSweepMaxCols + 64];
  const uint32_t row = blockIdx.x, lane = threadIdx.x;
  const int s = ring[row], e = ring[k.V + row];
  const int first = s - 4, last = e + 5;                       // the ring's points; last < first: none
  uint32_t* out = slots + (size_t)row * kFeatPerRing;
  uint32_t n_sharp = 0, n_less = 0, n_flat = 0;
  for (int i = first - 1 + (int)lane; i <= last; i += 64) flag[i - (first - 1)] = i >= 0 ? (uint8_t)meta[i] : 0;
  __syncthreads();

  // One walk over up to 64 candidates in walk order (lane order): returns when none of them passes any more (false) or
  // the walk's break was taken (true).  edge: :405-444; flat: :447-484.
  auto rounds = [&](bool edge, bool valid, uint32_t ind, float c, int* count) -> bool {
    uint32_t m = 0;
    bool alive = false;
    if (valid) {
      m = flag[(int)ind - (first - 1)];
      alive = edge ? (c > k.edge_threshold && !(m & kMetaGround)) : (c < k.surf_threshold && (m & kMetaGround));
    }
    for (;;) {
      const bool ok = alive && !(flag[(int)ind - (first - 1)] & kMetaPicked);
      const unsigned long long pass = __ballot(ok);
      if (!pass) return false;
      const int f = __ffsll((long long)pass) - 1;
      const uint32_t pind = __shfl(ind, f, 64), pm = __shfl(m, f, 64);
      ++*count;
      if (edge) {
        if (*count > 20) return true;                          // the 21st: break
        if (lane == 0) {
          if (*count <= 2) out[n_sharp] = pind;
          out[kFeatSharp + n_less] = pind;
        }
        if (*count <= 2) ++n_sharp;
        ++n_less;
      } else {
        if (lane == 0) out[kFeatSharp + kFeatLess + n_flat] = pind;
        ++n_flat;
        if (*count >= 4) return true;                          // the 4th is pushed and breaks before it suppresses
      }
      const int off = (int)lane - 5, fwd = (int)((pm >> 2) & 7u), bwd = (int)((pm >> 5) & 7u);
      if (lane < 11 && off >= -bwd && off <= fwd) flag[(int)pind + off - (first - 1)] |= kMetaPicked;   // one byte per lane
      alive = alive && (int)lane > f;
      __syncthreads();
    }
  };

  for (int j = 0; j < 6; ++j) {
    int sp, ep;
    if (!feat_sixth(s, e, j, &sp, &ep)) continue;
    const uint32_t len = (uint32_t)(ep - sp);
    for (uint32_t t = lane; t < len; t += 64) key[t] = smooth[sp + t];     // the sorted sixth, loads in flight together
    const float c_ep = curv[ep];
    __syncthreads();
    // the edge walk, k = ep down to sp
    int count = 0;
    bool done = rounds(true, lane == 0, (uint32_t)ep, c_ep, &count);
    for (uint32_t base = 0; base < len && !done; base += 64) {
      const uint32_t t = base + lane;
      const bool valid = t < len;
      const unsigned long long v = valid ? key[len - 1 - t] : 0ull;
      const float c = __uint_as_float((uint32_t)(v >> 32));
      done = rounds(true, valid, (uint32_t)v, c, &count);
      if (__ballot(valid && !(c > k.edge_threshold))) break;  // sorted: nothing behind it passes either
    }
    // the flat walk, k = sp up to ep
    count = 0;
    done = false;
    for (uint32_t base = 0; base < len && !done; base += 64) {
      const uint32_t t = base + lane;
      const bool valid = t < len;
      const unsigned long long v = valid ? key[t] : 0ull;
      const float c = __uint_as_float((uint32_t)(v >> 32));
      done = rounds(false, valid, (uint32_t)v, c, &count);
      if (__ballot(valid && !(c < k.surf_threshold))) break;
    }
    if (!done) rounds(false, lane == 0, (uint32_t)ep, c_ep, &count);
    __syncthreads();
  }
  if (lane == 0) {
    slot_cnt[3 * row + 0] = n_sharp;
    slot_cnt[3 * row + 1] = n_less;
    slot_cnt[3 * row + 2] = n_flat;
  }
}

// :288-290 then pcl::transformPointCloud(cloud, cloud, Affine3d): one workgroup per ring, lanes over its slots; waves
// 0 .. 2 sum what the rings before it hold of sharp, less sharp and flat
__global__ __launch_bounds__(256) void k_feat_emit(FeatParams k, const uint32_t* __restrict__ slots, const uint32_t* __restrict__ slot_cnt,
                                                   const float4* __restrict__ seg_pt, const uint32_t* __restrict__ seg_cr,
                                                   float4* __restrict__ feat, uint32_t* __restrict__ feat_idx, FeatResult* __restrict__ res) {
  __shared__ uint32_t before[3];
  const uint32_t row = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < 3) {
    uint32_t acc = 0;
    for (uint32_t r = lane; r < row; r += 64) acc += slot_cnt[3 * r + wave];
    acc = wave_sum(acc);
    if (lane == 0) {
      before[wave] = acc;
      if (row == k.V - 1) {
        res->n_feat[wave] = acc + slot_cnt[3 * row + wave];
        __threadfence_system();
      }
    }
  }
  __syncthreads();
  const uint32_t sl = threadIdx.x;
  if (sl >= kFeatPerRing) return;
  const int which = sl < kFeatSharp ? 0 : sl < kFeatSharp + kFeatLess ? 1 : 2;
  const uint32_t kth = sl - (which == 0 ? 0u : which == 1 ? kFeatSharp : kFeatSharp + kFeatLess);
  if (kth >= slot_cnt[3 * row + which]) return;
  const uint32_t idx = slots[(size_t)row * kFeatPerRing + sl], o = feat_offset(k.V, which) + before[which] + kth;
  const float4 q = seg_pt[idx];
  const float3 g = affine_to_float(k.R, k.t, q.y, q.z, q.x);
  feat[o] = make_float4(g.x, g.y, g.z, (float)(int)((seg_cr[idx] >> 16) & 0x7FFFu));
  feat_idx[o] = idx;
}

inline void features_free(LidarFeatures& f) { f = LidarFeatures(); }

// f.p is set
inline int features_alloc(LidarFeatures& f) {
  const size_t V = f.p.V, px = V * f.p.H, blocks = (px + 255) / 256;
  auto dev = [&f](auto** ptr, size_t count) { return dev_alloc_zeroed(f.mem.dev, ptr, count) == hipSuccess; };
  bool ok = dev(&f.block_cnt, blocks) && dev(&f.n_dev, 1) && dev(&f.curv, px) && dev(&f.meta, px) && dev(&f.smooth, px) &&
            dev(&f.slots, V * kFeatPerRing) && dev(&f.slot_cnt, V * 3);
  for (int b = 0; b < 2 && ok; ++b)
    ok = dev(&f.seg_pt[b], px) && dev(&f.seg_cr[b], px) && dev(&f.ring[b], 2 * V) && dev(&f.feat[b], V * kFeatPerRing) &&
         dev(&f.feat_idx[b], V * kFeatPerRing);
  if (!ok) return -1;
  if (host_mapped_alloc(f.mem.host, &f.res_host, &f.res_dev, sizeof(FeatResult)) != 0) return -1;
  std::memset(f.res_host, 0, sizeof(FeatResult));
  return 0;
}

// The launches of one sweep, behind k_sweep_output on its stream; everything goes to the [b] buffers.  The counts are in
// f.res_host once the sweep's own wait (k_feed_emit's release, which follows on the stream) has returned.
inline void features_launch(LidarFeatures& f, int b, const int32_t* label_img, const uint8_t* ground_img, const float* range_img,
                            const float4* pts, hipStream_t stream) {
  const FeatParams& k = f.p;
  const uint32_t px = k.V * k.H;
  const dim3 block(256), per_pixel((px + 255) / 256);
  hipLaunchKernelGGL(k_feat_blocks, per_pixel, block, 0, stream, k, label_img, ground_img, f.block_cnt);
  hipLaunchKernelGGL(k_feat_segment, per_pixel, block, 0, stream, k, label_img, ground_img, range_img, pts, f.block_cnt, f.seg_pt[b],
                     f.seg_cr[b], f.ring[b], f.n_dev, f.res_dev);
  hipLaunchKernelGGL(k_feat_curv, per_pixel, block, 0, stream, f.seg_pt[b], f.seg_cr[b], f.n_dev, f.curv, f.meta);
  hipLaunchKernelGGL(k_feat_sort, dim3(6 * k.V), block, 0, stream, k, f.ring[b], f.curv, f.smooth);
  hipLaunchKernelGGL(k_feat_extract, dim3(k.V), dim3(64), 0, stream, k, f.ring[b], f.curv, f.meta, f.smooth, f.slots, f.slot_cnt);
  hipLaunchKernelGGL(k_feat_emit, dim3(k.V), block, 0, stream, k, f.slots, f.slot_cnt, f.seg_pt[b], f.seg_cr[b], f.feat[b], f.feat_idx[b],
                     f.res_dev);
}

}  // namespace dddmr

#include "sweep_association.hip.h"   // SweepAssoc and its launches: what LidarFeatures::assoc points to
