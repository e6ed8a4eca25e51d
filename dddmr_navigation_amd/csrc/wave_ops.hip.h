// wave_ops.hip.h -- the wave and workgroup idioms the kernels share, one spelling each.  Device code only, nothing of the
// project included.  A wave is 64 lanes; unless a contract says otherwise every lane of the wave (block_*: of the
// workgroup) makes the call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace dddmr {

// relaxed device-scope loads: what another workgroup of this launch wrote with device-scope atomics
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_agent(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// This wave's stores and atomics have been acknowledged (written through to the level every CU of the chip reads:
// device-scope atomics and sc1 loads go there).  What a hand-off inside a launch needs here is exactly that plus a
// barrier / ticket; an agent-scope fence (__threadfence) also writes the XCD's L2 back, which cost the last launch
// 120 us when all 2090 workgroups issued one (profiles/r03_C5M_fused_kernel_stats.csv history in DESIGN.md).
__device__ __forceinline__ void wait_own_memory_ops() { __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// lane 63's value, in every lane (all 64 lanes active)
__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }
// how many bits of a ballot lie below the calling lane: its rank among the set lanes
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Inclusive prefix sum over the 64 lanes of a wave with DPP moves (register-to-register, a few
// cycles each) instead of LDS-crossbar shuffles: Hillis-Steele inside the 16-lane rows
// (row_shr 1, 2, 4, 8; lanes without a source add 0), then the row totals are carried over
// with row_bcast:15 (into rows 1 and 3) and row_bcast:31 (into rows 2 and 3).
// All 64 lanes must be active: an inactive lane contributes nothing and breaks the carries behind it.
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
  return v;
}

// exclusive prefix of one value per lane over a block of W waves, in lane order (two barriers; wsum = W LDS words)
template <int W>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t incl = wave_incl_scan_u32(v);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const uint32_t x = wsum[j];
    tot += x;
    if (j < w) base += x;
  }
  __syncthreads();
  *total = tot;
  return base + incl - v;
}

// exclusive rank of the flagged lanes of a block of W waves in lane order, and their number (two barriers; lds = W words)
template <int W>
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* lds, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) lds[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const uint32_t c = lds[w];
    if (w < wave) base += c;
    tot += c;
  }
  __syncthreads();
  *total = tot;
  return base + lanes_below(m);
}

// Wave-aggregated append to a counter in global memory or in LDS: one atomic per wave (none when no lane keeps), by the
// first keeping lane; the keeping lanes stay in lane order.  Returns the lane's output index (meaningless where !keep).
__device__ __forceinline__ uint32_t wave_append(bool keep, uint32_t* counter) {
  const unsigned long long mask = __ballot(keep);
  if (!mask) return 0u;
  const int leader = __ffsll((long long)mask) - 1;
  uint32_t base = 0;
  if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
  return (uint32_t)__shfl((int)base, leader, 64) + lanes_below(mask);
}

// Xor-butterfly reductions, offsets 32 down to 1: every lane gets the wave's minimum / maximum / wrapping sum.  For uint32_t,
// int, float (minimum and maximum only: fminf / fmaxf) and unsigned long long, which travels as two 32-bit halves.
__device__ __forceinline__ int wave_xor(int v, int off) { return __shfl_xor(v, off, 64); }
__device__ __forceinline__ uint32_t wave_xor(uint32_t v, int off) { return (uint32_t)__shfl_xor((int)v, off, 64); }
__device__ __forceinline__ float wave_xor(float v, int off) { return __shfl_xor(v, off, 64); }
__device__ __forceinline__ unsigned long long wave_xor(unsigned long long v, int off) {
  return ((unsigned long long)wave_xor((uint32_t)(v >> 32), off) << 32) | wave_xor((uint32_t)v, off);
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, wave_xor(v, off));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = max(v, wave_xor(v, off));
  return v;
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
  static_assert(!std::is_floating_point<T>::value, "a float sum depends on its order: spell it out where it is needed");
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += wave_xor(v, off);
  return v;
}

// Every thread of every workgroup calls it once, after its last write.  True in thread 0 of the workgroup that
// finishes last, which then sees what all the others wrote with device-scope atomics (device-scope ticket).
__device__ __forceinline__ bool last_block(uint32_t* ticket) {
  wait_own_memory_ops();
  __syncthreads();
  if (threadIdx.x != 0) return false;
  return __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
}

}  // namespace dddmr
