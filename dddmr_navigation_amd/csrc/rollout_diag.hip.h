// rollout_diag.hip.h -- diagnostics of rollout_engine.hip that no tick depends on: the phase stamps of a diagnostic build,
// the self-tests of the rollout's sin / cos and of the wave primitives, and the stream ceiling of the device.  Included by
// rollout_engine.hip after the context and its helpers are defined.
#pragma once
#include "wave_ops.hip.h"

namespace dddmr {

// dddmr_rollout_selftest_wave_ops: every primitive of wave_ops.hip.h once, in one workgroup of 256 lanes.  Lanes at or
// past n take part with value 0 and flag false (the primitives need whole waves).  out32 / out64 as the header lays out;
// the global append's counter is out32's word [9][2], preset by the host.
__global__ __launch_bounds__(256) void k_selftest_wave_ops(const uint32_t* __restrict__ values, const uint8_t* __restrict__ flags, uint32_t n,
                                                           uint32_t base, uint32_t* __restrict__ out32,
                                                           unsigned long long* __restrict__ out64) {
  __shared__ uint32_t s_w[4], s_counter;
  const uint32_t t = threadIdx.x;
  const uint32_t v = t < n ? values[t] : 0u;
  const bool flag = t < n && flags[t] != 0;
  const unsigned long long v64 = ((unsigned long long)v << 32) | (t & 63u);
  uint32_t* totals = out32 + 9 * 256;
  if (t == 0) s_counter = base;
  __syncthreads();
  uint32_t scan_total, rank_total;
  out32[0 * 256 + t] = wave_incl_scan_u32(v);
  out32[1 * 256 + t] = block_excl_scan<4>(v, s_w, &scan_total);
  out32[2 * 256 + t] = block_rank<4>(flag, s_w, &rank_total);
  out32[3 * 256 + t] = wave_append(flag, &totals[2]);
  out32[4 * 256 + t] = wave_append(flag, &s_counter);
  out32[5 * 256 + t] = wave_min(v);
  out32[6 * 256 + t] = wave_max(v);
  out32[7 * 256 + t] = wave_sum(v);
  out32[8 * 256 + t] = __float_as_uint(wave_min((float)v));
  out64[0 * 256 + t] = wave_min(v64);
  out64[1 * 256 + t] = wave_sum(v64);
  __syncthreads();
  if (t == 0) {
    totals[0] = scan_total;
    totals[1] = rank_total;
    totals[3] = s_counter;
  }
}

}  // namespace dddmr

extern "C" {

#ifdef DDDMR_PHASE_STAMPS
// diagnostic build only: copy the per-workgroup phase stamps of the last k_score launch
int dddmr_rollout_diag_stamps(unsigned long long* out, size_t n_words) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), n_words * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
// ... and of the last k_bin_count launch (binning, assignment and rollout workgroups)
int dddmr_rollout_diag_rstamps(unsigned long long* out, size_t n_words) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rstamps), n_words * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif

// The rollout's own sin / cos (sincos_heading, rollout_kernels.hip.h) of `n` angles, one per lane: what the tests bound
// its error with.
int dddmr_rollout_selftest_sincos(dddmr_rollout_ctx* ctx, const double* angles, size_t n, double* sin_out,
                                  double* cos_out) {
  if (!ctx || !angles || !sin_out || !cos_out || n == 0 || n > ((size_t)1 << 24)) return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "selftest_sincos");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevScope tmp;
  double* buf = nullptr;
  HIPCHK(ctx, dev_alloc(tmp.mem, &buf, 3 * n));
  HIPCHK(ctx, hipMemcpyAsync(buf, angles, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_selftest_sincos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, buf, (int)n,
                     buf + n, buf + 2 * n);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(sin_out, buf + n, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(cos_out, buf + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return DDDMR_OK;
}

// The primitives of wave_ops.hip.h over n <= 256 values and flags (none is allowed), one per lane of a single workgroup:
// what the tests compare with their own arithmetic.  Both appends start their counter at append_base.
int dddmr_rollout_selftest_wave_ops(dddmr_rollout_ctx* ctx, const uint32_t* values, const uint8_t* flags, size_t n,
                                    uint32_t append_base, uint32_t* out32, unsigned long long* out64) {
  if (!ctx || !out32 || !out64 || n > 256 || (n && (!values || !flags))) return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "selftest_wave_ops");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  constexpr size_t kOut32 = DDDMR_WAVE_OPS_OUT32, kOut64 = DDDMR_WAVE_OPS_OUT64;
  DevScope tmp;
  unsigned long long* buf64 = nullptr;                       // out64, out32, the values, the flags
  HIPCHK(ctx, dev_alloc(tmp.mem, &buf64, kOut64 + kOut32 / 2 + 256 / 2 + 256 / 8));
  uint32_t* buf32 = reinterpret_cast<uint32_t*>(buf64 + kOut64);
  uint32_t* val = buf32 + kOut32;
  uint8_t* flg = reinterpret_cast<uint8_t*>(val + 256);
  if (n) {
    HIPCHK(ctx, hipMemcpyAsync(val, values, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(flg, flags, n, hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(buf32 + 9 * 256 + 2), (int)append_base, 1, ctx->stream));
  hipLaunchKernelGGL(k_selftest_wave_ops, dim3(1), dim3(256), 0, ctx->stream, val, flg, (uint32_t)n, append_base, buf32, buf64);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out32, buf32, kOut32 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(out64, buf64, kOut64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return DDDMR_OK;
}

// Stream ceiling of this GPU ("a measured stream-copy ceiling on the same GPU ... both
// denominators"): `bytes` per buffer (>= 1 GiB defeats the 256 MB of MALL), `reps` launches each.
int dddmr_rollout_stream_ceiling(dddmr_rollout_ctx* ctx, size_t bytes, int32_t reps, double* copy_gbps,
                                 double* read_gbps) {
  if (!ctx || !copy_gbps || !read_gbps || reps <= 0 || bytes < (1u << 20)) return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "stream_ceiling");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t n = bytes / sizeof(float4);
  // one pass of the four-loads-in-flight loop per lane measured best (grid sweep 1k ... 64k workgroups:
  // copy 4.5 -> 5.2 TB/s, read 5.7 -> 6.0 TB/s; tools/exp_ceiling.py)
  const int blocks = ctx->ceil_blocks > 0 ? ctx->ceil_blocks : (int)std::min<size_t>(65536, std::max<size_t>(1, n / (256 * 4)));
  // on any return, in this order: the stream runs dry, the events go, the buffers go
  DevScope tmp;
  struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() { for (hipEvent_t e : {e0, e1}) if (e) (void)hipEventDestroy(e); }
  } ev;
  Drain drain{ctx->stream};
  float4 *src = nullptr, *dst = nullptr;
  float* sink = nullptr;
  HIPCHK(ctx, dev_alloc(tmp.mem, &src, n));
  HIPCHK(ctx, dev_alloc(tmp.mem, &dst, n));
  HIPCHK(ctx, dev_alloc(tmp.mem, &sink, (size_t)blocks * 256));
  HIPCHK(ctx, hipMemsetAsync(src, 0x11, n * sizeof(float4), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(dst, 0, n * sizeof(float4), ctx->stream));
  HIPCHK(ctx, hipEventCreate(&ev.e0));
  HIPCHK(ctx, hipEventCreate(&ev.e1));
  float ms = 0.f;
  hipLaunchKernelGGL(k_stream_copy, dim3(blocks), dim3(256), 0, ctx->stream, src, dst, n);   // warm-up
  HIPCHK(ctx, hipEventRecord(ev.e0, ctx->stream));
  for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_stream_copy, dim3(blocks), dim3(256), 0, ctx->stream, src, dst, n);
  HIPCHK(ctx, hipEventRecord(ev.e1, ctx->stream));
  HIPCHK(ctx, hipEventSynchronize(ev.e1));
  HIPCHK(ctx, hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *copy_gbps = 2.0 * (double)(n * sizeof(float4)) * reps / ((double)ms * 1e-3) / 1e9;
  hipLaunchKernelGGL(k_stream_read, dim3(blocks), dim3(256), 0, ctx->stream, src, sink, n);
  HIPCHK(ctx, hipEventRecord(ev.e0, ctx->stream));
  for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(k_stream_read, dim3(blocks), dim3(256), 0, ctx->stream, src, sink, n);
  HIPCHK(ctx, hipEventRecord(ev.e1, ctx->stream));
  HIPCHK(ctx, hipEventSynchronize(ev.e1));
  HIPCHK(ctx, hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *read_gbps = (double)(n * sizeof(float4)) * reps / ((double)ms * 1e-3) / 1e9;
  HIPCHK(ctx, hipGetLastError());
  return DDDMR_OK;
}

}  // extern "C"
