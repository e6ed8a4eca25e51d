// rollout_diag.hip.h -- diagnostics of rollout_engine.hip that no tick depends on: the phase stamps of a diagnostic build,
// the rollout's sin / cos self-test and the stream ceiling of the device.  Included by rollout_engine.hip after the
// context and its helpers are defined.
#pragma once

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
