// rollout_diag.hip.h -- diagnostics of rollout_engine.hip that no tick depends on: the phase stamps of a diagnostic build,
// the self-tests of the rollout's sin / cos, of the wave primitives and of the point grid, and the stream ceiling of the
// device.  Included by rollout_engine.hip after the context and its helpers are defined.
#pragma once
#include "point_grid_plan.hip.h"   // grid_shape, stage_cloud; point_grid.hip.h: the grid, its walks and its builder
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

// dddmr_rollout_selftest_wave_wide, first part: block_excl_scan<16> and wave_last in one workgroup of 1024 lanes (lanes at
// or past n take part with value 0).  scan[0][t] the exclusive prefix, scan[1][t] wave_last of t's wave's inclusive scan.
__global__ __launch_bounds__(1024) void k_selftest_wave_wide_scan(const uint32_t* __restrict__ values, uint32_t n, uint32_t* __restrict__ scan,
                                                                  uint32_t* __restrict__ misc) {
  __shared__ uint32_t s_w[16];
  const uint32_t t = threadIdx.x;
  const uint32_t v = t < n ? values[t] : 0u;
  uint32_t total;
  scan[t] = block_excl_scan<16>(v, s_w, &total);
  scan[1024 + t] = wave_last(wave_incl_scan_u32(v));
  if (t == 0) misc[0] = total;
}
// ... second part: the reductions on the types the kernels use and selftest_wave_ops does not, over one wave whose
// lanes hold the 64 words as they are (float: their bits).
__global__ __launch_bounds__(64) void k_selftest_wave_wide_reduce(const uint32_t* __restrict__ lanes, uint32_t* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  const uint32_t w = lanes[t];
  out[0 * 64 + t] = __float_as_uint(wave_min(__uint_as_float(w)));
  out[1 * 64 + t] = __float_as_uint(wave_max(__uint_as_float(w)));
  out[2 * 64 + t] = (uint32_t)wave_min((int)w);
  out[3 * 64 + t] = (uint32_t)wave_max((int)w);
}
// ... third part: last_block's hand-off.  Lane 63 of each of a workgroup's four waves stores one word to the
// workgroup's own slots with a device-scope atomic; whoever last_block names reads all 4 * gridDim.x slots with
// ld_agent, stores their sum and counts itself a winner.  The word of slot i: wave_wide_word(gridDim.x, i).
__host__ __device__ inline uint32_t wave_wide_word(uint32_t groups, uint32_t i) { return groups * 0x9E3779B1u + i * i + 1u; }
__global__ __launch_bounds__(256) void k_selftest_wave_wide_last(uint32_t* __restrict__ slots, uint32_t* __restrict__ ticket,
                                                                 uint32_t* __restrict__ misc) {
  if ((threadIdx.x & 63u) == 63u) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    __hip_atomic_store(&slots[i], wave_wide_word(gridDim.x, i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (last_block(ticket)) {
    uint32_t sum = 0;
    for (uint32_t i = 0; i < 4u * gridDim.x; ++i) sum += ld_agent(&slots[i]);
    misc[2] = sum;
    atomicAdd(&misc[1], 1u);
  }
}

// dddmr_rollout_selftest_point_grid: the thread-per-query walks of point_grid.hip.h, eight words per query as the header
// lays out.
__global__ __launch_bounds__(256) void k_selftest_grid_thread(PointGrid g, const float* __restrict__ queries, uint32_t m, float r_box, float r2,
                                                              int stop_at, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const float qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
  uint32_t* o = out + 8 * (size_t)i;
  o[0] = (uint32_t)grid_radius_count(g, qx, qy, qz, r_box, r2, stop_at);
  o[1] = (uint32_t)grid_radius_count(g, qx, qy, qz, r_box, r2, 0x7fffffff);
  o[2] = __float_as_uint(grid_nearest(g, qx, qy, qz, r_box));
  const GridHit hit = grid_nearest_id(g, qx, qy, qz, r_box, r2);
  o[3] = hit.id;
  o[4] = __float_as_uint(hit.d2);
  uint32_t cnt = 0, sum = 0, x = 0;
  grid_for_each(g, qx, qy, qz, r_box, [&](const float4 p) {
    const uint32_t id = __float_as_uint(p.w);
    ++cnt;
    sum += id;
    x ^= id;
    return false;
  });
  o[5] = cnt;
  o[6] = sum;
  o[7] = x;
}
// ... and the wave-per-query walk, five words per query.
__global__ __launch_bounds__(256) void k_selftest_grid_wave(PointGrid g, const float* __restrict__ queries, uint32_t m, float r_box, float r2,
                                                            uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m) return;                                        // (the whole wave)
  const float qx = queries[3 * i], qy = queries[3 * i + 1], qz = queries[3 * i + 2];
  uint32_t cnt = 0, sum = 0, x = 0, inside = 0;
  float best = __int_as_float(0x7F800000);
  grid_for_each_wave(g, qx, qy, qz, r_box, lane, [&](const float4 p) {
    const uint32_t id = __float_as_uint(p.w);
    const float d2 = l2_simple(p.x, p.y, p.z, qx, qy, qz);
    ++cnt;
    sum += id;
    x ^= id;
    if (d2 < r2) ++inside;
    best = fminf(best, d2);
  });
  cnt = wave_sum(cnt);
  sum = wave_sum(sum);
  inside = wave_sum(inside);
  best = wave_min(best);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x ^= wave_xor(x, off);
  if (lane == 0) {
    uint32_t* o = out + 5 * (size_t)i;
    o[0] = cnt;
    o[1] = sum;
    o[2] = x;
    o[3] = inside;
    o[4] = __float_as_uint(best);
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

// The rest of wave_ops.hip.h: block_excl_scan<16> and wave_last over n <= 1024 values in one workgroup of 1024 lanes, the
// float and int reductions over the 64 words of `lanes`, and last_block's hand-off among n_groups workgroups.
int dddmr_rollout_selftest_wave_wide(dddmr_rollout_ctx* ctx, const uint32_t* values, size_t n, const uint32_t* lanes, uint32_t n_groups,
                                     uint32_t* scan_out, uint32_t* reduce_out, uint32_t* misc_out) {
  if (!ctx || !lanes || !scan_out || !reduce_out || !misc_out || n > 1024 || (n && !values) || n_groups == 0 ||
      n_groups > DDDMR_WAVE_WIDE_MAX_GROUPS)
    return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "selftest_wave_wide");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  constexpr size_t kScan = DDDMR_WAVE_WIDE_SCAN, kReduce = DDDMR_WAVE_WIDE_REDUCE, kMisc = DDDMR_WAVE_WIDE_MISC;
  DevScope tmp;
  uint32_t* buf = nullptr;                                   // scan, reduce, misc and the ticket, the values, the lanes, the slots
  HIPCHK(ctx, dev_alloc(tmp.mem, &buf, kScan + kReduce + kMisc + 1 + 1024 + 64 + 4 * (size_t)n_groups));
  Drain drain{ctx->stream};                                  // behind `tmp`: an error exit waits before the buffer is freed
  uint32_t *scan = buf, *reduce = scan + kScan, *misc = reduce + kReduce, *ticket = misc + kMisc, *val = ticket + 1, *lan = val + 1024,
           *slots = lan + 64;
  HIPCHK(ctx, hipMemsetAsync(misc, 0, (kMisc + 1) * sizeof(uint32_t), ctx->stream));
  if (n) HIPCHK(ctx, hipMemcpyAsync(val, values, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(lan, lanes, 64 * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_selftest_wave_wide_scan, dim3(1), dim3(1024), 0, ctx->stream, val, (uint32_t)n, scan, misc);
  hipLaunchKernelGGL(k_selftest_wave_wide_reduce, dim3(1), dim3(64), 0, ctx->stream, lan, reduce);
  hipLaunchKernelGGL(k_selftest_wave_wide_last, dim3(n_groups), dim3(256), 0, ctx->stream, slots, ticket, misc);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(scan_out, scan, kScan * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(reduce_out, reduce, kReduce * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(misc_out, misc, kMisc * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  drain.armed = false;
  return DDDMR_OK;
}

// The point grid as the modules use it -- grid_shape, grid_alloc and grid_build over the caller's points and box, then
// every walk of point_grid.hip.h over the caller's queries -- with the grid itself and the walks' results copied back.
int dddmr_rollout_selftest_point_grid(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, const float lo[3], const float hi[3],
                                      const float cell[2], uint32_t cap_cells, const float* queries, size_t m, const float radius[2],
                                      int32_t stop_at, uint32_t grid_out[8], uint32_t* cell_start_out, uint32_t* sorted_out,
                                      uint32_t* thread_out, uint32_t* wave_out) {
  if (!ctx || !lo || !hi || !cell || !radius || !grid_out || !cell_start_out) return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "selftest_point_grid");
  if (n > DDDMR_POINT_GRID_MAX_POINTS || m > DDDMR_POINT_GRID_MAX_QUERIES || (n && (!xyz || !sorted_out)) ||
      (m && (!queries || !thread_out || !wave_out)))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "selftest_point_grid: %zu points (at most %d), %zu queries (at most %d), or a null pointer with a count",
                n, DDDMR_POINT_GRID_MAX_POINTS, m, DDDMR_POINT_GRID_MAX_QUERIES);
  if (cap_cells == 0 || cap_cells > DDDMR_POINT_GRID_MAX_CELLS || stop_at < 1)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "selftest_point_grid: cap_cells %u outside 1 .. %d, or stop_at %d below 1", cap_cells,
                DDDMR_POINT_GRID_MAX_CELLS, stop_at);
  // the int casts of grid_shape and of the cell functions stay defined: coordinates within 1e6 m, cells of 1 cm at least
  for (int a = 0; a < 3; ++a)
    if (!(std::fabs(lo[a]) <= 1e6f) || !(std::fabs(hi[a]) <= 1e6f) || !(lo[a] <= hi[a]))
      return fail(ctx, DDDMR_ERR_BAD_ARG, "selftest_point_grid: the box is not finite within 1e6 m, or lo > hi");
  if (!(cell[0] >= 0.01f && cell[0] <= 1e6f) || !(cell[1] >= 0.01f && cell[1] <= 1e6f) || !(radius[0] >= 0.f && radius[0] <= 1e6f) ||
      !(radius[1] >= 0.f && radius[1] <= 1e12f))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "selftest_point_grid: a cell size outside 0.01 .. 1e6 m, or r_box / r2 negative or not finite");
  std::vector<float4> pts(std::max<size_t>(n, 1));
  float box_lo[3], box_hi[3];
  if (!stage_cloud(xyz, n, 12, pts.data(), box_lo, box_hi) || !cloud_box_ok(box_lo, box_lo) || !cloud_box_ok(box_hi, box_hi))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "selftest_point_grid: a point is not finite within 1e6 m");
  for (size_t i = 0; i < 3 * m; ++i)
    if (!(std::fabs(queries[i]) <= 1e6f)) return fail(ctx, DDDMR_ERR_BAD_ARG, "selftest_point_grid: a query is not finite within 1e6 m");
  HIPCHK(ctx, hipSetDevice(ctx->device));

  GridBuf b;
  grid_shape(b.g, lo, hi, cell[0], cell[1], cap_cells);
  const size_t cells = (size_t)b.g.nx * b.g.ny * b.g.nz;
  DevScope tmp;
  float4* dev_pts = nullptr;
  uint2* slot = nullptr;
  float* dev_q = nullptr;
  uint32_t* dev_out = nullptr;                               // [m][8] of the thread walk, then [m][5] of the wave walk
  void* temp = nullptr;
  size_t temp_bytes = 0;
  {
    uint32_t* v = nullptr;
    HIPCHK(ctx, rocprim::exclusive_scan(nullptr, temp_bytes, v, v, 0u, cells + 1, rocprim::plus<uint32_t>(), ctx->stream));
  }
  if (grid_alloc(tmp.mem, b, (uint32_t)cells, (uint32_t)n) != 0) return fail(ctx, DDDMR_ERR_HIP, "selftest_point_grid: grid storage");
  HIPCHK(ctx, dev_alloc(tmp.mem, &dev_pts, pts.size()));
  HIPCHK(ctx, dev_alloc(tmp.mem, &slot, pts.size()));
  HIPCHK(ctx, dev_alloc(tmp.mem, &dev_q, 3 * std::max<size_t>(m, 1)));
  HIPCHK(ctx, dev_alloc(tmp.mem, &dev_out, 13 * std::max<size_t>(m, 1)));
  HIPCHK(ctx, dev_alloc(tmp.mem, reinterpret_cast<unsigned char**>(&temp), std::max<size_t>(temp_bytes, 1)));
  Drain drain{ctx->stream};                                  // behind `tmp`: an error exit waits before the scratch is freed
  HIPCHK(ctx, hipMemcpyAsync(dev_pts, pts.data(), pts.size() * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  if (m) HIPCHK(ctx, hipMemcpyAsync(dev_q, queries, 3 * m * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (const int rc = grid_build(ctx, temp, temp_bytes, b, dev_pts, (uint32_t)n, slot, ctx->stream)) return rc;
  if (m) {
    hipLaunchKernelGGL(k_selftest_grid_thread, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, b.g, dev_q, (uint32_t)m, radius[0],
                       radius[1], (int)stop_at, dev_out);
    hipLaunchKernelGGL(k_selftest_grid_wave, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, ctx->stream, b.g, dev_q, (uint32_t)m, radius[0],
                       radius[1], dev_out + 8 * m);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(cell_start_out, b.g.cell_start, (cells + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (n) HIPCHK(ctx, hipMemcpyAsync(sorted_out, b.g.sorted, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  if (m) {
    HIPCHK(ctx, hipMemcpyAsync(thread_out, dev_out, 8 * m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(wave_out, dev_out + 8 * m, 5 * m * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  drain.armed = false;
  const float geom[5] = {b.g.ox, b.g.oy, b.g.oz, b.g.inv_xy, b.g.inv_z};
  grid_out[0] = (uint32_t)b.g.nx;
  grid_out[1] = (uint32_t)b.g.ny;
  grid_out[2] = (uint32_t)b.g.nz;
  std::memcpy(grid_out + 3, geom, sizeof(geom));
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
