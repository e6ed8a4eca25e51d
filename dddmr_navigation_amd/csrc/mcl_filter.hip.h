// mcl_filter.hip.h -- mcl_3dl's particle set in device memory: the filter step as a chain of device calls in which no
// per-particle result crosses the bus.  The caller draws every random number; the device consumes them in the
// reference's order (citations relative to the reference's src/dddmr_mcl_3dl/):
//   pf::ParticleFilter::measure / expectation / expectationBiased / covariance / max   include/mcl_3dl/pf.h:247-362
//   resampleUsingNoiseGenerator / addNoiseUsingNoiseGenerator                          include/mcl_3dl/pf.h:182-232
//   ParticleWeightedMeanQuat::add, State6DOF::operator+                                 include/mcl_3dl/state_6dof.h:222-234,303-315
//   MotionPredictionModelDifferentialDrive::predict                                     ..._differential_drive.h:56-67
//   the bias lambda, update_noise_func, integ_reset_func                                src/mcl_3dl.cpp:518-530,221-229,570-575
//
// Per-particle stages take one lane per particle.  A sum whose order the result shows is taken in index order: pf::measure's
// sum, the running sum that decides p_num and resample's accum prefix are ONE lane's serial loop over values staged in
// LDS; the means' ten sums each and the covariance's 21 are one accumulator per lane of ONE wave, every lane walking the
// same staged rows in index order.  No tree, no scan over floats.  Float operations go through exact_float.hip.h
// (no fused multiply-add); the pure host part is mcl_filter_plan.hip.h.
//
// Poses, integrals, noise and probabilities are double-buffered: an entry writes the other generation and the host flips
// the index once the stream has drained without an error, so a refused or failed call changes nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_memory.hip.h"        // Owned, dev_alloc, Drain, feed_wait
#include "mcl_filter_plan.hip.h"
#include "mcl_measure.hip.h"
#include "mcl_observation.hip.h"   // the prepared observation

#pragma clang fp contract(off)

namespace dddmr {

constexpr uint32_t kFilterChunk = 2048;       // floats of one staged chunk of a serial loop (8 KiB of LDS)
constexpr uint32_t kFilterRows = 64;          // term rows staged per step of k_filter_reduce
constexpr uint32_t kFilterTerms = 20;         // ten of the biased mean, ten of the unbiased one
constexpr uint32_t kFilterNoRow = 0xffffffffu;
// A serial loop reads this many staged values into registers before its dependent adds, so that the LDS reads do not
// wait for one another; the adds keep their order.
constexpr uint32_t kFilterAhead = 8;

struct FilterOut {                            // device memory, downloaded once per measure
  float sums_b[10], sums_u[10];               // p_sum_, e_.pos_, front_sum_, up_sum_
  float mean_u[7];
  float cov[21];                              // (j, k), j <= k, row by row
  float max_state[13];
  float weight_sum;
  uint32_t p_num, restored, max_index;
};

struct FilterRs {                             // device memory: resample's counts
  uint32_t n_dup, n_at_end, n_ties, ok;
};

struct FilterGen {                            // one generation's pointers
  const float *pose, *integ, *noise, *prob;
};
struct FilterGenOut {
  float *pose, *integ, *noise, *prob;
};

// Quat * Vec3 with the RAW rotation (quat.h:139-143)
__device__ __forceinline__ float3 filter_rotate(float4 q, float vx, float vy, float vz) {
  const float4 a = mcl_qmul(q, make_float4(vx, vy, vz, 0.0f));
  const float4 b = mcl_qmul(a, make_float4(-q.x, -q.y, -q.z, q.w));
  return make_float3(b.x, b.y, b.z);
}

// predict(), one lane per particle
__global__ __launch_bounds__(256) void k_filter_predict(uint32_t n, FilterOdom o, FilterGen in, float* __restrict__ pose_out,
                                                        float* __restrict__ integ_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float* ps = in.pose + 7 * (size_t)i;
  const float* ig = in.integ + 6 * (size_t)i;
  const float* nz = in.noise + 4 * (size_t)i;
  const float ll = nz[0], la = nz[1], al = nz[2], aa = nz[3];
  const float4 rot = make_float4(ps[3], ps[4], ps[5], ps[6]);
  // diff = relative_translation_ * float(1.0 + noise_ll_) + Vec3(noise_al_ * relative_angle_, 0, 0)
  const float s1 = (float)(1.0 + (double)ll);
  const float dx = fadd(fmul(o.rt[0], s1), fmul(al, o.rel_ang));
  const float dy = fadd(fmul(o.rt[1], s1), 0.0f);
  const float dz = fadd(fmul(o.rt[2], s1), 0.0f);
  float lx = fadd(ig[0], fsub(dx, o.rt[0])), ly = fadd(ig[1], fsub(dy, o.rt[1])), lz = fadd(ig[2], fsub(dz, o.rt[2]));
  const float3 mv = filter_rotate(rot, dx, dy, dz);
  const float yaw_diff = fadd(fmul(la, o.rt_norm), fmul(aa, o.rel_ang));
  // Quat(Vec3(0, 0, 1), yaw_diff): setAxisAng divides the axis by its norm 1, then normalize()
  const float half = yaw_diff / 2;
  const float sn = sinf(half);
  const float4 qz = mcl_rotation(fmul(0.0f, sn), fmul(0.0f, sn), fmul(1.0f, sn), cosf(half));
  float4 r = mcl_qmul(mcl_qmul(qz, rot), make_float4(o.rq[0], o.rq[1], o.rq[2], o.rq[3]));
  r = mcl_rotation(r.x, r.y, r.z, r.w);
  float* po = pose_out + 7 * (size_t)i;
  po[0] = fadd(ps[0], mv.x); po[1] = fadd(ps[1], mv.y); po[2] = fadd(ps[2], mv.z);
  po[3] = r.x; po[4] = r.y; po[5] = r.z; po[6] = r.w;
  float* io = integ_out + 6 * (size_t)i;
  io[0] = fmul(lx, o.decay_lin); io[1] = fmul(ly, o.decay_lin); io[2] = fmul(lz, o.decay_lin);
  io[3] = fmul(fadd(ig[3], 0.0f), o.decay_ang); io[4] = fmul(fadd(ig[4], 0.0f), o.decay_ang);
  io[5] = fmul(fadd(ig[5], yaw_diff), o.decay_ang);
}

// State6DOF::operator+ of particle `src` and a noise row into particle i of the other generation
__device__ __forceinline__ void filter_add_row(const FilterGen& in, uint32_t src, const float* __restrict__ nz, const FilterGenOut& out, uint32_t i,
                                               bool normalize) {
  const float* ps = in.pose + 7 * (size_t)src;
  const float* ig = in.integ + 6 * (size_t)src;
  float4 r = mcl_qmul(make_float4(nz[3], nz[4], nz[5], nz[6]), make_float4(ps[3], ps[4], ps[5], ps[6]));   // a.rot_ * rot_
  if (normalize) r = mcl_rotation(r.x, r.y, r.z, r.w);
  float* po = out.pose + 7 * (size_t)i;
  po[0] = fadd(ps[0], nz[0]); po[1] = fadd(ps[1], nz[1]); po[2] = fadd(ps[2], nz[2]);
  po[3] = r.x; po[4] = r.y; po[5] = r.z; po[6] = r.w;
  float* io = out.integ + 6 * (size_t)i;
  io[0] = fadd(ig[0], nz[0]); io[1] = fadd(ig[1], nz[1]); io[2] = fadd(ig[2], nz[2]);
  io[3] = fadd(ig[3], nz[7]); io[4] = fadd(ig[4], nz[8]); io[5] = fadd(ig[5], nz[9]);
  float* no = out.noise + 4 * (size_t)i;                       // the operator's result is default-constructed: noise_* 0
  no[0] = 0.0f; no[1] = 0.0f; no[2] = 0.0f; no[3] = 0.0f;
}

__global__ __launch_bounds__(256) void k_filter_add_noise(uint32_t n, FilterGen in, const float* __restrict__ rows, FilterGenOut out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  filter_add_row(in, i, rows + 10 * (size_t)i, out, i, false);
}

// pf::measure's products
__global__ __launch_bounds__(256) void k_filter_weigh(uint32_t n, const float* __restrict__ prob, const float* __restrict__ lik,
                                                      float* __restrict__ prod) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) prod[i] = fmul(prob[i], lik[i]);
}

// ... and their float sum in index order: one workgroup stages, one lane adds
__global__ __launch_bounds__(256) void k_filter_sum(uint32_t n, const float* __restrict__ prod, FilterOut* __restrict__ out) {
  __shared__ float s_c[kFilterChunk];
  float sum = 0.0f;
  for (uint32_t base = 0; base < n; base += kFilterChunk) {
    const uint32_t cnt = min(kFilterChunk, n - base);
    for (uint32_t j = threadIdx.x; j < cnt; j += 256) s_c[j] = prod[base + j];
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t j = 0;
      for (; j + kFilterAhead <= cnt; j += kFilterAhead) {
        float v[kFilterAhead];
#pragma unroll
        for (uint32_t a = 0; a < kFilterAhead; ++a) v[a] = s_c[j + a];
#pragma unroll
        for (uint32_t a = 0; a < kFilterAhead; ++a) sum = fadd(sum, v[a]);
      }
      for (; j < cnt; ++j) sum = fadd(sum, s_c[j]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out->weight_sum = sum;
    out->restored = sum > 0.0f ? 0u : 1u;
  }
}

// The division (or the restore), the bias, and both means' term rows; one lane per particle.
//   prob_old  the generation before the measure;  prob_new  in: the products, out: the probabilities after it
//   terms     [n][20]: w, pos * w, front * w, up * w with w = p * bias, then the same with w = p
__global__ __launch_bounds__(256) void k_filter_terms(uint32_t n, const float* __restrict__ prob_old, float* __restrict__ prob_new,
                                                      const FilterOut* __restrict__ out, const float* __restrict__ pose, FilterBias b,
                                                      float* __restrict__ bias, float* __restrict__ terms) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float sum = out->weight_sum;
  const float p = sum > 0.0f ? prob_new[i] / sum : prob_old[i];
  prob_new[i] = p;
  const float* ps = pose + 7 * (size_t)i;
  const float4 rot = make_float4(ps[3], ps[4], ps[5], ps[6]);
  float pb = 1.0f;
  if (b.has_prev) {
    const float dx = fsub(ps[0], b.prev_pos[0]), dy = fsub(ps[1], b.prev_pos[1]), dz = fsub(ps[2], b.prev_pos[2]);
    const float lin_diff = sqrtf(dot3(dx, dy, dz, dx, dy, dz));
    const float4 q = mcl_qmul(rot, make_float4(b.prev_inv[0], b.prev_inv[1], b.prev_inv[2], b.prev_inv[3]));
    float ang = 0.0f;                                                        // getAxisAng
    if (!(fabs((double)q.w) >= 1.0 - 0.000001)) {
      ang = (float)((double)acosf(q.w) * 2.0);
      if ((double)ang > M_PI) ang = (float)((double)ang - 2.0 * M_PI);
    }
    const float nl_lin = fmul(b.a_lin, expf(fmul(-lin_diff, lin_diff) / b.sq2_lin));
    const float nl_ang = fmul(b.a_ang, expf(fmul(-ang, ang) / b.sq2_ang));
    pb = (float)((double)fmul(nl_lin, nl_ang) + 1e-6);
  }
  bias[i] = pb;
  const float3 front = filter_rotate(rot, 1.0f, 0.0f, 0.0f), up = filter_rotate(rot, 0.0f, 0.0f, 1.0f);
  float* t = terms + kFilterTerms * (size_t)i;
  const float w[2] = {fmul(p, pb), p};
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    float* r = t + 10 * m;
    r[0] = w[m];
    r[1] = fmul(ps[0], w[m]); r[2] = fmul(ps[1], w[m]); r[3] = fmul(ps[2], w[m]);
    r[4] = fmul(front.x, w[m]); r[5] = fmul(front.y, w[m]); r[6] = fmul(front.z, w[m]);
    r[7] = fmul(up.x, w[m]); r[8] = fmul(up.y, w[m]); r[9] = fmul(up.z, w[m]);
  }
}

// p_num and max(), both means' sums, expectation(1.0)'s mean and the covariance: ONE wave.
__global__ __launch_bounds__(64) void k_filter_reduce(uint32_t n, const float* __restrict__ prob, const float* __restrict__ terms,
                                                      const float* __restrict__ pose, const float* __restrict__ integ,
                                                      FilterOut* __restrict__ out) {
  __shared__ float s_c[kFilterChunk];
  __shared__ float s_t[kFilterRows * kFilterTerms];
  __shared__ float s_pose[kFilterRows * 7];
  __shared__ float s_p[kFilterRows];
  __shared__ float s_sum[kFilterTerms];
  __shared__ float s_e[7];
  __shared__ uint32_t s_num[2];
  const uint32_t lane = threadIdx.x;
  // the running sum of expectation(1.0) / covariance(1.0) that decides p_num, and max(): lane 0, in index order
  {
    float run = 0.0f, best = 0.0f;
    uint32_t p_num = 0, best_i = 0;
    bool open = true;
    for (uint32_t base = 0; base < n; base += kFilterChunk) {
      const uint32_t cnt = min(kFilterChunk, n - base);
      for (uint32_t j = lane; j < cnt; j += 64) s_c[j] = prob[base + j];
      __syncthreads();
      if (lane == 0) {
        auto step = [&](float p, uint32_t i) {
          if (open) {
            run = fadd(run, p);
            ++p_num;
            if (run > 1.0f) open = false;
          }
          if (i == 0) best = p;
          else if (best < p) { best = p; best_i = i; }
        };
        uint32_t j = 0;
        for (; j + kFilterAhead <= cnt; j += kFilterAhead) {
          float v[kFilterAhead];
#pragma unroll
          for (uint32_t a = 0; a < kFilterAhead; ++a) v[a] = s_c[j + a];
#pragma unroll
          for (uint32_t a = 0; a < kFilterAhead; ++a) step(v[a], base + j + a);
        }
        for (; j < cnt; ++j) step(s_c[j], base + j);
      }
      __syncthreads();
    }
    if (lane == 0) { s_num[0] = p_num; s_num[1] = best_i; }
    __syncthreads();
  }
  const uint32_t p_num = s_num[0], best_i = s_num[1];
  // the sums: lanes 0..9 the biased mean's over every particle, lanes 10..19 the unbiased one's over the first p_num
  {
    const uint32_t lim = lane < 10 ? n : p_num;
    float acc = 0.0f;
    for (uint32_t base = 0; base < n; base += kFilterRows) {
      const uint32_t cnt = min(kFilterRows, n - base);
      const float* src = terms + kFilterTerms * (size_t)base;
      for (uint32_t j = lane; j < cnt * kFilterTerms; j += 64) s_t[j] = src[j];
      __syncthreads();
      if (lane < kFilterTerms) {
        const uint32_t rows = lim > base ? min(cnt, lim - base) : 0u;
        uint32_t r = 0;
        for (; r + kFilterAhead <= rows; r += kFilterAhead) {
          float v[kFilterAhead];
#pragma unroll
          for (uint32_t a = 0; a < kFilterAhead; ++a) v[a] = s_t[(r + a) * kFilterTerms + lane];
#pragma unroll
          for (uint32_t a = 0; a < kFilterAhead; ++a) acc = fadd(acc, v[a]);
        }
        for (; r < rows; ++r) acc = fadd(acc, s_t[r * kFilterTerms + lane]);
      }
      __syncthreads();
    }
    if (lane < kFilterTerms) s_sum[lane] = acc;
    __syncthreads();
  }
  if (lane == 0) {
    float e[7];
    filter_mean_from_sums(s_sum + 10, e);
    for (int c = 0; c < 7; ++c) { s_e[c] = e[c]; out->mean_u[c] = e[c]; }
    out->p_num = p_num;
    out->max_index = best_i;
  }
  if (lane < 10) out->sums_b[lane] = s_sum[lane];
  else if (lane < 20) out->sums_u[lane - 10] = s_sum[lane];
  if (lane < 7) out->max_state[lane] = pose[7 * (size_t)best_i + lane];
  else if (lane < 13) out->max_state[lane] = integ[6 * (size_t)best_i + (lane - 7)];
  __syncthreads();
  // covariance: lane (j, k), j <= k < 6; covElement(e, j, k) * probability_, accumulated over the first p_num particles
  {
    uint32_t cj = 0, ck = 0;
    {
      uint32_t at = lane;
      for (cj = 0; cj < 6; ++cj) {
        if (at < 6 - cj) { ck = cj + at; break; }
        at -= 6 - cj;
      }
    }
    const bool mine = lane < 21;
    const float ej = mine ? s_e[cj] : 0.0f, ek = mine ? s_e[ck] : 0.0f;
    float acc = 0.0f;
    for (uint32_t base = 0; base < p_num; base += kFilterRows) {
      const uint32_t cnt = min(kFilterRows, p_num - base);
      const float* src = pose + 7 * (size_t)base;
      for (uint32_t j = lane; j < cnt * 7; j += 64) s_pose[j] = src[j];
      if (lane < cnt) s_p[lane] = prob[base + lane];
      __syncthreads();
      if (mine) {
        auto term = [&](uint32_t r) { return fmul(fmul(fsub(s_pose[r * 7 + ck], ek), fsub(s_pose[r * 7 + cj], ej)), s_p[r]); };
        uint32_t r = 0;
        for (; r + kFilterAhead <= cnt; r += kFilterAhead) {
          float v[kFilterAhead];
#pragma unroll
          for (uint32_t a = 0; a < kFilterAhead; ++a) v[a] = term(r + a);
#pragma unroll
          for (uint32_t a = 0; a < kFilterAhead; ++a) acc = fadd(acc, v[a]);
        }
        for (; r < cnt; ++r) acc = fadd(acc, term(r));
      }
      __syncthreads();
    }
    if (mine) out->cov[lane] = acc / s_sum[10];
  }
}

// resample's map: the accum prefix by one lane, every particle's pick by binary search, the duplicates' noise rows.
//   accum [n] scratch; pick [n] the particle whose state particle i takes; row [n] its noise row or kFilterNoRow
__global__ __launch_bounds__(256) void k_filter_resample_plan(uint32_t n, const float* __restrict__ prob, float u, uint32_t rows,
                                                              float* __restrict__ accum, uint32_t* __restrict__ pick, uint32_t* __restrict__ row,
                                                              FilterRs* __restrict__ rs) {
  __shared__ float s_c[kFilterChunk];
  __shared__ uint32_t s_cnt[256];
  __shared__ float s_total;
  __shared__ uint32_t s_ties, s_end;
  const uint32_t tid = threadIdx.x;
  {
    float acc = 0.0f;
    uint32_t ties = 0;
    for (uint32_t base = 0; base < n; base += kFilterChunk) {
      const uint32_t cnt = min(kFilterChunk, n - base);
      for (uint32_t j = tid; j < cnt; j += 256) s_c[j] = prob[base + j];
      __syncthreads();
      if (tid == 0) {
        auto step = [&](float p, uint32_t j) {
          const float prev = acc;
          acc = fadd(acc, p);
          if (base + j > 0 && acc == prev) ++ties;
          s_c[j] = acc;
        };
        uint32_t j = 0;
        for (; j + kFilterAhead <= cnt; j += kFilterAhead) {
          float v[kFilterAhead];
#pragma unroll
          for (uint32_t a = 0; a < kFilterAhead; ++a) v[a] = s_c[j + a];
#pragma unroll
          for (uint32_t a = 0; a < kFilterAhead; ++a) step(v[a], j + a);
        }
        for (; j < cnt; ++j) step(s_c[j], j);
      }
      __syncthreads();
      for (uint32_t j = tid; j < cnt; j += 256) accum[base + j] = s_c[j];
      __syncthreads();
    }
    if (tid == 0) { s_total = acc; s_ties = ties; s_end = 0; }
    __syncthreads();
  }
  const float pstep = s_total / (float)n;
  const float initial_p = fmul(u, pstep);
  // raw picks: std::lower_bound over the non-decreasing prefix (the lowest index among equal values); n = end()
  for (uint32_t i = tid; i < n; i += 256) {
    const float pscan = fadd(fmul(pstep, (float)i), initial_p);
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (accum[mid] < pscan) lo = mid + 1; else hi = mid;
    }
    row[i] = lo;                                       // (the raw pick, replaced below)
    if (lo == n) atomicAdd(&s_end, 1u);
  }
  __syncthreads();
  // pscan does not decrease with i, so the particles past the end are the last s_end ones; they keep the last valid pick
  const uint32_t n_end = s_end, first_end = n - n_end;
  const uint32_t last_valid = first_end ? row[first_end - 1] : 0u;
  const uint32_t per = (n + 255u) / 256u;
  const uint32_t b0 = min(tid * per, n), b1 = min(b0 + per, n);
  uint32_t dups = 0;
  for (uint32_t i = b0; i < b1; ++i) {
    const uint32_t raw = row[i];
    const uint32_t prev = i ? row[i - 1] : 0u;         // it_prev starts at begin()
    const bool dup = i < first_end && raw == prev;
    pick[i] = i < first_end ? raw : last_valid;
    dups += dup ? 1u : 0u;
  }
  s_cnt[tid] = dups;
  __syncthreads();                                     // (every raw pick has been read: the rows may be written)
  if (tid == 0) {
    uint32_t at = 0;
    for (uint32_t t = 0; t < 256; ++t) { const uint32_t c = s_cnt[t]; s_cnt[t] = at; at += c; }
    rs->n_dup = at; rs->n_at_end = n_end; rs->n_ties = s_ties; rs->ok = at <= rows ? 1u : 0u;
  }
  __syncthreads();
  uint32_t at = s_cnt[tid];
  uint32_t prev = b0 ? pick[b0 - 1] : 0u;
  // (a particle past the end is never a duplicate, and pick[b0 - 1] of a particle before first_end is its raw pick)
  for (uint32_t i = b0; i < b1; ++i) {
    const uint32_t cur = pick[i];
    const bool dup = i < first_end && cur == prev;
    row[i] = dup ? at++ : kFilterNoRow;
    prev = cur;
  }
}

__global__ __launch_bounds__(256) void k_filter_resample_apply(uint32_t n, const FilterRs* __restrict__ rs, const uint32_t* __restrict__ pick,
                                                               const uint32_t* __restrict__ row, const float* __restrict__ rows, float prob,
                                                               FilterGen in, FilterGenOut out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || !rs->ok) return;
  const uint32_t src = pick[i], r = row[i];
  out.prob[i] = prob;
  if (r != kFilterNoRow) {
    filter_add_row(in, src, rows + 10 * (size_t)r, out, i, true);
    return;
  }
  for (int c = 0; c < 7; ++c) out.pose[7 * (size_t)i + c] = in.pose[7 * (size_t)src + c];
  for (int c = 0; c < 6; ++c) out.integ[6 * (size_t)i + c] = in.integ[6 * (size_t)src + c];
  for (int c = 0; c < 4; ++c) out.noise[4 * (size_t)i + c] = in.noise[4 * (size_t)src + c];
}

}  // namespace dddmr

// ---- host (included by rollout_engine.hip after the context) ---------------------------------------------------------
namespace {

struct FilterState {
  dddmr_mcl_filter_config cfg{};
  float lin_tc = 0, ang_tc = 0, var_dist = 0, var_ang = 0;     // as the reference stores them
  uint32_t n = 0;
  bool have = false;                          // set_particles has run
  float *pose[2] = {}, *integ[2] = {}, *noise[2] = {}, *prob[2] = {};
  int g_pose = 0, g_integ = 0, g_noise = 0, g_prob = 0;        // the generation that answers, per array
  float *bias = nullptr, *lik = nullptr, *qual = nullptr, *terms = nullptr, *accum = nullptr, *rows = nullptr;
  uint32_t *pick = nullptr, *row = nullptr;
  FilterOut* out = nullptr;
  FilterRs* rs = nullptr;
  Owned mem;

  FilterGen gen() const { return FilterGen{pose[g_pose], integ[g_integ], noise[g_noise], prob[g_prob]}; }
  FilterGenOut other() const { return FilterGenOut{pose[g_pose ^ 1], integ[g_integ ^ 1], noise[g_noise ^ 1], prob[g_prob ^ 1]}; }
};
static_assert(!std::is_copy_constructible_v<FilterState>);
static_assert(sizeof(dddmr_mcl_filter_config) == 40 && sizeof(dddmr_mcl_filter_estimate) == 368 && sizeof(dddmr_mcl_filter_resample_stats) == 24,
              "the ctypes mirror (_capi.py) pins these sizes");

int filter_alloc(dddmr_rollout_ctx* ctx, FilterState* f) {
  DevAllocs& mem = f->mem.dev;
  const size_t N = f->cfg.max_particles;
  for (int g = 0; g < 2; ++g) {
    HIPCHK(ctx, dev_alloc(mem, &f->pose[g], N * 7));
    HIPCHK(ctx, dev_alloc(mem, &f->integ[g], N * 6));
    HIPCHK(ctx, dev_alloc(mem, &f->noise[g], N * 4));
    HIPCHK(ctx, dev_alloc(mem, &f->prob[g], N));
  }
  HIPCHK(ctx, dev_alloc(mem, &f->bias, N));
  HIPCHK(ctx, dev_alloc(mem, &f->lik, N));
  HIPCHK(ctx, dev_alloc(mem, &f->qual, N));
  HIPCHK(ctx, dev_alloc(mem, &f->terms, N * kFilterTerms));
  HIPCHK(ctx, dev_alloc(mem, &f->accum, N));
  HIPCHK(ctx, dev_alloc(mem, &f->rows, N * 10));
  HIPCHK(ctx, dev_alloc(mem, &f->pick, N));
  HIPCHK(ctx, dev_alloc(mem, &f->row, N));
  HIPCHK(ctx, dev_alloc(mem, &f->out, 1));
  HIPCHK(ctx, dev_alloc(mem, &f->rs, 1));
  return DDDMR_OK;
}

bool filter_finite(const float* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// The entries' common head: tick_mu held by the caller.  `need_particles`: refuse before the first set_particles.
int filter_get(dddmr_rollout_ctx* ctx, const char* what, bool need_particles, MclState** s_out, FilterState** f_out) {
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  MclState* s = ctx->mcl.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_create", what);
  FilterState* f = s->filter.get();
  if (!f) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_filter_create", what);
  if (need_particles && !f->have) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_filter_set_particles", what);
  *s_out = s;
  *f_out = f;
  return DDDMR_OK;
}

inline dim3 filter_grid(uint32_t n) { return dim3((n + 255u) / 256u); }

}  // namespace

extern "C" {

int dddmr_rollout_mcl_filter_create(dddmr_rollout_ctx* ctx, const dddmr_mcl_filter_config* cfg) {
  if (!ctx || !cfg) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_filter_create";
  const double v[4] = {cfg->odom_err_integ_lin_tc, cfg->odom_err_integ_ang_tc, cfg->bias_var_dist, cfg->bias_var_ang};
  for (double d : v)
    if (!std::isfinite(d) || !(d > 0) || !std::isfinite((float)d) || !((float)d > 0.f))
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: the time constants and the bias variances must be finite and positive, as floats too", what);
  if (cfg->max_particles == 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: 0 particles", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
  MclState* s = ctx->mcl.get();
  if (!s) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_create", what);
  if (cfg->max_particles > s->cfg.max_particles)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %u particles, mcl_create's capacity is %u", what, cfg->max_particles, s->cfg.max_particles);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  auto f = std::make_unique<FilterState>();
  f->cfg = *cfg;
  f->lin_tc = (float)cfg->odom_err_integ_lin_tc;
  f->ang_tc = (float)cfg->odom_err_integ_ang_tc;
  f->var_dist = (float)cfg->bias_var_dist;
  f->var_ang = (float)cfg->bias_var_ang;
  const int rc = filter_alloc(ctx, f.get());
  if (rc == DDDMR_OK) s->filter.reset(f.release());      // only a complete state is ever visible; the old one survives a failed create
  return rc;
}

int dddmr_rollout_mcl_filter_set_particles(dddmr_rollout_ctx* ctx, const float* states, const float* probability, const float* noise4, size_t n) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_filter_set_particles";
  if (!states || n == 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: no particle", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s;
  FilterState* f;
  if (const int rc = filter_get(ctx, what, false, &s, &f)) return rc;
  if (n > f->cfg.max_particles) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu particles, capacity %u", what, n, f->cfg.max_particles);
  if (!filter_finite(states, n * 13) || (noise4 && !filter_finite(noise4, n * 4)))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a state or noise component is not finite", what);
  if (probability)
    for (size_t i = 0; i < n; ++i)
      if (!std::isfinite(probability[i]) || probability[i] < 0.f)
        return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: probability %zu is negative or not finite", what, i);
  std::vector<float> pose(n * 7), integ(n * 6), prob(n), nz(n * 4, 0.0f);
  const float p0 = (float)(1.0 / (double)n);             // init: p.probability_ = 1.0 / particles_.size()
  for (size_t i = 0; i < n; ++i) {
    std::memcpy(&pose[7 * i], states + 13 * i, 7 * sizeof(float));
    std::memcpy(&integ[6 * i], states + 13 * i + 7, 6 * sizeof(float));
    prob[i] = probability ? probability[i] : p0;
  }
  if (noise4) std::memcpy(nz.data(), noise4, n * 4 * sizeof(float));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const FilterGenOut o = f->other();
  HIPCHK(ctx, hipMemcpy(o.pose, pose.data(), n * 7 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(o.integ, integ.data(), n * 6 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(o.noise, nz.data(), n * 4 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(o.prob, prob.data(), n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemset(f->bias, 0, n * sizeof(float)));   // Particle(): probability_bias_ = 0.0
  f->g_pose ^= 1; f->g_integ ^= 1; f->g_noise ^= 1; f->g_prob ^= 1;
  f->n = (uint32_t)n;
  f->have = true;
  return DDDMR_OK;
}

int dddmr_rollout_mcl_filter_get_particles(dddmr_rollout_ctx* ctx, float* states_out, float* probability_out, float* bias_out, float* noise4_out,
                                           size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_filter_get_particles";
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s;
  FilterState* f;
  if (const int rc = filter_get(ctx, what, true, &s, &f)) return rc;
  const size_t N = f->n;
  *n = N;
  if (!states_out && !probability_out && !bias_out && !noise4_out) return DDDMR_OK;
  if (capacity < N) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu < %zu particles", what, capacity, N);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const FilterGen g = f->gen();
  if (states_out) {
    std::vector<float> pose(N * 7), integ(N * 6);
    HIPCHK(ctx, hipMemcpy(pose.data(), g.pose, N * 7 * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(integ.data(), g.integ, N * 6 * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) {
      std::memcpy(states_out + 13 * i, &pose[7 * i], 7 * sizeof(float));
      std::memcpy(states_out + 13 * i + 7, &integ[6 * i], 6 * sizeof(float));
    }
  }
  if (probability_out) HIPCHK(ctx, hipMemcpy(probability_out, g.prob, N * sizeof(float), hipMemcpyDeviceToHost));
  if (bias_out) HIPCHK(ctx, hipMemcpy(bias_out, f->bias, N * sizeof(float), hipMemcpyDeviceToHost));
  if (noise4_out) HIPCHK(ctx, hipMemcpy(noise4_out, g.noise, N * 4 * sizeof(float), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

int dddmr_rollout_mcl_filter_predict(dddmr_rollout_ctx* ctx, const float odom_prev[7], const float odom_cur[7], double time_diff) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_filter_predict";
  if (!odom_prev || !odom_cur || !filter_finite(odom_prev, 7) || !filter_finite(odom_cur, 7) || !std::isfinite(time_diff) ||
      !std::isfinite((float)time_diff))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a null or non-finite odometry pose or time_diff", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s;
  FilterState* f;
  if (const int rc = filter_get(ctx, what, true, &s, &f)) return rc;
  const FilterOdom o = filter_set_odoms(odom_prev, odom_cur, (float)time_diff, f->lin_tc, f->ang_tc);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Drain drain{ctx->stream};
  const FilterGenOut out = f->other();
  hipLaunchKernelGGL(k_filter_predict, filter_grid(f->n), dim3(256), 0, ctx->stream, f->n, o, f->gen(), out.pose, out.integ);
  HIPCHK(ctx, hipGetLastError());
  drain.armed = false;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  f->g_pose ^= 1; f->g_integ ^= 1;
  return DDDMR_OK;
}

int dddmr_rollout_mcl_filter_set_noise(dddmr_rollout_ctx* ctx, const float* noise4, size_t n) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_filter_set_noise";
  if (!noise4) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s;
  FilterState* f;
  if (const int rc = filter_get(ctx, what, true, &s, &f)) return rc;
  if (n != f->n) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: %zu rows for %u particles", what, n, f->n);
  if (!filter_finite(noise4, n * 4)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a noise component is not finite", what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemcpy(f->noise[f->g_noise ^ 1], noise4, n * 4 * sizeof(float), hipMemcpyHostToDevice));
  f->g_noise ^= 1;
  return DDDMR_OK;
}

int dddmr_rollout_mcl_filter_reset_integ(dddmr_rollout_ctx* ctx) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s;
  FilterState* f;
  if (const int rc = filter_get(ctx, "mcl_filter_reset_integ", true, &s, &f)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemset(f->integ[f->g_integ ^ 1], 0, (size_t)f->n * 6 * sizeof(float)));   // Vec3(): +0.0f
  f->g_integ ^= 1;
  return DDDMR_OK;
}

int dddmr_rollout_mcl_filter_measure(dddmr_rollout_ctx* ctx, const float* likelihood, const float* quality, size_t n, const float* state_prev,
                                     dddmr_mcl_filter_estimate* estimate, dddmr_mcl_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_filter_measure";
  if (stats) *stats = dddmr_mcl_stats{};
  if (!estimate) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null estimate", what);
  *estimate = dddmr_mcl_filter_estimate{};
  if (!likelihood && quality) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: quality without likelihood", what);
  if (state_prev && !filter_finite(state_prev, 7)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: state_prev is not finite", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s;
  FilterState* f;
  if (const int rc = filter_get(ctx, what, true, &s, &f)) return rc;
  const uint32_t N = f->n;
  float q_min = 1.0f, q_max = 0.0f;
  const float4* obs_dev = nullptr;
  uint32_t n_flat = 0, n_ls = 0;
  if (likelihood) {
    if (n != N) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: %zu likelihoods for %u particles", what, n, N);
    for (size_t i = 0; i < n; ++i)
      if (!std::isfinite(likelihood[i]) || likelihood[i] < 0.f)
        return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: likelihood %zu is negative or not finite", what, i);
    if (quality)
      for (size_t i = 0; i < n; ++i) {                    // src/mcl_3dl.cpp:495-498
        if (q_min > quality[i]) q_min = quality[i];
        if (q_max < quality[i]) q_max = quality[i];
      }
  } else {
    MclObs* o = s->obs.get();
    if (!o) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_set_observation_config", what);
    if (s->cur < 0) return fail(ctx, DDDMR_ERR_STATE, "%s before mcl_set_map", what);
    const int b = o->cur;
    if (o->n_flat[b] + o->n_ls[b] == 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: no observation point (the reference divides 0 by 0)", what);
    obs_dev = o->obs[b]; n_flat = o->n_flat[b]; n_ls = o->n_ls[b];
  }
  const FilterBias bias = filter_bias_plan(state_prev, f->var_dist, f->var_ang);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Drain drain{st};
  const FilterGen g = f->gen();
  float* prob_new = f->prob[f->g_prob ^ 1];
  uint32_t launches = 4;
  if (likelihood) {
    HIPCHK(ctx, hipMemcpyAsync(f->lik, likelihood, (size_t)N * sizeof(float), hipMemcpyHostToDevice, st));
  } else {
    mcl_launch(ctx, s, obs_dev, n_flat, n_ls, g.pose, N, f->lik, f->qual);
    launches += 3;
  }
  hipLaunchKernelGGL(k_filter_weigh, filter_grid(N), dim3(256), 0, st, N, g.prob, f->lik, prob_new);
  hipLaunchKernelGGL(k_filter_sum, dim3(1), dim3(256), 0, st, N, prob_new, f->out);
  hipLaunchKernelGGL(k_filter_terms, filter_grid(N), dim3(256), 0, st, N, g.prob, prob_new, f->out, g.pose, bias, f->bias, f->terms);
  hipLaunchKernelGGL(k_filter_reduce, dim3(1), dim3(64), 0, st, N, prob_new, f->terms, g.pose, g.integ, f->out);
  HIPCHK(ctx, hipGetLastError());
  FilterOut r;
  HIPCHK(ctx, hipMemcpyAsync(&r, f->out, sizeof(r), hipMemcpyDeviceToHost, st));
  drain.armed = false;
  HIPCHK(ctx, hipStreamSynchronize(st));                 // the one wait
  if (!likelihood) {
    const MclResult m = *s->res_host;
    q_min = m.q_min; q_max = m.q_max;
    if (stats) {
      stats->quality_min = m.q_min; stats->quality_max = m.q_max;
      stats->n_bad_states = m.n_bad; stats->n_over_capacity = m.n_over; stats->max_ground_neighbours_seen = m.max_ground;
      stats->launches = 3; stats->host_waits = 1;
    }
    s->last_n = m.n_over ? 0 : N;
    if (m.n_over)
      return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %u particles with more than max_ground_neighbours %u ground points inside the radius (up to %u)",
                  what, m.n_over, s->cfg.max_ground_neighbours, m.max_ground);
  }
  f->g_prob ^= 1;
  dddmr_mcl_filter_estimate& e = *estimate;
  filter_mean_from_sums(r.sums_b, e.mean_biased);
  std::memcpy(e.mean, r.mean_u, sizeof(e.mean));
  std::memcpy(e.max_state, r.max_state, sizeof(e.max_state));
  e.max_index = r.max_index;
  for (int j = 0, at = 0; j < 6; ++j)
    for (int k = j; k < 6; ++k, ++at) e.cov[6 * j + k] = e.cov[6 * k + j] = r.cov[at];
  std::memcpy(e.sums_biased, r.sums_b, sizeof(e.sums_biased));
  std::memcpy(e.sums, r.sums_u, sizeof(e.sums));
  e.weight_sum = r.weight_sum;
  e.bias_sum = r.sums_b[0];
  e.p_num = r.p_num;
  e.restored = r.restored;
  e.quality_min = q_min; e.quality_max = q_max;
  e.launches = launches; e.host_waits = 1;
  return DDDMR_OK;
}

int dddmr_rollout_mcl_filter_resample(dddmr_rollout_ctx* ctx, double u, const float* noise, size_t rows, dddmr_mcl_filter_resample_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_filter_resample";
  if (stats) *stats = dddmr_mcl_filter_resample_stats{};
  const float uf = (float)u;
  if (!(u >= 0.0 && u < 1.0) || !(uf < 1.0f)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: u must lie in [0, 1), as a float too", what);
  if (rows && !noise) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null noise rows", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s;
  FilterState* f;
  if (const int rc = filter_get(ctx, what, true, &s, &f)) return rc;
  const uint32_t N = f->n;
  const size_t used = std::min<size_t>(rows, N);         // (there are never more duplicates than particles)
  if (!filter_finite(noise, used * 10)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a noise component is not finite", what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Drain drain{st};
  if (used) HIPCHK(ctx, hipMemcpyAsync(f->rows, noise, used * 10 * sizeof(float), hipMemcpyHostToDevice, st));
  const FilterGen g = f->gen();
  hipLaunchKernelGGL(k_filter_resample_plan, dim3(1), dim3(256), 0, st, N, g.prob, uf, (uint32_t)used, f->accum, f->pick, f->row, f->rs);
  hipLaunchKernelGGL(k_filter_resample_apply, filter_grid(N), dim3(256), 0, st, N, f->rs, f->pick, f->row, f->rows, (float)(1.0 / (double)N), g,
                     f->other());
  HIPCHK(ctx, hipGetLastError());
  FilterRs r;
  HIPCHK(ctx, hipMemcpyAsync(&r, f->rs, sizeof(r), hipMemcpyDeviceToHost, st));
  drain.armed = false;
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (stats) {
    stats->n_duplicates = r.n_dup; stats->n_at_end = r.n_at_end; stats->n_ties = r.n_ties;
    stats->launches = 2; stats->host_waits = 1;
  }
  if (!r.ok) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %u duplicates, %zu noise rows", what, r.n_dup, rows);
  f->g_pose ^= 1; f->g_integ ^= 1; f->g_noise ^= 1; f->g_prob ^= 1;
  return DDDMR_OK;
}

int dddmr_rollout_mcl_filter_add_noise(dddmr_rollout_ctx* ctx, const float* noise, size_t n) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "mcl_filter_add_noise";
  if (!noise) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: null argument", what);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  MclState* s;
  FilterState* f;
  if (const int rc = filter_get(ctx, what, true, &s, &f)) return rc;
  if (n != f->n) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: %zu rows for %u particles", what, n, f->n);
  if (!filter_finite(noise, n * 10)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: a noise component is not finite", what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Drain drain{st};
  HIPCHK(ctx, hipMemcpyAsync(f->rows, noise, n * 10 * sizeof(float), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_filter_add_noise, filter_grid(f->n), dim3(256), 0, st, f->n, f->gen(), f->rows, f->other());
  HIPCHK(ctx, hipGetLastError());
  drain.armed = false;
  HIPCHK(ctx, hipStreamSynchronize(st));
  f->g_pose ^= 1; f->g_integ ^= 1; f->g_noise ^= 1;
  return DDDMR_OK;
}

}  // extern "C"
