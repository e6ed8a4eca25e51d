// perception_stack.hip.h -- the perception stack over the device layers of a context: one doClear_then_Mark pass of
// StackedPerception (src/dddmr_perception_3d/src/stacked_perception.cpp:72-90) with each layer on its own sensor's
// observation, then the stacked minimum dGraph (get_min_dGraphValue, :114-126), the lethal masks (aggregateLethal,
// :142-155) and the list of ground nodes whose stacked value or mask changed in this pass.  include/dddmr_rollout.h
// restates the semantics.
//
// The layers are not copied: the lidar pass is marking_update_on (marking_host.hip.h), the depth pass
// depth_layer_update_locked (depth_layer.hip.h), the very functions the stand-alone entries call.
//
// Locks, always in this order: tick_mu (the stack itself, the lidar layer, the context's stream) -> producer_mu (the depth
// layer, the feeds' stream) -> cloud_mu (short: pinning the aggregate and reading what it was published from).  The lidar
// observation is cut out of the PINNED aggregate with the per-source counts publish_cloud recorded under cloud_mu, so a
// concurrent set_scan_source cannot tear it: it fills another buffer.  producer_mu is taken after the lidar pass and held
// over the depth pass, the min kernel and its wait, so neither layer's arrays move under the kernel.
//
// Streams: the lidar pass runs on the context's stream, the depth pass on the feeds' stream, one after the other; both
// end with a host wait of their own, so k_stack_min (context's stream) needs no event.  One more wait brings the change
// count back; the change list itself is written by the kernel into host-mapped memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "depth_layer.hip.h"    // DepthLayerState, depth_layer_update_locked
#include "dev_memory.hip.h"     // Owned, dev_alloc, Drain
#include "marking_host.hip.h"   // MarkingState, marking_update_on
#include "wave_ops.hip.h"       // wave_append

namespace dddmr {

constexpr int kStackMaxLayers = DDDMR_STACK_MAX_LAYERS;
constexpr double kStackStart = 99999.9;          // get_min_dGraphValue's tmp (stacked_perception.cpp:116)

struct MinStackArgs {
  const double* value[kStackMaxLayers];          // in layer order; null: an unset host slot
  const uint8_t* lethal[kStackMaxLayers];        // null: a host layer
  uint32_t n_layers;
  uint32_t n_nodes;                              // n_ground + 1
  uint32_t cap;                                  // entries the change list takes
  double* min_pub;                               // [n_nodes] published stacked dGraph
  uint8_t* mask_pub;                             // [n_nodes]
  uint32_t* chg_node;                            // [cap] host-mapped
  double* chg_value;                             // [cap]
  uint8_t* chg_mask;                             // [cap]
  uint32_t* n_changed;                           // device counter, zero at launch
};

// One lane per ground node (grid-stride by whole waves, so every lane of a wave makes the same trips and the ballot is
// complete).  Changed nodes are appended with one counter add per wave; lanes past the capacity count but do not store.
__global__ __launch_bounds__(256) void k_stack_min(MinStackArgs a) {
  const int lane = threadIdx.x & 63;
  for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < a.n_nodes; base += gridDim.x * 256u) {
    const uint32_t i = base + (uint32_t)lane;
    const bool valid = i < a.n_nodes;
    double v = kStackStart;
    uint32_t mask = 0;
    bool changed = false;
    if (valid) {
#pragma unroll
      for (int l = 0; l < kStackMaxLayers; ++l) {
        if ((uint32_t)l < a.n_layers) {
          if (a.value[l]) {
            const double x = a.value[l][i];
            v = (x < v) ? x : v;                       // std::min(tmp, x): not fmin, a NaN leaves v alone
          }
          if (a.lethal[l] && a.lethal[l][i]) mask |= 1u << l;
        }
      }
      changed = __double_as_longlong(v) != __double_as_longlong(a.min_pub[i]) || mask != (uint32_t)a.mask_pub[i];
      if (changed) {
        a.min_pub[i] = v;
        a.mask_pub[i] = (uint8_t)mask;
      }
    }
    const uint32_t at = wave_append(changed, a.n_changed);
    if (changed && at < a.cap) {
      a.chg_node[at] = i;
      a.chg_value[at] = v;
      a.chg_mask[at] = (uint8_t)mask;
    }
  }
}

}  // namespace dddmr

// ---- host ---------------------------------------------------------------------------------------------------------
namespace {

struct StackState {
  dddmr_stack_config cfg{};
  uint32_t n_nodes = 0;
  double* min_pub = nullptr;                 // device
  uint8_t* mask_pub = nullptr;
  double* host_layer[DDDMR_STACK_MAX_HOST] = {};     // device, allocated with the stack; host_set says which take part
  bool host_set[DDDMR_STACK_MAX_HOST] = {};
  uint32_t* n_changed_dev = nullptr;
  float4* lidar_obs = nullptr;               // gather buffer for lidar sources that are not neighbours in the aggregate (lazy)
  Owned mem;
  // host-mapped: uint32 count | pad | double value[cap] | uint32 node[cap] | uint8 mask[cap]
  char *list_host = nullptr, *list_dev = nullptr;
  uint32_t n_changed = 0;                    // of the last update (true count)
};

static_assert(!std::is_copy_constructible_v<StackState>);

StackState* stack_of(dddmr_rollout_ctx* ctx, const char* what) {
  if (!ctx->stack) (void)fail(ctx, DDDMR_ERR_STATE, "%s before stack_create (or after a later marking_create / depth_layer_create)", what);
  return ctx->stack.get();
}

size_t stack_cap(const StackState* s) { return std::max<size_t>(s->cfg.max_changes, 1); }
double* stack_list_value(const StackState* s, char* base) { return reinterpret_cast<double*>(base + 8); }
uint32_t* stack_list_node(const StackState* s, char* base) { return reinterpret_cast<uint32_t*>(base + 8 + 8 * stack_cap(s)); }
uint8_t* stack_list_mask(const StackState* s, char* base) { return reinterpret_cast<uint8_t*>(base + 8 + 12 * stack_cap(s)); }

// A host slot for a layer that fills it device to device (static_layer_bind): its array, null for a slot out of range;
// and the mark stack_set_host_layer leaves once the values are in.
double* stack_host_slot(StackState* s, int slot) { return slot >= 0 && slot < s->cfg.n_host_layers ? s->host_layer[slot] : nullptr; }
void stack_host_slot_set(StackState* s, int slot) { s->host_set[slot] = true; }

// The stacked arrays from the layers as they are now, on the context's stream, and the wait for it.  tick_mu held, and
// producer_mu when the stack has a depth layer.  publish_only: after create / reset -- the change list comes out empty.
int stack_recompute(dddmr_rollout_ctx* ctx, StackState* s, bool publish_only, uint32_t* ops) {
  MinStackArgs a{};
  for (int p = 0; p < s->cfg.n_order; ++p) {
    const int id = s->cfg.layer_order[p];
    if (id == DDDMR_STACK_LIDAR) { a.value[p] = ctx->marking->store.s.dgraph; a.lethal[p] = ctx->marking->store.s.lethal; }
    else if (id == DDDMR_STACK_DEPTH) { a.value[p] = ctx->dlayer->store.s.dgraph; a.lethal[p] = ctx->dlayer->store.s.lethal; }
    else if (s->host_set[id - DDDMR_STACK_HOST0]) a.value[p] = s->host_layer[id - DDDMR_STACK_HOST0];
  }
  a.n_layers = (uint32_t)s->cfg.n_order;
  a.n_nodes = s->n_nodes;
  a.cap = publish_only ? 0u : s->cfg.max_changes;
  a.min_pub = s->min_pub;
  a.mask_pub = s->mask_pub;
  a.chg_value = stack_list_value(s, s->list_dev);
  a.chg_node = stack_list_node(s, s->list_dev);
  a.chg_mask = stack_list_mask(s, s->list_dev);
  a.n_changed = s->n_changed_dev;
  hipStream_t st = ctx->stream;
  Drain drain{st};                           // an error exit leaves nothing running that writes the state's arrays
  HIPCHK(ctx, hipMemsetAsync(s->n_changed_dev, 0, sizeof(uint32_t), st));
  const uint32_t blocks = std::min<uint32_t>((s->n_nodes + 255u) / 256u, 2048u);
  hipLaunchKernelGGL(k_stack_min, dim3(blocks), dim3(256), 0, st, a);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(s->list_host, s->n_changed_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  drain.armed = false;
  if (ops) *ops += 3;
  s->n_changed = publish_only ? 0u : *reinterpret_cast<const uint32_t*>(s->list_host);
  return DDDMR_OK;
}

}  // namespace

extern "C" {

int dddmr_rollout_stack_create(dddmr_rollout_ctx* ctx, const dddmr_stack_config* cfg) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!cfg) return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_create: null config");
  if (cfg->n_host_layers < 0 || cfg->n_host_layers > DDDMR_STACK_MAX_HOST || cfg->n_ground >= (1u << 30))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_create: %d host layers (at most %d), n_ground %u", cfg->n_host_layers, DDDMR_STACK_MAX_HOST, cfg->n_ground);
  if (cfg->max_changes > (1u << 28)) return fail(ctx, DDDMR_ERR_CAPACITY, "stack_create: max_changes %u", cfg->max_changes);
  // layer_order: every layer of the stack exactly once
  const int n_layers = (cfg->use_lidar_layer != 0) + (cfg->use_depth_layer != 0) + cfg->n_host_layers;
  bool seen[DDDMR_STACK_MAX_LAYERS] = {};
  bool order_ok = cfg->n_order == n_layers;
  for (int p = 0; order_ok && p < n_layers; ++p) {
    const int id = cfg->layer_order[p];
    order_ok = id >= 0 && id < DDDMR_STACK_MAX_LAYERS && !seen[id] &&
               (id == DDDMR_STACK_LIDAR ? cfg->use_lidar_layer != 0 : id == DDDMR_STACK_DEPTH ? cfg->use_depth_layer != 0 : id - DDDMR_STACK_HOST0 < cfg->n_host_layers);
    if (order_ok) seen[id] = true;
  }
  if (!order_ok) return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_create: layer_order must name each of the stack's %d layers exactly once", n_layers);
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "stack_create while a tick_begin is pending");
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if (cfg->use_lidar_layer) {
    if (!ctx->marking) return fail(ctx, DDDMR_ERR_STATE, "stack_create: the lidar layer is asked for before marking_create");
    if (ctx->marking->store.n_ground != cfg->n_ground)
      return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_create: n_ground %u, the lidar layer has %u", cfg->n_ground, ctx->marking->store.n_ground);
  }
  if (cfg->use_depth_layer) {
    if (!ctx->dlayer) return fail(ctx, DDDMR_ERR_STATE, "stack_create: the depth layer is asked for before depth_layer_create");
    if (ctx->dlayer->store.n_ground != cfg->n_ground)
      return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_create: n_ground %u, the depth layer has %u", cfg->n_ground, ctx->dlayer->store.n_ground);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  auto s = std::make_unique<StackState>();
  s->cfg = *cfg;
  s->n_nodes = cfg->n_ground + 1;
  DevAllocs& mem = s->mem.dev;
  HIPCHK(ctx, dev_alloc(mem, &s->min_pub, s->n_nodes));
  HIPCHK(ctx, dev_alloc(mem, &s->mask_pub, s->n_nodes));
  HIPCHK(ctx, dev_alloc(mem, &s->n_changed_dev, 1));
  for (int i = 0; i < cfg->n_host_layers; ++i) HIPCHK(ctx, dev_alloc(mem, &s->host_layer[i], s->n_nodes));
  const size_t bytes = 8 + 13 * stack_cap(s.get());
  if (host_mapped_alloc(s->mem.host, &s->list_host, &s->list_dev, bytes) != 0) return fail(ctx, DDDMR_ERR_HIP, "stack_create: change list of %zu bytes", bytes);
  // (the published arrays start as a pattern no result has, so the first pass writes every node)
  Drain drain{ctx->stream};                              // behind `s`: an error exit waits for the memsets before the state dies
  HIPCHK(ctx, hipMemsetAsync(s->min_pub, 0xFF, (size_t)s->n_nodes * sizeof(double), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(s->mask_pub, 0xFF, s->n_nodes, ctx->stream));
  const int rc = stack_recompute(ctx, s.get(), true, nullptr);
  drain.armed = false;                                   // (stack_recompute has waited, or drained)
  if (rc == DDDMR_OK) ctx->stack.reset(s.release());     // only a complete state is ever visible; the old one survives a failed create
  return rc;
}

int dddmr_rollout_stack_set_host_layer(dddmr_rollout_ctx* ctx, int32_t slot, const double* values) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StackState* s = stack_of(ctx, "stack_set_host_layer");
  if (!s) return DDDMR_ERR_STATE;
  if (slot < 0 || slot >= s->cfg.n_host_layers) return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_set_host_layer: slot %d of %d", slot, s->cfg.n_host_layers);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (values) HIPCHK(ctx, hipMemcpy(s->host_layer[slot], values, (size_t)s->n_nodes * sizeof(double), hipMemcpyHostToDevice));
  s->host_set[slot] = values != nullptr;
  return DDDMR_OK;
}

int dddmr_rollout_stack_update(dddmr_rollout_ctx* ctx, const double T_base_sensor[7], const double T_gbl_base[7],
                               dddmr_stack_stats* stats) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!stats) return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_update: null stats");
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StackState* s = stack_of(ctx, "stack_update");
  if (!s) return DDDMR_ERR_STATE;
  const bool lidar = s->cfg.use_lidar_layer != 0, depth = s->cfg.use_depth_layer != 0;
  if ((lidar && !T_base_sensor) || ((lidar || depth) && !T_gbl_base)) return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_update: null transform");
  if (depth)
    for (int i = 0; i < 7; ++i)
      if (!std::isfinite(T_gbl_base[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "stack_update: non-finite transform");
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "stack_update while a tick_begin is pending");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  dddmr_stack_stats out{};
  uint32_t ops = 0;
  // ---- lidar layer, on the lidar sources' segments of the pinned aggregate ----
  if (lidar) {
    MarkingState* m = ctx->marking.get();
    auto pass = [&]() -> int {
      CloudPin pin(ctx);
      Drain drain{ctx->stream, false};                   // behind the pin: armed by the gather copies, which read the pinned aggregate
      const int cidx = pin.idx();
      m->cur = ctx->stream;
      HIPCHK(ctx, pin.wait_on(m->cur));
      SourceLayout L;
      {
        std::lock_guard<std::mutex> lk(ctx->cloud_mu);
        L = ctx->cloud_layout[cidx];
      }
      if (!L.from_sources)
        return fail(ctx, DDDMR_ERR_STATE, "stack_update: the published aggregate did not come from the sources (a set_cloud since the last feed)");
      // maximal runs of lidar points in the aggregate
      struct Run { uint32_t at, n; } runs[DDDMR_MAX_SOURCES];
      int n_runs = 0;
      uint32_t total = 0;
      for (int i = 0; i < DDDMR_MAX_SOURCES; ++i) {
        if (!((L.lidar_mask >> i) & 1u) || !L.n[i]) continue;
        if (n_runs && runs[n_runs - 1].at + runs[n_runs - 1].n == L.at[i]) runs[n_runs - 1].n += L.n[i];
        else runs[n_runs++] = Run{L.at[i], L.n[i]};
        total += L.n[i];
      }
      if (L.total > ctx->cloud_n[cidx]) return fail(ctx, DDDMR_ERR_STATE, "stack_update: source counts %u beyond the aggregate's %u points", L.total, ctx->cloud_n[cidx]);
      const float4* obs = ctx->cloud_dev[cidx] + (n_runs ? runs[0].at : 0u);
      if (n_runs > 1) {
        if (!s->lidar_obs) HIPCHK(ctx, dev_alloc(s->mem.dev, &s->lidar_obs, (size_t)std::max<uint32_t>(ctx->cfg.max_points, 1)));
        uint32_t to = 0;
        drain.armed = true;
        for (int r = 0; r < n_runs; ++r) {
          HIPCHK(ctx, hipMemcpyAsync(s->lidar_obs + to, ctx->cloud_dev[cidx] + runs[r].at, (size_t)runs[r].n * sizeof(float4), hipMemcpyDeviceToDevice, m->cur));
          to += runs[r].n;
          ++ops;
        }
        obs = s->lidar_obs;
      }
      const int rc = marking_update_on(ctx, m, obs, total, T_base_sensor, T_gbl_base, &out.lidar);
      drain.armed = drain.armed && rc != DDDMR_OK;       // (a successful update has waited for the stream)
      return rc;
    };
    out.lidar_rc = pass();
    ops += m->launches_last;
    out.host_waits += 1;
  }
  // ---- depth layer; from here on its arrays stay put until the stacked arrays are published ----
  std::unique_lock<std::mutex> prod(ctx->producer_mu, std::defer_lock);
  if (depth) {
    prod.lock();
    if (!ctx->sources.depth_frustums_ready()) {
      out.depth_skipped = 1;                             // isFirstScanReady: the plugin returns early, the stack goes on
    } else {
      out.depth_rc = depth_layer_update_locked(ctx, T_gbl_base, &out.depth);
      ops += out.depth.launches;
      out.host_waits += out.depth.host_waits;
    }
  }
  // ---- stacked arrays and change list, whatever the layers returned ----
  const int rc = stack_recompute(ctx, s, false, &ops);
  out.host_waits += 1;
  out.n_changed = s->n_changed;
  out.launches = ops;
  *stats = out;
  if (rc != DDDMR_OK) return rc;
  if (out.lidar_rc != DDDMR_OK) return out.lidar_rc;
  return out.depth_rc;
}

int dddmr_rollout_stack_get_changes(dddmr_rollout_ctx* ctx, uint32_t* node_out, double* value_out, uint8_t* lethal_mask_out,
                                    size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StackState* s = stack_of(ctx, "stack_get_changes");
  if (!s) return DDDMR_ERR_STATE;
  const size_t c = s->n_changed;
  *n = c;
  if (c > s->cfg.max_changes) return fail(ctx, DDDMR_ERR_CAPACITY, "stack_get_changes: %zu changes, max_changes %u", c, s->cfg.max_changes);
  if (!node_out && !value_out && !lethal_mask_out) return DDDMR_OK;
  if (c > capacity) return fail(ctx, DDDMR_ERR_CAPACITY, "stack_get_changes: capacity %zu < %zu", capacity, c);
  if (node_out) std::memcpy(node_out, stack_list_node(s, s->list_host), c * sizeof(uint32_t));
  if (value_out) std::memcpy(value_out, stack_list_value(s, s->list_host), c * sizeof(double));
  if (lethal_mask_out) std::memcpy(lethal_mask_out, stack_list_mask(s, s->list_host), c);
  return DDDMR_OK;
}

int dddmr_rollout_stack_get_min_dgraph(dddmr_rollout_ctx* ctx, double* values_out, size_t capacity) {
  if (!ctx || !values_out) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StackState* s = stack_of(ctx, "stack_get_min_dgraph");
  if (!s) return DDDMR_ERR_STATE;
  if (capacity < s->n_nodes) return fail(ctx, DDDMR_ERR_CAPACITY, "stack_get_min_dgraph: capacity %zu < %u", capacity, s->n_nodes);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpy(values_out, s->min_pub, (size_t)s->n_nodes * sizeof(double), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

int dddmr_rollout_stack_get_lethal_mask(dddmr_rollout_ctx* ctx, uint8_t* mask_out, size_t capacity) {
  if (!ctx || !mask_out) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StackState* s = stack_of(ctx, "stack_get_lethal_mask");
  if (!s) return DDDMR_ERR_STATE;
  if (capacity < s->n_nodes) return fail(ctx, DDDMR_ERR_CAPACITY, "stack_get_lethal_mask: capacity %zu < %u", capacity, s->n_nodes);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpy(mask_out, s->mask_pub, s->n_nodes, hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

int dddmr_rollout_stack_get_lethal_nodes(dddmr_rollout_ctx* ctx, uint32_t* node_out, size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StackState* s = stack_of(ctx, "stack_get_lethal_nodes");
  if (!s) return DDDMR_ERR_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint8_t> mask(s->n_nodes);
  HIPCHK(ctx, hipMemcpy(mask.data(), s->mask_pub, s->n_nodes, hipMemcpyDeviceToHost));
  size_t total = 0;
  for (int p = 0; p < s->cfg.n_order; ++p) {
    if (s->cfg.layer_order[p] >= DDDMR_STACK_HOST0) continue;
    for (uint32_t i = 0; i < s->cfg.n_ground; ++i)
      if ((mask[i] >> p) & 1u) {
        if (node_out && total < capacity) node_out[total] = i;
        ++total;
      }
  }
  *n = total;
  if (node_out && total > capacity) return fail(ctx, DDDMR_ERR_CAPACITY, "stack_get_lethal_nodes: capacity %zu < %zu", capacity, total);
  return DDDMR_OK;
}

int dddmr_rollout_stack_reset(dddmr_rollout_ctx* ctx) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  StackState* s = stack_of(ctx, "stack_reset");
  if (!s) return DDDMR_ERR_STATE;
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "stack_reset while a tick_begin is pending");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc = DDDMR_OK;
  if (s->cfg.use_lidar_layer) rc = marking_reset_locked(ctx, ctx->marking.get());
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if (s->cfg.use_depth_layer) {
    const int rd = store_reset(ctx, ctx->dlayer->store, ctx->copy_stream, ctx->dlayer->cfg.max_obstacle_distance);
    if (rc == DDDMR_OK) rc = rd;
  }
  const int rr = stack_recompute(ctx, s, true, nullptr);
  return rc != DDDMR_OK ? rc : rr;
}

}  // extern "C"
