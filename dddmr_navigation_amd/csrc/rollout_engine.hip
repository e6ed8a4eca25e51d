// rollout_engine.hip -- context, host-side theory initialisation and the C-ABI
// (include/dddmr_rollout.h) of the MI355X local-planner rollout engine.
//
// Host responsibilities (cheap, per tick): planning the tick (tick_plan.hip.h: the theory's initialise(), the local
// costmap tile, the launch shapes) and launching the five kernels of rollout_kernels.hip.h.
// Everything proportional to N_traj x N_steps or to the cloud runs on the GPU.
// Here: the context, create / destroy, the cloud triple buffer, the tick and its read-backs.  The multi-rank exchange is
// in rollout_comm.hip.h, the diagnostics in rollout_diag.hip.h, the sensor sources and the modules in the headers
// included at the end.
//
// Citations are relative to /root/reference/src/dddmr_local_planner/.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and enums only: the library is dlopen()ed by dddmr_rollout_comm_init

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dddmr_rollout.h"

// fail() (below, behind the context) and HIPCHK, ahead of the headers: point_grid.hip.h's grid_build reports through them
namespace { int fail(dddmr_rollout_ctx* ctx, int code, const char* fmt, ...); }
#define HIPCHK(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, DDDMR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                      \
  } while (0)

#include "dev_memory.hip.h"   // DevAllocs, DevScope, Drain: the context's memory, the diagnostics' temporaries
#include "rollout_kernels.hip.h"
#include "tick_plan.hip.h"
#include "perception_kernels.hip.h"
#include "depth_feed.hip.h"
#include "depth_image.hip.h"
#include "depth_clear.hip.h"
#include "lidar_sweep.hip.h"
#include "lidar_features.hip.h"
#include "measure_kernels.hip.h"
#include "point_grid_plan.hip.h"   // cloud_arg_ok
#include "source_table.hip.h"

using namespace dddmr;

namespace {

constexpr int kCloudBufs = 3;              // front / busy / free, see dddmr_rollout_ctx

// The module states, defined in the headers included at the end.  Each frees what it owns when it dies, and dies only
// while the context's device is current: in its module's create (after hipSetDevice) and in dddmr_rollout_destroy.
struct MarkingState;                       // global-mode marking / clearing layer, marking_host.hip.h
struct DepthMarkState;                     // the depth camera's selfMark, depth_mark.hip.h
struct DepthLayerState;                    // the depth camera layer's store, dGraph and lethal set, depth_layer.hip.h
struct StackState;                         // the perception stack over the two layers, perception_stack.hip.h
struct MclState;                           // the particle filter's lidar likelihood, mcl_measure.hip.h
struct StaticLayerState;                   // the static and no-entry layers' sGraph and dGraphs, static_layer.hip.h
struct GlobalPlanState;                    // the pre-graph global planner's A* over them, global_plan.hip.h
struct GpCloudState;                       // what the default A* on the ground cloud keeps beside it, global_plan_cloud.hip.h
template <class T>
using ModuleSlot = std::unique_ptr<T, LateDelete<T>>;   // enters its slot once complete (each module's create)

// What a sensor source owns, beside its record in the context's SourceTable (sensor_sources.hip.h keeps the two in step).
// Each state frees its memory when it dies: assigning an empty SourceOwned tears the source down (release_source).
struct SourceOwned {
  std::unique_ptr<PerceptionScratch> feed; // scan sources above 0: stitcher state and staging (source 0 feeds through ctx->feed)
  std::unique_ptr<DepthSource> depth;      // depth sources
  std::unique_ptr<DepthImage> dimg;        // ... that are fed images
  std::unique_ptr<LidarSweep> sweep;       // sweep sources
  Owned scan_obs;                          // a scan source's observation buffer, made by its first feed
  // the latest observation on the device, an alias: of the buffer in scan_obs, of the depth source's current frame buffer
  // or of the sweep's current observation buffer
  float4* obs = nullptr;
  DcFrustum frustum{};                     // depth sources: valid while the record says has_frustum
};

}  // namespace

struct dddmr_rollout_ctx {
  dddmr_rollout_config cfg{};
  std::vector<dddmr_theory_config> theories;
  int device = 0;
  hipStream_t stream = nullptr, copy_stream = nullptr;
  DevAllocs mem;           // every device allocation of the context itself (the modules and sources own theirs)
  HostAllocs host;         // ... and its pinned host memory
  // k_rollout state arrays, grown on demand: [n_local][max steps of the tick] (of st_sc a tick with shared heading rows
  // fills only the first nth rows, one per angular sample)
  TrajInfo* traj_info = nullptr;
  double2* st_sc = nullptr;
  float2* st_xy = nullptr;
  double2* st_pp = nullptr;   // per trajectory: pure pursuit (distance, folded yaw) on its last pose, from the rollout
  size_t st_cap = 0;       // (trajectory, step) pairs the state arrays hold
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evs0 = nullptr, evs1 = nullptr, cloud_ready[kCloudBufs] = {nullptr, nullptr, nullptr};

  // device memory
  float4* cloud_dev[kCloudBufs] = {nullptr, nullptr, nullptr};
  uint32_t cloud_n[kCloudBufs] = {0, 0, 0};
  // where a published aggregate came from (recorded by publish_cloud under cloud_mu; nothing published yet: the sources'
  // empty aggregate).  What the perception stack cuts the lidar sources' observation out of a pinned aggregate with.
  SourceLayout cloud_layout[kCloudBufs];
  uint2* pt_slot = nullptr;
  Pt3* sorted = nullptr;
  uint32_t *cell_count = nullptr, *cell_start = nullptr;
  uint32_t* row_tab = nullptr;       // compact row-run index of the tick's grid (k_bin_scatter -> k_score)
  float* axes_dev = nullptr;
  float4* samples_dev = nullptr;
  float4* plan_dev = nullptr;
  float* plan_pairs_dev = nullptr;     // the same poses as pair records, padded: phase P's scalar walk (plan_pack_pairs)
  double* costs = nullptr;
  TrajPartial* partial = nullptr;      // per local trajectory: what k_score hands k_finalize on a multi-round shard
  int32_t* steps = nullptr;
  float4* samples_out = nullptr;
  int64_t* best_key = nullptr;
  uint32_t* overflow = nullptr;
  DevResult* result_dev = nullptr;   // device alias of result_host (host-mapped)
  uint32_t* tickets = nullptr;       // [0] binning ticket, [1] scoring ticket
  // load feedback (device): per-trajectory load of the last tick, tile assignment of this one
  float4* blocked_plan = nullptr;      // PathBlockedStrategy scratch: kBlockedMaxPlan points, a flag bit each
  uint32_t* blocked_flags = nullptr;
  uint32_t* traj_load = nullptr;
  uint32_t* assign = nullptr;
  TickFeedback feedback;     // what traj_load describes, and the collided share of the last tick
  TickKnobs knobs;           // what create read from the environment and the device for plan_tick
  // DDDMR_POISON=1 (tests): fill the per-trajectory outputs with NaN / -1 patterns before every
  // tick, so a trajectory the scorer skipped cannot pass for scored with last tick's values
  bool poison = false;
  // DDDMR_HOST_PROF=1: host-side time of the tick's stages, printed at destroy
  bool host_prof = false;
  bool debug_grid = false;   // DDDMR_DEBUG_GRID: the third tick prints its k_score shape
  int ceil_blocks = 0;       // DDDMR_CEIL_BLOCKS: workgroups of the stream-ceiling kernels (0: sized by the buffers)
  double prof_ns[4] = {0, 0, 0, 0};
  uint64_t prof_n = 0;
  double* poses_dev = nullptr;
  // perception feed scratch
  PerceptionScratch feed{};
  // The sensor sources feeding one aggregate: the bookkeeping and its rules in source_table.hip.h, the entry points in
  // sensor_sources.hip.h.  Both under producer_mu.
  static constexpr int kMaxSources = DDDMR_MAX_SOURCES;
  SourceTable sources;
  SourceOwned src[kMaxSources];
  std::unique_ptr<DepthClear> dclear;   // the clearing verdicts' scratch (depth_clear.hip.h), allocated by the first verdict / point-test call

  // pinned host memory
  float4* cloud_stage[kCloudBufs] = {nullptr, nullptr, nullptr};   // pinned staging, one per device cloud buffer
  float* small_stage = nullptr;  // axes / sample list / plan / scan upload
  DevResult* result_host = nullptr;

  // prune plan (host copy)
  uint32_t plan_m = 0;
  double plan_last[7] = {0, 0, 0, 0, 0, 0, 1};

  // Cloud triple buffer: `front` is the published observation the next tick reads, `busy` the one
  // a pending tick (or path_blocked) is reading, and there is always a third that is neither, so
  // set_cloud / set_scan never wait for a tick and never overwrite what one reads.
  std::mutex cloud_mu;
  std::mutex producer_mu;   // serialises set_cloud / set_scan callers (one producer at a time)
  int front = 0;
  int busy = -1;
  // buffer i was published but no wait on cloud_ready[i] has been enqueued on `stream` yet
  bool wait_pending[kCloudBufs] = {false, false, false};

  // multi-rank contexts (dddmr_rollout_comm_init): the library's own RCCL communicator; the tick then
  // runs k_score -> ncclAllReduce(min) of the ranks' (cost bits, -index) slots -> k_resolve on `stream`
  ncclComm_t comm = nullptr;
  int comm_ranks = 0;
  bool comm_loopback = false;        // single-device rehearsal of the exchange: the peers' words are set by the host
  int64_t* slots_dev = nullptr;      // [2 * comm_ranks] send: own slot written by k_score, INT64_MAX elsewhere
  int64_t* slots_red = nullptr;      // [2 * comm_ranks] receive
  DevResult* local_result_dev = nullptr;

  ModuleSlot<MarkingState> marking;  // dddmr_rollout_marking_create
  ModuleSlot<DepthMarkState> dmark;  // dddmr_rollout_depth_mark_create
  ModuleSlot<DepthLayerState> dlayer; // dddmr_rollout_depth_layer_create
  ModuleSlot<StackState> stack;      // dddmr_rollout_stack_create (tick_mu)
  ModuleSlot<MclState> mcl;          // dddmr_rollout_mcl_create (tick_mu)
  ModuleSlot<StaticLayerState> slayer; // dddmr_rollout_static_layer_create (tick_mu)
  ModuleSlot<GlobalPlanState> gplan;   // dddmr_rollout_global_plan_create (tick_mu)
  ModuleSlot<GpCloudState> gcloud;     // the first dddmr_rollout_global_plan_plan_on_cloud / set_lethal_points / set_graph_node_weights (tick_mu)

  std::mutex tick_mu;
  std::mutex err_mu;        // last_error is written by tick and sensor threads alike
  std::string last_error;

  // last tick (for get_debug / get_best_poses / resolve)
  DevTick last{};
  bool have_last = false;
  Window last_window;
  int timing = 1;   // DDDMR_TIMING: 0 no HIP events, 1 around k_score (score_ms), 2 also around the whole tick
  int timing_every = 1;   // DDDMR_TIMING_EVERY: record the events on every n-th tick only
  int spin = 1;     // DDDMR_SPIN: poll the host-mapped result instead of hipStreamSynchronize
  int last_heading_rows = -1; // what the last launched tick did (dddmr_rollout_heading_rows)
  int last_fused_walk = -1;   // ... and which way its k_score walked the prune plan (dddmr_rollout_fused_walk)
  int last_deal = -1;         // ... and how its assignment dealt the trajectories (dddmr_rollout_deal)
  int last_score_paths = -1;  // ... and which optional paths its k_score took (dddmr_rollout_score_paths)
  int last_assigned = 0;      // ... and whether it had an assignment at all (dddmr_rollout_get_deal)
  uint32_t seq = 0;
  DevResult last_result{};   // host copy of the last COLLECTED tick's result
  float last_score_ms = 0.f, last_device_ms = 0.f;
  // a tick whose kernels are enqueued but whose result has not been collected yet
  struct Pending {
    bool active = false;
    TickPlan plan;                 // what the tick's kernels were launched with
    bool timed = false, timed_all = false;
    Window window;                 // becomes last_window when the tick is collected
  } pend;
};

namespace {

// A consumer's pin on a cloud buffer (tick_mu held): while `busy` names the buffer no producer recycles it.
//  - kFront pins the published front buffer and releases it when the pin goes out of scope, on any return.  `busy` is
//    -1 whenever one is taken: every pinner holds tick_mu and releases before it returns, and every entry point but the
//    marking update refuses while a tick is pending.
//  - keep() hands the pin to the pending tick (tick_enqueue succeeded); kAdopted in tick_collect takes it back and
//    releases it.
//  - kOfPendingTick looks at the buffer a pending tick pins without ever releasing it (the overlapped marking update,
//    on a stream of its own: it always has to wait for the upload there).
// The "upload still pending" flag of the buffer is only cleared once the stream wait is enqueued (wait_on): an early
// error return between the pin and the wait must not lose the ordering against copy_stream.
class CloudPin {
 public:
  enum Mode { kFront, kOfPendingTick, kAdopted };
  explicit CloudPin(dddmr_rollout_ctx* c, Mode mode = kFront) : c_(c), owns_(mode != kOfPendingTick) {
    if (mode == kAdopted) {   // (only holders of tick_mu write `busy`: reading it takes no lock, and tick_collect took none)
      idx_ = c_->busy;
      return;
    }
    std::lock_guard<std::mutex> lk(c_->cloud_mu);
    if (mode == kFront) {
      idx_ = c_->busy = c_->front;
      need_wait_ = c_->wait_pending[idx_];
    } else {
      idx_ = c_->busy;
      need_wait_ = true;
    }
    is_front_ = idx_ >= 0 && idx_ == c_->front;
  }
  CloudPin(const CloudPin&) = delete;
  CloudPin& operator=(const CloudPin&) = delete;
  ~CloudPin() {
    if (!owns_) return;
    std::lock_guard<std::mutex> lk(c_->cloud_mu);
    c_->busy = -1;
  }
  int idx() const { return idx_; }
  bool is_front() const { return is_front_; }    // no newer observation had been published when the pin was taken (not kAdopted)
  uint32_t n_points() const { return c_->cloud_n[idx_]; }
  const float4* dev() const { return c_->cloud_dev[idx_]; }
  // `stream` waits for the buffer's upload, if it still has to
  hipError_t wait_on(hipStream_t stream) {
    if (!need_wait_) return hipSuccess;
    const hipError_t e = hipStreamWaitEvent(stream, c_->cloud_ready[idx_], 0);
    if (e != hipSuccess) return e;
    need_wait_ = false;
    if (owns_) {
      std::lock_guard<std::mutex> lk(c_->cloud_mu);
      c_->wait_pending[idx_] = false;   // (idx is pinned, so it cannot have been republished meanwhile)
    }
    return hipSuccess;
  }
  void keep() { owns_ = false; }

 private:
  dddmr_rollout_ctx* c_;
  bool owns_;
  int idx_ = -1;
  bool need_wait_ = false, is_front_ = false;
};

void release_source(dddmr_rollout_ctx* c, int id);   // sensor_sources.hip.h

int fail(dddmr_rollout_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) {
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    ctx->last_error = buf;
  }
  return code;
}

int refuse_pending(dddmr_rollout_ctx* ctx, const char* what) {
  return fail(ctx, DDDMR_ERR_STATE, "%s while a tick_begin is pending", what);
}
// An entry point that must not run beside a pending tick: holds tick_mu from here on, refuses under its name.
#define TICK_IDLE(ctx, what)                        \
  std::lock_guard<std::mutex> tk((ctx)->tick_mu);   \
  if ((ctx)->pend.active) return refuse_pending(ctx, what)

const dddmr_theory_config* find_theory(const dddmr_rollout_ctx* ctx, const char* name) {
  for (const auto& t : ctx->theories)
    if (std::strncmp(t.name, name, DDDMR_NAME_LEN) == 0) return &t;
  return nullptr;
}

// Every DDDMR_* variable this file listens to, read once per context, before its first HIP call.  (DDDMR_RCCL_LIB stays
// with rccl(), which runs without a context; the modules read their own.)
void read_env(dddmr_rollout_ctx* ctx) {
  TickKnobs& kn = ctx->knobs;
  if (const char* e = std::getenv("DDDMR_CELL")) {
    const float v = (float)std::atof(e);
    if (v > 0.01f && v < 10.f) { kn.cell_size = v; kn.cell_forced = true; }
  }
  if (const char* e = std::getenv("DDDMR_TILE")) kn.tile_override = std::atoi(e);
  if (const char* e = std::getenv("DDDMR_RT")) kn.rt_override = std::atoi(e);
  if (const char* e = std::getenv("DDDMR_THREADS")) kn.threads_override = std::atoi(e) == 512 ? 512 : 256;
  if (const char* e = std::getenv("DDDMR_TAIL_ROUND")) kn.tail_round = std::atoi(e) != 0;
  if (const char* e = std::getenv("DDDMR_HEADING_ROWS")) kn.heading_rows = std::atoi(e) != 0;
  if (const char* e = std::getenv("DDDMR_FUSE_WALK")) kn.fuse_walk = std::atoi(e) != 0;
  if (const char* e = std::getenv("DDDMR_SKIP_DEAD")) kn.skip_dead = std::atoi(e) != 0;
  if (const char* e = std::getenv("DDDMR_DEAL")) kn.deal_mode = std::min(std::max(std::atoi(e), -1), 2);
  if (const char* e = std::getenv("DDDMR_FINAL")) kn.final_mode = std::atoi(e) ? 1 : 0;
  if (const char* e = std::getenv("DDDMR_PROBE")) kn.probe_mode = std::atoi(e) ? 1 : 0;
  if (const char* e = std::getenv("DDDMR_TIMING")) ctx->timing = std::atoi(e);
  if (const char* e = std::getenv("DDDMR_TIMING_EVERY")) ctx->timing_every = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("DDDMR_SPIN")) ctx->spin = std::atoi(e);
  const struct { const char* name; bool* on; } given[] = {   // switched on by being set, to whatever
      {"DDDMR_NO_ASSIGN", &kn.no_assign}, {"DDDMR_NO_BOXFAST", &kn.no_boxfast}, {"DDDMR_NO_TAB", &kn.no_tab},
      {"DDDMR_GNZ_ONE", &kn.gnz_one},     {"DDDMR_POISON", &ctx->poison},       {"DDDMR_HOST_PROF", &ctx->host_prof},
      {"DDDMR_DEBUG_GRID", &ctx->debug_grid}};
  for (const auto& g : given) *g.on = std::getenv(g.name) != nullptr;
  if (const char* e = std::getenv("DDDMR_CEIL_BLOCKS")) ctx->ceil_blocks = std::max(1, std::atoi(e));
}

}  // namespace

#include "rollout_comm.hip.h"

extern "C" {

const char* dddmr_rollout_version(void) { return "dddmr-rollout-mi355x 0.1 (gfx950)"; }

size_t dddmr_rollout_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(dddmr_critic_config);
    case 1: return sizeof(dddmr_theory_config);
    case 2: return sizeof(dddmr_rollout_config);
    case 3: return sizeof(dddmr_tick_input);
    case 4: return sizeof(dddmr_rollout_result);
    case 5: return sizeof(dddmr_rollout_debug);
    case 6: return sizeof(dddmr_marking_config);
    case 7: return sizeof(dddmr_marking_stats);
    case 8: return sizeof(dddmr_depth_source_config);
    case 9: return sizeof(dddmr_depth_image_config);
    case 10: return sizeof(dddmr_depth_frustum_config);
    case 11: return sizeof(dddmr_depth_mark_config);
    case 12: return sizeof(dddmr_depth_mark_stats);
    case 13: return sizeof(dddmr_depth_layer_config);
    case 14: return sizeof(dddmr_depth_layer_stats);
    case 15: return sizeof(dddmr_stack_config);
    case 16: return sizeof(dddmr_stack_stats);
    case 17: return sizeof(dddmr_lidar_sweep_config);
    case 18: return sizeof(dddmr_mcl_config);
    case 19: return sizeof(dddmr_mcl_stats);
    case 20: return sizeof(dddmr_lidar_features_config);
    case 21: return sizeof(dddmr_mcl_observation_config);
    case 22: return sizeof(dddmr_mcl_observation_stats);
    default: return 0;
  }
}

int64_t dddmr_rollout_pack_key(double cost, uint32_t global_index) { return pack_key(cost, global_index); }
int32_t dddmr_rollout_key_index(int64_t key) { return key_index(key); }

const char* dddmr_rollout_last_error(dddmr_rollout_ctx* ctx) {
  if (!ctx) return "null context";
  // a per-thread copy: another thread may replace the context's string at any time
  static thread_local std::string copy;
  {
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    copy = ctx->last_error;
  }
  return copy.c_str();
}

void dddmr_rollout_destroy(dddmr_rollout_ctx* ctx) {
  if (!ctx) return;
  if (ctx->host_prof && ctx->prof_n)
    std::fprintf(stderr, "[dddmr] host time per tick over %llu ticks: prepare %.2f us, launches %.2f us, wait for result %.2f us\n",
                 (unsigned long long)ctx->prof_n, ctx->prof_ns[0] / ctx->prof_n * 1e-3, ctx->prof_ns[1] / ctx->prof_n * 1e-3,
                 ctx->prof_ns[2] / ctx->prof_n * 1e-3);
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
  ctx->marking.reset();                  // (the modules go between the waits above and the streams' end below)
  ctx->dmark.reset();
  ctx->stack.reset();
  ctx->dlayer.reset();
  ctx->mcl.reset();
  ctx->gcloud.reset();
  ctx->gplan.reset();
  ctx->slayer.reset();
  if (ctx->comm) (void)rccl().comm_destroy(ctx->comm);
  dev_free(ctx->mem);
  perception_free(ctx->feed);
  ctx->dclear.reset();
  for (int i = 0; i < dddmr_rollout_ctx::kMaxSources; ++i) release_source(ctx, i);
  host_free(ctx->host);
  for (hipEvent_t e : {ctx->cloud_ready[0], ctx->cloud_ready[1], ctx->cloud_ready[2], ctx->ev0, ctx->ev1, ctx->evs0, ctx->evs1})
    if (e) (void)hipEventDestroy(e);
  for (hipStream_t s : {ctx->stream, ctx->copy_stream})
    if (s) (void)hipStreamDestroy(s);
  delete ctx;
}

int dddmr_rollout_create(const dddmr_rollout_config* cfg, dddmr_rollout_ctx** out) {
  if (!cfg || !out) return DDDMR_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->abi_version != DDDMR_ROLLOUT_ABI_VERSION) return DDDMR_ERR_BAD_ARG;
  if (cfg->n_theories <= 0 || !cfg->theories) return DDDMR_ERR_BAD_ARG;
  if (cfg->max_points == 0 || cfg->max_trajectories == 0 || cfg->max_steps == 0) return DDDMR_ERR_BAD_ARG;
  if (cfg->max_trajectories >= (1u << kKeyIndexBits)) return DDDMR_ERR_CAPACITY;
  if (cfg->max_points >= (1u << 20)) return DDDMR_ERR_CAPACITY;   // a row run's length is packed into 20 bits
  if (cfg->max_steps > 4096) return DDDMR_ERR_CAPACITY;          // a pair index is packed into 12 bits
  if (cfg->max_plan_poses > (uint32_t)kMaxPlan) return DDDMR_ERR_CAPACITY;
  for (int i = 0; i < cfg->n_theories; ++i) {
    const auto& t = cfg->theories[i];
    if (t.n_critics < 0 || t.n_critics > DDDMR_MAX_CRITICS) return DDDMR_ERR_BAD_ARG;
    if (t.kind < 0 || t.kind > DDDMR_THEORY_DD_ROTATE_INPLACE) return DDDMR_ERR_BAD_ARG;
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return DDDMR_ERR_NO_DEVICE;
  if (cfg->device < 0 || cfg->device >= n_dev) return DDDMR_ERR_NO_DEVICE;

  auto* ctx = new dddmr_rollout_ctx();
  ctx->cfg = *cfg;
  ctx->theories.assign(cfg->theories, cfg->theories + cfg->n_theories);
  ctx->cfg.theories = ctx->theories.data();
  ctx->device = cfg->device;
  read_env(ctx);

  auto init = [&]() -> int {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
      hipDeviceProp_t prop;
      HIPCHK(ctx, hipGetDeviceProperties(&prop, ctx->device));
      ctx->knobs.n_cu = std::max(1, prop.multiProcessorCount);
    }
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (hipEvent_t* e : {&ctx->ev0, &ctx->ev1, &ctx->evs0, &ctx->evs1}) HIPCHK(ctx, hipEventCreate(e));
    const size_t P = cfg->max_points, N = cfg->max_trajectories;
    // the pair records: whole trips of phase P's scalar-load walk plus one chunk of slack for its last request ahead
    const size_t plan_cap = plan_padded_poses(std::max<uint32_t>(cfg->max_plan_poses, 1));
    DevAllocs& mem = ctx->mem;
    for (int i = 0; i < kCloudBufs; ++i) {
      HIPCHK(ctx, dev_alloc(mem, &ctx->cloud_dev[i], P));
      HIPCHK(ctx, hipEventCreateWithFlags(&ctx->cloud_ready[i], hipEventDisableTiming));
    }
    HIPCHK(ctx, dev_alloc(mem, &ctx->pt_slot, P));
    HIPCHK(ctx, dev_alloc(mem, &ctx->sorted, P + kItem));
    HIPCHK(ctx, hipMemset(ctx->sorted, 0, (P + kItem) * sizeof(Pt3)));
    HIPCHK(ctx, dev_alloc(mem, &ctx->cell_count, (size_t)kCapCells + 1));
    HIPCHK(ctx, dev_alloc(mem, &ctx->cell_start, (size_t)kCapCells + 1));
    HIPCHK(ctx, hipMemset(ctx->cell_count, 0, (kCapCells + 1) * sizeof(uint32_t)));
    HIPCHK(ctx, dev_alloc(mem, &ctx->row_tab, (size_t)kTabCap));
    HIPCHK(ctx, dev_alloc(mem, &ctx->axes_dev, (size_t)3 * kMaxAxis));
    HIPCHK(ctx, dev_alloc(mem, &ctx->samples_dev, N));
    HIPCHK(ctx, dev_alloc(mem, &ctx->plan_dev, std::max<size_t>(cfg->max_plan_poses, 1)));
    HIPCHK(ctx, dev_alloc(mem, &ctx->plan_pairs_dev, plan_cap * kPlanPoseWords));
    HIPCHK(ctx, dev_alloc(mem, &ctx->costs, N));
    HIPCHK(ctx, dev_alloc(mem, &ctx->partial, N));
    HIPCHK(ctx, dev_alloc(mem, &ctx->steps, N));
    HIPCHK(ctx, dev_alloc(mem, &ctx->samples_out, N));
    // words 0..2: unused (the binning launch still resets them); from kSlotBase on: four words per workgroup of the
    // launch that ends the scoring (k_score on single-round shards, k_finalize on multi-round ones)
    HIPCHK(ctx, dev_alloc(mem, &ctx->best_key, (size_t)kSlotBase + (size_t)kSlotWords * N));
    HIPCHK(ctx, dev_alloc(mem, &ctx->overflow, 1));
    HIPCHK(ctx, dev_alloc(mem, &ctx->traj_load, N));
    HIPCHK(ctx, hipMemset(ctx->traj_load, 0, N * sizeof(uint32_t)));
    HIPCHK(ctx, dev_alloc(mem, &ctx->assign, N));
    HIPCHK(ctx, dev_alloc(mem, &ctx->tickets, 2));
    HIPCHK(ctx, hipMemset(ctx->tickets, 0, 2 * sizeof(uint32_t)));
    HIPCHK(ctx, dev_alloc(mem, &ctx->poses_dev, (size_t)cfg->max_steps * 7));
    HIPCHK(ctx, dev_alloc(mem, &ctx->blocked_plan, (size_t)kBlockedMaxPlan));
    HIPCHK(ctx, dev_alloc(mem, &ctx->blocked_flags, (size_t)kBlockedMaxPlan / 32));
    for (int i = 0; i < kCloudBufs; ++i) HIPCHK(ctx, host_alloc(ctx->host, &ctx->cloud_stage[i], P * sizeof(float4)));
    const size_t small = std::max<size_t>({3 * kMaxAxis * sizeof(float), N * sizeof(float4),
                                           plan_cap * sizeof(float4)});
    HIPCHK(ctx, host_alloc(ctx->host, &ctx->small_stage, small));
    if (host_mapped_alloc(ctx->host, &ctx->result_host, &ctx->result_dev, sizeof(DevResult)) != 0)
      return fail(ctx, DDDMR_ERR_HIP, "result record allocation failed");
    const int rc = perception_alloc(ctx->feed, P);
    if (rc != 0) return fail(ctx, DDDMR_ERR_HIP, "perception scratch allocation failed");
    {
      const void* big_lds_kernels[] = {
          reinterpret_cast<const void*>(k_rollout), reinterpret_cast<const void*>(k_bin_count),
#define DDDMR_SCORE_KERNELS(T, L) \
  reinterpret_cast<const void*>(k_score<T, L, false, false>), reinterpret_cast<const void*>(k_score<T, L, true, false>), \
  reinterpret_cast<const void*>(k_score<T, L, false, true>), reinterpret_cast<const void*>(k_score<T, L, true, true>)
          DDDMR_SCORE_KERNELS(256, false), DDDMR_SCORE_KERNELS(256, true), DDDMR_SCORE_KERNELS(512, false), DDDMR_SCORE_KERNELS(512, true)};
#undef DDDMR_SCORE_KERNELS
      for (const void* f : big_lds_kernels) HIPCHK(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kScoreLdsMax));
    }
    HIPCHK(ctx, hipDeviceSynchronize());
    return DDDMR_OK;
  };
  const int rc = init();
  if (rc != DDDMR_OK) {
    fprintf(stderr, "dddmr_rollout_create: %s\n", ctx->last_error.c_str());
    dddmr_rollout_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return DDDMR_OK;
}

// Publish a device-side cloud buffer as the new front buffer.  producer_mu held.  layout: where its points came from
// (the sources' layout(), single_lidar_layout() for the single-producer set_scan, foreign_layout() for a set_cloud).
static void publish_cloud(dddmr_rollout_ctx* ctx, int idx, uint32_t n, const SourceLayout& layout) {
  std::lock_guard<std::mutex> lk(ctx->cloud_mu);
  ctx->cloud_n[idx] = n;
  ctx->cloud_layout[idx] = layout;
  ctx->front = idx;
  ctx->wait_pending[idx] = true;
}

// Pick the buffer to fill: neither the published front nor the one a pending tick reads.
// Never waits (the round-1 double buffer blocked -- on one thread forever -- when a second
// observation arrived while a tick_begin was pending); producer_mu must be held.
static int acquire_back(dddmr_rollout_ctx* ctx) {
  std::lock_guard<std::mutex> lk(ctx->cloud_mu);
  for (int i = 0; i < kCloudBufs; ++i)
    if (i != ctx->front && i != ctx->busy) return i;
  return -1;   // unreachable: three buffers, two exclusions
}

int dddmr_rollout_set_cloud(dddmr_rollout_ctx* ctx, const float* xyzi, size_t n_points,
                            size_t stride_bytes) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!cloud_arg_ok(xyzi, n_points, stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "set_cloud: bad pointer/stride");
  if (n_points > ctx->cfg.max_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "set_cloud: %zu points > max_points %u", n_points, ctx->cfg.max_points);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  const int back = acquire_back(ctx);
  // The staging buffer of this slot may still feed the copy of an earlier call.
  HIPCHK(ctx, hipEventSynchronize(ctx->cloud_ready[back]));
  // Repack to float4 (PCL PointXYZI is 32 bytes wide) in pinned memory, in a few chunks so
  // that the DMA of one chunk runs while the next is repacked.  The call does not wait for
  // the copies: consumers wait on cloud_ready[back] (the tick's stream does so on the device).
  const size_t sf = stride_bytes / 4;
  const bool has_i = stride_bytes >= 16;
  float4* stage = ctx->cloud_stage[back];
  const size_t kChunks = n_points >= 32768 ? 4 : 1;
  for (size_t c = 0; c < kChunks; ++c) {
    const size_t b = n_points * c / kChunks, e = n_points * (c + 1) / kChunks;
    if (stride_bytes == 16) {
      std::memcpy(stage + b, xyzi + 4 * b, (e - b) * sizeof(float4));
    } else {
      for (size_t i = b; i < e; ++i) {
        const float* p = xyzi + i * sf;
        stage[i] = make_float4(p[0], p[1], p[2], has_i ? p[3] : 0.f);
      }
    }
    if (e > b)
      HIPCHK(ctx, hipMemcpyAsync(ctx->cloud_dev[back] + b, stage + b, (e - b) * sizeof(float4), hipMemcpyHostToDevice,
                                 ctx->copy_stream));
  }
  HIPCHK(ctx, hipEventRecord(ctx->cloud_ready[back], ctx->copy_stream));
  publish_cloud(ctx, back, (uint32_t)n_points, foreign_layout());
  return DDDMR_OK;
}

int dddmr_rollout_get_cloud(dddmr_rollout_ctx* ctx, float* xyzi_out, size_t capacity, size_t* n_points) {
  if (!ctx || !n_points) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  TICK_IDLE(ctx, "get_cloud");
  CloudPin pin(ctx);                            // a producer must not recycle the buffer while it is copied
  const int idx = pin.idx();
  const uint32_t n = pin.n_points();
  *n_points = n;
  if (!xyzi_out) return DDDMR_OK;
  if (capacity < n) return fail(ctx, DDDMR_ERR_CAPACITY, "get_cloud: capacity %zu < %u", capacity, n);
  HIPCHK(ctx, hipEventSynchronize(ctx->cloud_ready[idx]));      // set_cloud returns before its copy has landed
  if (n) HIPCHK(ctx, hipMemcpy(xyzi_out, ctx->cloud_dev[idx], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

int dddmr_rollout_path_blocked(dddmr_rollout_ctx* ctx, const float* plan_xyzi, size_t n_plan, double check_radius,
                               double* ratio, int32_t* opinion, uint8_t* blocked_flags) {
  if (!ctx || !ratio || !opinion) return DDDMR_ERR_BAD_ARG;
  if (n_plan > 0 && !plan_xyzi) return fail(ctx, DDDMR_ERR_BAD_ARG, "path_blocked: null plan");
  if (n_plan > (size_t)kBlockedMaxPlan)
    return fail(ctx, DDDMR_ERR_CAPACITY, "path_blocked: %zu plan points > %d", n_plan, kBlockedMaxPlan);
  TICK_IDLE(ctx, "path_blocked");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  *ratio = 0.0;
  *opinion = DDDMR_OPINION_PASS;
  if (blocked_flags) std::memset(blocked_flags, 0, n_plan);
  // pin the front cloud like a tick does; an error return past the launch waits for the stream before the pin lets go
  CloudPin pin(ctx);
  Drain drain{ctx->stream, false};
  const uint32_t n_points = pin.n_points();
  if (n_points <= 5 || n_plan == 0) return DDDMR_OK;                  // path_blocked_strategy.cpp:62-64
  BlockedParams b;
  b.n_points = (int)n_points;
  b.m = (int)n_plan;
  b.r2 = static_cast<float>(check_radius * check_radius);             // pcl::KdTreeFLANN::radiusSearch
  bool any = false;
  for (int a = 0; a < 3; ++a) { b.lo[a] = 3.402823466e+38f; b.hi[a] = -3.402823466e+38f; }
  for (size_t i = 0; i < n_plan; ++i) {
    if (plan_xyzi[4 * i + 3] < 0) continue;
    any = true;
    for (int a = 0; a < 3; ++a) {
      b.lo[a] = std::min(b.lo[a], plan_xyzi[4 * i + a]);
      b.hi[a] = std::max(b.hi[a], plan_xyzi[4 * i + a]);
    }
  }
  if (any) {
    // conservative reject box: a point farther than r from the plan's box along an axis cannot be within r
    const float grow = (float)(std::fabs(check_radius) * 1.000001 + 1e-6);
    for (int a = 0; a < 3; ++a) {
      b.lo[a] = std::nextafter(b.lo[a] - grow, -3.402823466e+38f);
      b.hi[a] = std::nextafter(b.hi[a] + grow, 3.402823466e+38f);
    }
    HIPCHK(ctx, pin.wait_on(ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->blocked_plan, plan_xyzi, n_plan * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->blocked_flags, 0, (kBlockedMaxPlan / 32) * sizeof(uint32_t), ctx->stream));
    const int blocks = (int)std::min<uint32_t>(1024, (n_points + 255) / 256);
    uint32_t words[kBlockedMaxPlan / 32];
    drain.armed = true;                        // from here on the stream reads the pinned cloud (and writes `words`)
    hipLaunchKernelGGL(k_path_blocked, dim3(blocks), dim3(256), 0, ctx->stream, b, pin.dev(),
                       ctx->blocked_plan, ctx->blocked_flags);
    HIPCHK(ctx, hipMemcpyAsync(words, ctx->blocked_flags, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    drain.armed = false;
    size_t blocked = 0;
    for (size_t i = 0; i < n_plan; ++i) {
      const bool hit = (words[i >> 5] >> (i & 31)) & 1u;
      if (hit) ++blocked;
      if (blocked_flags) blocked_flags[i] = hit ? 1 : 0;
    }
    const float orig = (float)n_plan, blk = (float)blocked;           // float division, double scale (:91-93)
    *ratio = (blk) / (orig) * 100.0;
  }
  if (*ratio > 0.0) *opinion = DDDMR_OPINION_PATH_BLOCKED_WAIT;       // :96-97
  return DDDMR_OK;
}

int dddmr_rollout_set_prune_plan(dddmr_rollout_ctx* ctx, const double* poses, size_t n_poses) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (n_poses > 0 && !poses) return fail(ctx, DDDMR_ERR_BAD_ARG, "set_prune_plan: null poses");
  if (n_poses > ctx->cfg.max_plan_poses)
    return fail(ctx, DDDMR_ERR_CAPACITY, "set_prune_plan: %zu poses > max_plan_poses %u", n_poses,
                ctx->cfg.max_plan_poses);
  TICK_IDLE(ctx, "set_prune_plan");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // ModelSharedData::updateData: positions as float PointXYZI (model_shared_data.h:83-91)
  // For phase P's scalar walk the same positions go up a second time as pair records, padded with copies of the last
  // pose to whole loop trips (plan_pack_pairs).  Packed and written on every call, never per tick, so a shorter plan
  // after a longer one is padded afresh.
  if (n_poses) {
    std::vector<float4> xyz(n_poses);
    for (size_t i = 0; i < n_poses; ++i)
      xyz[i] = make_float4((float)poses[7 * i + 0], (float)poses[7 * i + 1], (float)poses[7 * i + 2], 0.f);
    std::vector<float> pairs(plan_padded_poses(n_poses) * kPlanPoseWords);
    plan_pack_pairs(xyz.data(), n_poses, pairs.data());
    HIPCHK(ctx, hipMemcpy(ctx->plan_dev, xyz.data(), xyz.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->plan_pairs_dev, pairs.data(), pairs.size() * sizeof(float), hipMemcpyHostToDevice));
    std::memcpy(ctx->plan_last, poses + 7 * (n_poses - 1), 7 * sizeof(double));
  }
  ctx->plan_m = (uint32_t)n_poses;
  return DDDMR_OK;
}

}  // extern "C"

namespace {

// "no trajectory": what every such result shares; the key is the caller's (resolve keeps the one it was given)
void set_no_winner(dddmr_rollout_result* out) {
  out->planner_state = DDDMR_ALL_TRAJECTORIES_FAIL;
  out->best_index = -1;
  out->best_cost = -1.0;
  out->vx = out->vy = out->wz = 0.0;
}

void no_winner(dddmr_rollout_result* out) {
  std::memset(out, 0, sizeof(*out));
  set_no_winner(out);
  out->key = kKeyNone;
}

// Enqueue one tick: plan it (tick_plan.hip.h, arithmetic alone), then upload and launch what the plan says; tick_mu
// must be held.
int tick_enqueue(dddmr_rollout_ctx* ctx, const char* theory_name, const dddmr_tick_input* in) {
  const auto prof_t0 = std::chrono::steady_clock::now();
  const dddmr_theory_config* th = find_theory(ctx, theory_name);
  if (!th) return fail(ctx, DDDMR_ERR_UNKNOWN_THEORY, "unknown theory '%s'", theory_name);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  Window& w = ctx->pend.window;
  make_window(*th, *in, w);   // initialise(): velocity samples of this tick

  // The cloud's front buffer is pinned before the plan's capacity checks, because the plan needs its size.  No caller
  // can tell: the pin releases the buffer again on any error return (CloudPin), once nothing reads it any more (Drain).
  CloudPin pin(ctx);
  Drain drain{ctx->stream, false};

  TickPlan& p = ctx->pend.plan;
  DevTick& k = p.k;
  const int theory_id = (int)(th - ctx->theories.data());
  const bool exchange = ctx->comm || ctx->comm_loopback;
  std::string err;
  const int rc = plan_tick(ctx->knobs, ctx->feedback, ctx->cfg, *th, theory_id, *in, w, pin.n_points(), ctx->plan_m,
                           ctx->plan_last, exchange, &p, &err);
  if (rc != DDDMR_OK) return fail(ctx, rc, "%s", err.c_str());
  if (ctx->seq == 0 && ctx->debug_grid)     // (the first tick: tests read the size of the row-run index k_score stages here)
    std::fprintf(stderr, "[dddmr] grid: %d x %d x %d cells, row-run index of %d entries in LDS\n", k.gnx, k.gny, k.gnz, k.tab_entries);
  if (ctx->seq == 3 && ctx->debug_grid)
    std::fprintf(stderr, "[dddmr] k_score shape: %d lanes, tile %d, %d-step rows, %zu bytes of dynamic LDS (tile+1 would need %zu)\n", p.thr, k.tile,
                 p.s_tick, p.score_lds, plan_score_lds(k, k.tile + 1));

  // small per-tick uploads (sample axes or explicit list)
  if (p.upload == kUploadList) {
    std::memcpy(ctx->small_stage, w.list.data(), w.list.size() * sizeof(float4));
    HIPCHK(ctx, hipMemcpyAsync(ctx->samples_dev, ctx->small_stage, w.list.size() * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  } else if (p.upload == kUploadAxesDev) {
    float* a = ctx->small_stage;
    std::memcpy(a, w.ax.data(), w.ax.size() * sizeof(float));
    std::memcpy(a + k.ay_ofs, w.ay.data(), w.ay.size() * sizeof(float));
    std::memcpy(a + k.ath_ofs, w.ath.data(), w.ath.size() * sizeof(float));
    HIPCHK(ctx, hipMemcpyAsync(ctx->axes_dev, a, 3 * kMaxAxis * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  }
  if (k.n_local > 0) {
    // state arrays of the body-frame rollout
    const size_t need = (size_t)k.n_local * (size_t)p.s_tick;
    if (need > ctx->st_cap || !ctx->traj_info) {
      HIPCHK(ctx, hipDeviceSynchronize());
      ctx->st_cap = 0;
      const size_t cap = need + need / 4 + 1024;
      HIPCHK(ctx, dev_realloc(ctx->mem, &ctx->st_sc, cap));
      HIPCHK(ctx, dev_realloc(ctx->mem, &ctx->st_xy, cap));
      HIPCHK(ctx, dev_realloc(ctx->mem, &ctx->st_pp, (size_t)ctx->cfg.max_trajectories));
      ctx->st_cap = cap;
      if (!ctx->traj_info) HIPCHK(ctx, dev_alloc(ctx->mem, &ctx->traj_info, (size_t)ctx->cfg.max_trajectories));
    }
  }
  HIPCHK(ctx, pin.wait_on(ctx->stream));

  const auto prof_t1 = std::chrono::steady_clock::now();
  if (ctx->poison && k.n_local > 0) {
    HIPCHK(ctx, hipMemsetAsync(ctx->costs, 0xFF, (size_t)k.n_local * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->steps, 0xFF, (size_t)k.n_local * sizeof(int32_t), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->samples_out, 0xFF, (size_t)k.n_local * sizeof(float4), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->partial, 0xFF, (size_t)k.n_local * sizeof(TrajPartial), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->st_pp, 0xFF, (size_t)k.n_local * sizeof(double2), ctx->stream));
  }
  k.seq = ++ctx->seq;
  if (k.seq == 0) k.seq = ctx->seq = 1;
  // HIP events serialise the queue around them (~3 us each); timed ticks are sampled
  const bool timed = ctx->timing >= 1 && (ctx->seq % (uint32_t)ctx->timing_every) == 0;
  const bool timed_all = timed && ctx->timing >= 2;
  if (timed_all) HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  // traj_load will describe this tick's shard of this theory
  ctx->feedback.load_theory = theory_id;
  ctx->feedback.load_nlocal = k.n_local;
  ctx->last_heading_rows = p.heading_rows;
  ctx->last_fused_walk = k.n_local > 0 ? p.fused_walk : 0;
  ctx->last_score_paths = k.n_local > 0 ? (p.skip_dead ? 1 : 0) : 0;
  ctx->last_deal = p.deal;
  ctx->last_assigned = k.use_assign;
  drain.armed = true;       // from here on the stream reads the pinned cloud
  if (k.n_points > 0) {
    hipLaunchKernelGGL(k_bin_count, dim3(p.cnt_blocks + p.roll_blocks + (k.use_assign ? k.assign_groups : 0)), dim3(kBinThreads),
                       p.roll_launch_lds, ctx->stream, k, pin.dev(), ctx->cell_count, ctx->cell_start, ctx->pt_slot, ctx->tickets,
                       ctx->best_key, ctx->overflow, ctx->axes_dev, ctx->samples_dev, ctx->traj_info, ctx->st_sc,
                       ctx->st_xy, ctx->st_pp, ctx->traj_load, ctx->assign, p.heading_rows, p.deal, p.deal_head);
    hipLaunchKernelGGL(k_bin_scatter, dim3(p.bin_blocks), dim3(256), 0, ctx->stream, k, pin.dev(),
                       ctx->pt_slot, ctx->cell_start, ctx->sorted, ctx->row_tab);
  } else {
    hipLaunchKernelGGL(k_bin_reset, dim3(1), dim3(256), 0, ctx->stream, k, ctx->cell_count, ctx->cell_start,
                       ctx->best_key, ctx->overflow);
    if (p.roll_blocks > 0)
      hipLaunchKernelGGL(k_rollout, dim3(p.roll_blocks), dim3(256), p.roll_launch_lds, ctx->stream, k, ctx->axes_dev,
                         ctx->samples_dev, ctx->traj_info, ctx->st_sc, ctx->st_xy, ctx->st_pp, p.heading_rows);
    if (k.use_assign)
      hipLaunchKernelGGL(k_assign, dim3(k.assign_groups), dim3(kBinThreads), 0, ctx->stream, k, ctx->traj_load, ctx->assign, p.deal,
                         p.deal_head);
  }
  if (timed) HIPCHK(ctx, hipEventRecord(ctx->evs0, ctx->stream));
  // multi-rank context: k_score leaves the shard's winner on the device (staging record + its slot of
  // the all-reduce), k_resolve publishes the global one
  DevResult* score_result = exchange ? ctx->local_result_dev : ctx->result_dev;
  int64_t* score_words = exchange ? ctx->slots_dev + 2 * p.rank : nullptr;
  if (k.n_local > 0) {
    const int wgs = k.n_tiles;
    const size_t lds = p.score_lds;
#define DDDMR_LAUNCH_SCORE(T, L)                                                                                   \
  do { if (k.probe) DDDMR_LAUNCH_SCORE_P(T, L, true); else DDDMR_LAUNCH_SCORE_P(T, L, false); } while (0)
#define DDDMR_LAUNCH_SCORE_P(T, L, P)                                                                              \
  do { if (p.deal != kDealSnake) DDDMR_LAUNCH_SCORE_K(T, L, P, true); else DDDMR_LAUNCH_SCORE_K(T, L, P, false); } while (0)
#define DDDMR_LAUNCH_SCORE_K(T, L, P, I)                                                                           \
  hipLaunchKernelGGL((k_score<T, L, P, I>), dim3(wgs), dim3(T), lds, ctx->stream, k, ctx->traj_info, ctx->st_sc,     \
                     ctx->st_xy, ctx->plan_dev, ctx->cell_start, ctx->sorted, ctx->costs, ctx->steps,             \
                     ctx->samples_out, ctx->best_key, ctx->overflow, ctx->tickets + 1, score_result, ctx->assign, \
                     ctx->traj_load, score_words, ctx->row_tab, ctx->plan_pairs_dev, ctx->partial, p.fused_walk,  \
                     ctx->st_pp, p.deal, p.skip_dead)
    if (p.thr == 512) { if (p.lean) DDDMR_LAUNCH_SCORE(512, true); else DDDMR_LAUNCH_SCORE(512, false); }
    else              { if (p.lean) DDDMR_LAUNCH_SCORE(256, true); else DDDMR_LAUNCH_SCORE(256, false); }
#undef DDDMR_LAUNCH_SCORE
#undef DDDMR_LAUNCH_SCORE_P
#undef DDDMR_LAUNCH_SCORE_K
  } else {
    hipLaunchKernelGGL(k_empty_result, dim3(1), dim3(64), 0, ctx->stream, k, ctx->cell_start, score_result, score_words);
  }
  if (timed) HIPCHK(ctx, hipEventRecord(ctx->evs1, ctx->stream));
  // multi-round shards: stacked scoring + exact argmin, one lane per trajectory (the HIP-event score_ms above then
  // covers k_score without the stacked scoring)
  if (k.n_local > 0 && k.final_kernel)
    hipLaunchKernelGGL(k_finalize, dim3((k.n_local + kFinalThreads - 1) / kFinalThreads), dim3(kFinalThreads), 0, ctx->stream, k,
                       ctx->traj_info, ctx->partial, ctx->costs, ctx->steps, ctx->samples_out, ctx->traj_load, ctx->best_key,
                       ctx->cell_start, ctx->overflow, ctx->tickets + 1, score_result, score_words);
  if (exchange) {
    // ONE collective per tick, on the tick's stream: ordered after k_score / k_finalize (which wrote this rank's two
    // words of slots_dev) and before k_resolve by stream order alone; no host synchronisation in between.
    if (ctx->comm) {
      const int nrc = rccl().all_reduce(ctx->slots_dev, ctx->slots_red, (size_t)2 * ctx->comm_ranks, ncclInt64, ncclMin,
                                        ctx->comm, ctx->stream);
      if (nrc != ncclSuccess) return fail(ctx, DDDMR_ERR_HIP, "ncclAllReduce failed: %s", rccl().error_string((ncclResult_t)nrc));
    } else {
      HIPCHK(ctx, hipMemcpyAsync(ctx->slots_red, ctx->slots_dev, (size_t)2 * ctx->comm_ranks * sizeof(int64_t),
                                 hipMemcpyDeviceToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(k_resolve, dim3(1), dim3(64), 0, ctx->stream, k, ctx->slots_red, ctx->comm_ranks,
                       ctx->local_result_dev, ctx->axes_dev, ctx->samples_dev, ctx->result_dev);
  }
  if (timed_all) HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIPCHK(ctx, hipGetLastError());
  if (ctx->host_prof) {
    const auto prof_t2 = std::chrono::steady_clock::now();
    ctx->prof_ns[0] += std::chrono::duration<double, std::nano>(prof_t1 - prof_t0).count();
    ctx->prof_ns[1] += std::chrono::duration<double, std::nano>(prof_t2 - prof_t1).count();
    ++ctx->prof_n;
  }
  pin.keep();             // the cloud buffer stays pinned until tick_collect
  drain.armed = false;    // ... which waits for the tick
  ctx->pend.active = true;
  ctx->pend.timed = timed;
  ctx->pend.timed_all = timed_all;
  return DDDMR_OK;
}

// Wait for the enqueued tick and decode its result; tick_mu must be held.
int tick_collect(dddmr_rollout_ctx* ctx, dddmr_rollout_result* out) {
  if (!ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "tick_end without tick_begin");
  ctx->pend.active = false;
  CloudPin pin(ctx, CloudPin::kAdopted);   // releases the tick's cloud buffer on any return
  const TickPlan& p = ctx->pend.plan;
  const DevTick& k = p.k;
  no_winner(out);
  out->n_samples = p.n_samples;
  out->local_begin = p.local_begin;
  out->n_local = p.n_local;
  const auto prof_c0 = std::chrono::steady_clock::now();
  // The last k_score workgroup stores the result into host-mapped memory and then
  // the tick's sequence number (system-scope release): polling it beats a stream
  // synchronise by several microseconds.  Bounded; falls back to the stream sync.
  const bool seen = ctx->spin && wait_seq(&ctx->result_host->seq, k.seq);
  if (!seen) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->pend.timed) {
    HIPCHK(ctx, hipEventSynchronize(ctx->pend.timed_all ? ctx->ev1 : ctx->evs1));
    if (ctx->pend.timed_all) HIPCHK(ctx, hipEventElapsedTime(&ctx->last_device_ms, ctx->ev0, ctx->ev1));
    HIPCHK(ctx, hipEventElapsedTime(&ctx->last_score_ms, ctx->evs0, ctx->evs1));
  }
  const float ms = ctx->last_device_ms, score_ms = ctx->last_score_ms;   // latest sampled values

  if (ctx->host_prof) ctx->prof_ns[2] += std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - prof_c0).count();
  const DevResult r = *ctx->result_host;
  ctx->last_result = r;
  if (k.n_local > 0) ctx->feedback.collided_share = (float)r.n_collided / (float)k.n_local;
  ctx->last = k;
  ctx->last_window = ctx->pend.window;
  ctx->have_last = true;
  if (r.overflow)
    return fail(ctx, DDDMR_ERR_CAPACITY, "device capacity flag %u (1: trajectory longer than %d steps, 2: cuboid spans more than %d cell rows)",
                r.overflow, p.s_tick, kRows);
  out->device_ms = ms;
  out->score_ms = score_ms;
  out->n_points_binned = r.n_binned;
  out->key = r.key;
  if (r.index >= 0) {
    out->planner_state = DDDMR_TRAJECTORY_FOUND;
    out->best_index = r.index;
    out->best_cost = r.cost;
    out->vx = r.vx; out->vy = r.vy; out->wz = r.wz;
  }
  return DDDMR_OK;
}

}  // namespace

extern "C" {

int dddmr_rollout_tick(dddmr_rollout_ctx* ctx, const char* theory_name, const dddmr_tick_input* in,
                       dddmr_rollout_result* out) {
  if (!ctx || !theory_name || !in || !out) return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "tick");
  no_winner(out);
  const int rc = tick_enqueue(ctx, theory_name, in);
  if (rc != DDDMR_OK) return rc;
  return tick_collect(ctx, out);
}

int dddmr_rollout_tick_begin(dddmr_rollout_ctx* ctx, const char* theory_name, const dddmr_tick_input* in) {
  if (!ctx || !theory_name || !in) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (ctx->pend.active) return fail(ctx, DDDMR_ERR_STATE, "tick_begin while another tick_begin is pending");
  return tick_enqueue(ctx, theory_name, in);
}

int dddmr_rollout_tick_end(dddmr_rollout_ctx* ctx, dddmr_rollout_result* out) {
  if (!ctx || !out) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  return tick_collect(ctx, out);
}

int dddmr_rollout_resolve(dddmr_rollout_ctx* ctx, int64_t reduced_key, dddmr_rollout_result* inout) {
  if (!ctx || !inout) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (!ctx->have_last) return fail(ctx, DDDMR_ERR_STATE, "resolve before any tick");
  inout->key = reduced_key;
  const int32_t idx = key_index(reduced_key);
  if (idx < 0) {
    set_no_winner(inout);
    return DDDMR_OK;
  }
  if (idx >= ctx->last.n_global) return fail(ctx, DDDMR_ERR_BAD_ARG, "resolve: index %d out of range", idx);
  float vx, vy, wz;
  sample_of(ctx->last_window, idx, &vx, &vy, &wz);
  inout->planner_state = DDDMR_TRAJECTORY_FOUND;
  inout->best_index = idx;
  inout->vx = vx; inout->vy = vy; inout->wz = wz;
  if (ctx->last_result.index == idx) {
    inout->best_cost = ctx->last_result.cost;   // this rank's own winner: exact
  } else {
    // winner lives on another rank (or an older tick): the key carries the cost's top 40 bits
    union { double d; uint64_t u; } cv;
    cv.u = (uint64_t)reduced_key & ~((1ull << kKeyIndexBits) - 1);
    inout->best_cost = cv.d;
  }
  return DDDMR_OK;
}

void dddmr_rollout_winner_words(const dddmr_rollout_result* r, int64_t words[2]) {
  words[0] = words[1] = INT64_MAX;
  if (!r || r->best_index < 0) return;
  words[0] = cost_bits(r->best_cost);
  if (words[0] != INT64_MAX) words[1] = -(int64_t)r->best_index;
}

int dddmr_rollout_resolve_words(dddmr_rollout_ctx* ctx, const int64_t* words, int32_t n_ranks,
                                dddmr_rollout_result* inout) {
  if (!ctx || !inout || !words || n_ranks <= 0) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (!ctx->have_last) return fail(ctx, DDDMR_ERR_STATE, "resolve before any tick");
  // minimum cost (full doubles), equal costs -> highest index: local_planner.cpp:460 over the whole batch
  int64_t c = INT64_MAX, ni = INT64_MAX;
  for (int r = 0; r < n_ranks; ++r) {
    const int64_t cr = words[2 * r], ir = words[2 * r + 1];
    if (cr == INT64_MAX) continue;
    if (cr < c || (cr == c && ir < ni)) { c = cr; ni = ir; }
  }
  if (c == INT64_MAX) {
    set_no_winner(inout);
    inout->key = kKeyNone;
    return DDDMR_OK;
  }
  const int64_t idx = -ni;
  if (idx < 0 || idx >= ctx->last.n_global) return fail(ctx, DDDMR_ERR_BAD_ARG, "resolve_words: index %lld out of range", (long long)idx);
  float vx, vy, wz;
  sample_of(ctx->last_window, (int)idx, &vx, &vy, &wz);
  union { double d; int64_t i; } cv;
  cv.i = c;
  inout->planner_state = DDDMR_TRAJECTORY_FOUND;
  inout->best_index = (int32_t)idx;
  inout->best_cost = cv.d;
  inout->vx = vx; inout->vy = vy; inout->wz = wz;
  inout->key = pack_key(cv.d, (uint32_t)idx);
  return DDDMR_OK;
}

int dddmr_rollout_device_count(int32_t* n_out) {
  if (!n_out) return DDDMR_ERR_BAD_ARG;
  int n = 0;
  *n_out = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return DDDMR_ERR_NO_DEVICE; }
  *n_out = n;
  return DDDMR_OK;
}

// The theory's initialise() alone: the velocity samples a tick with these inputs would roll out, in the
// reference's generation order (x-major, y, theta-minor).  Host-only, no device work.
int dddmr_rollout_samples(dddmr_rollout_ctx* ctx, const char* theory_name, const dddmr_tick_input* in, float* samples_out,
                          size_t capacity, size_t* n_samples) {
  if (!ctx || !theory_name || !in || !n_samples) return DDDMR_ERR_BAD_ARG;
  const dddmr_theory_config* th = find_theory(ctx, theory_name);
  if (!th) return fail(ctx, DDDMR_ERR_UNKNOWN_THEORY, "unknown theory '%s'", theory_name);
  Window w;
  make_window(*th, *in, w);
  const size_t n = w.count();
  *n_samples = n;
  if (!samples_out) return DDDMR_OK;
  if (capacity < n) return fail(ctx, DDDMR_ERR_CAPACITY, "samples: capacity %zu < %zu", capacity, n);
  for (size_t i = 0; i < n; ++i) sample_of(w, (int)i, samples_out + 3 * i, samples_out + 3 * i + 1, samples_out + 3 * i + 2);
  return DDDMR_OK;
}

int dddmr_rollout_heading_rows(dddmr_rollout_ctx* ctx) {
  if (!ctx) return -1;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  return ctx->last_heading_rows;
}

int dddmr_rollout_fused_walk(dddmr_rollout_ctx* ctx) {
  if (!ctx) return -1;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  return ctx->last_fused_walk;
}

int dddmr_rollout_score_paths(dddmr_rollout_ctx* ctx) {
  if (!ctx) return -1;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  return ctx->last_score_paths;
}

int dddmr_rollout_deal(dddmr_rollout_ctx* ctx) {
  if (!ctx) return -1;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  return ctx->last_deal;
}

int dddmr_rollout_get_deal(dddmr_rollout_ctx* ctx, uint32_t* assign_out, uint32_t* load_out, size_t capacity, size_t* n_local,
                           int32_t* assigned) {
  if (!ctx || !n_local) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (!ctx->have_last) return fail(ctx, DDDMR_ERR_STATE, "get_deal before any tick");
  if (ctx->pend.active) return refuse_pending(ctx, "get_deal");
  const size_t n = (size_t)ctx->last.n_local;
  *n_local = n;
  if (assigned) *assigned = ctx->last_assigned;
  if ((!assign_out && !load_out) || n == 0) return DDDMR_OK;
  if (capacity < n) return fail(ctx, DDDMR_ERR_CAPACITY, "get_deal: capacity %zu < %zu", capacity, n);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (assign_out) {
    if (ctx->last_assigned) {
      HIPCHK(ctx, hipMemcpy(assign_out, ctx->assign, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    } else {
      for (size_t i = 0; i < n; ++i) assign_out[i] = (uint32_t)i;     // strided: slot s holds trajectory s
    }
  }
  if (load_out) HIPCHK(ctx, hipMemcpy(load_out, ctx->traj_load, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return DDDMR_OK;
}

int dddmr_rollout_get_debug(dddmr_rollout_ctx* ctx, dddmr_rollout_debug* dbg) {
  if (!ctx || !dbg) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (!ctx->have_last) return fail(ctx, DDDMR_ERR_STATE, "get_debug before any tick");
  if (ctx->pend.active) return refuse_pending(ctx, "get_debug");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // the tick may have returned on the polled sequence number
  const size_t n = (size_t)ctx->last.n_local;
  if (n == 0) return DDDMR_OK;
  if (dbg->costs) HIPCHK(ctx, hipMemcpy(dbg->costs, ctx->costs, n * sizeof(double), hipMemcpyDeviceToHost));
  if (dbg->steps) HIPCHK(ctx, hipMemcpy(dbg->steps, ctx->steps, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (dbg->samples) {
    std::vector<float4> tmp(n);
    HIPCHK(ctx, hipMemcpy(tmp.data(), ctx->samples_out, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
      dbg->samples[3 * i + 0] = tmp[i].x;
      dbg->samples[3 * i + 1] = tmp[i].y;
      dbg->samples[3 * i + 2] = tmp[i].z;
    }
  }
  return DDDMR_OK;
}

int dddmr_rollout_get_pose_arrays(dddmr_rollout_ctx* ctx, int32_t which, double* poses_out, size_t capacity,
                                  size_t* n_poses) {
  if (!ctx || !n_poses || (which != 0 && which != 1)) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (!ctx->have_last) return fail(ctx, DDDMR_ERR_STATE, "get_pose_arrays before any tick");
  if (ctx->pend.active) return refuse_pending(ctx, "get_pose_arrays");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const int n = ctx->last.n_local;
  *n_poses = 0;
  if (n <= 0) return DDDMR_OK;
  std::vector<int32_t> steps(n), off(n);
  std::vector<double> costs(n);
  HIPCHK(ctx, hipMemcpy(steps.data(), ctx->steps, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(costs.data(), ctx->costs, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    // generated: nextTrajectory returned true (steps > 0); accepted: cost_ >= 0 (local_planner.cpp:463)
    const bool want = steps[i] > 0 && (which == 0 || costs[i] >= 0.0);
    off[i] = want ? (int32_t)total : -1;
    if (want) total += (size_t)steps[i];
  }
  *n_poses = total;
  if (!poses_out || total == 0) return DDDMR_OK;
  if (capacity < total) return fail(ctx, DDDMR_ERR_CAPACITY, "get_pose_arrays: capacity %zu < %zu", capacity, total);
  if (total > (size_t)INT32_MAX) return fail(ctx, DDDMR_ERR_CAPACITY, "get_pose_arrays: %zu poses", total);
  DevScope tmp;
  int32_t* off_dev = nullptr;
  double* out_dev = nullptr;
  HIPCHK(ctx, dev_alloc(tmp.mem, &off_dev, (size_t)n));
  if (dev_alloc(tmp.mem, &out_dev, total * 7) != hipSuccess)
    return fail(ctx, DDDMR_ERR_HIP, "get_pose_arrays: out of device memory for %zu poses", total);
  const size_t pairs = (size_t)n * (size_t)ctx->last.max_steps;
  HIPCHK(ctx, hipMemcpyAsync(off_dev, off.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_pose_arrays, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, ctx->stream, ctx->last, off_dev,
                     ctx->steps, ctx->traj_info, ctx->st_sc, ctx->st_xy, out_dev);
  HIPCHK(ctx, hipMemcpyAsync(poses_out, out_dev, total * 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return DDDMR_OK;
}

// The last collected tick's winner on this rank, for get_best_poses / get_best_cuboids (tick_mu held): its local index
// and step count, with the stream idle.  *li < 0, *ns == 0: no winner, or it lives on another rank.
static int best_local(dddmr_rollout_ctx* ctx, const char* what, int* li, int32_t* ns) {
  *li = -1;
  *ns = 0;
  if (!ctx->have_last) return fail(ctx, DDDMR_ERR_STATE, "%s before any tick", what);
  if (ctx->pend.active) return refuse_pending(ctx, what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const int32_t idx = ctx->last_result.index;
  if (idx < 0) return DDDMR_OK;
  const int l = idx - ctx->last.begin;
  if (l < 0 || l >= ctx->last.n_local) return DDDMR_OK;  // winner is on another rank
  HIPCHK(ctx, hipMemcpy(ns, ctx->steps + l, sizeof(int32_t), hipMemcpyDeviceToHost));
  *li = l;
  return DDDMR_OK;
}

int dddmr_rollout_get_best_poses(dddmr_rollout_ctx* ctx, double* poses_out, size_t capacity, size_t* n_poses) {
  if (!ctx || !n_poses) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  int li;
  int32_t ns;
  const int rc = best_local(ctx, "get_best_poses", &li, &ns);
  if (rc != DDDMR_OK) return rc;
  *n_poses = (size_t)ns;
  if (li < 0 || !poses_out) return DDDMR_OK;
  if (capacity < (size_t)ns) return fail(ctx, DDDMR_ERR_CAPACITY, "get_best_poses: capacity %zu < %d", capacity, ns);
  hipLaunchKernelGGL(k_trajectory_poses, dim3(1), dim3(64), 0, ctx->stream, ctx->last, li, ctx->samples_out,
                     ctx->steps, ctx->poses_dev, (float*)nullptr);
  HIPCHK(ctx, hipMemcpyAsync(poses_out, ctx->poses_dev, (size_t)ns * 7 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return DDDMR_OK;
}

int dddmr_rollout_get_best_cuboids(dddmr_rollout_ctx* ctx, float* vertices_out, size_t capacity_poses, size_t* n_poses) {
  if (!ctx || !n_poses) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  int li;
  int32_t ns;
  const int rc = best_local(ctx, "get_best_cuboids", &li, &ns);
  if (rc != DDDMR_OK) return rc;
  *n_poses = (size_t)ns;
  if (li < 0 || !vertices_out || ns == 0) return DDDMR_OK;
  if (capacity_poses < (size_t)ns) return fail(ctx, DDDMR_ERR_CAPACITY, "get_best_cuboids: capacity %zu < %d", capacity_poses, ns);
  DevScope tmp;
  float* cub_dev = nullptr;
  HIPCHK(ctx, dev_alloc(tmp.mem, &cub_dev, (size_t)ns * 24));
  hipLaunchKernelGGL(k_trajectory_poses, dim3(1), dim3(64), 0, ctx->stream, ctx->last, li, ctx->samples_out,
                     ctx->steps, ctx->poses_dev, cub_dev);
  HIPCHK(ctx, hipMemcpyAsync(vertices_out, cub_dev, (size_t)ns * 24 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return DDDMR_OK;
}

}  // extern "C"

#include "rollout_diag.hip.h"
#include "sensor_sources.hip.h"
#include "marking_host.hip.h"
#include "depth_mark.hip.h"
#include "depth_layer.hip.h"
#include "perception_stack.hip.h"
#include "mcl_measure.hip.h"
#include "mcl_observation.hip.h"
#include "mcl_submap.hip.h"
#include "mcl_filter.hip.h"
#include "static_layer.hip.h"
#include "global_plan.hip.h"
#include "global_plan_cloud.hip.h"
