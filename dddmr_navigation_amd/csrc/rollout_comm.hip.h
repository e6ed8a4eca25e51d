// rollout_comm.hip.h -- the multi-rank exchange of rollout_engine.hip: the RCCL loader and the dddmr_rollout_comm_* entry
// points (a communicator of the library's own, or its single-device rehearsal, the loopback).  Included by
// rollout_engine.hip after the context and its helpers are defined; the tick itself enqueues the collective.
#pragma once

namespace {

// RCCL entry points, resolved at run time: the engine has no link-time dependency on librccl (hosts
// that never call dddmr_rollout_comm_init do not need it), and a process that already holds a copy --
// PyTorch ships its own librccl.so -- shares it instead of loading a second one.
struct Rccl {
  void* handle = nullptr;
  ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
  ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
  ncclResult_t (*comm_count)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*error_string)(ncclResult_t) = nullptr;
  std::string why;
  bool ok() const { return handle != nullptr; }
};
Rccl& rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* h = nullptr;
    if (const char* e = std::getenv("DDDMR_RCCL_LIB")) h = dlopen(e, RTLD_NOW | RTLD_GLOBAL);
    for (const char* n : names) {
      if (h) break;
      h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!h) { r.why = std::string("librccl not found: ") + (dlerror() ? dlerror() : "?"); return; }
    r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
    r.comm_init_rank = reinterpret_cast<decltype(r.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
    r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
    r.comm_count = reinterpret_cast<decltype(r.comm_count)>(dlsym(h, "ncclCommCount"));
    r.all_reduce = reinterpret_cast<decltype(r.all_reduce)>(dlsym(h, "ncclAllReduce"));
    r.error_string = reinterpret_cast<decltype(r.error_string)>(dlsym(h, "ncclGetErrorString"));
    if (!r.get_unique_id || !r.comm_init_rank || !r.comm_destroy || !r.comm_count || !r.all_reduce || !r.error_string) {
      r.why = "librccl lacks an expected symbol";
      return;
    }
    r.handle = h;
  });
  return r;
}

}  // namespace

extern "C" {

int dddmr_rollout_comm_unique_id(uint8_t id_out[DDDMR_COMM_ID_BYTES]) {
  static_assert(DDDMR_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  if (!id_out) return DDDMR_ERR_BAD_ARG;
  if (!rccl().ok()) return DDDMR_ERR_NO_DEVICE;
  ncclUniqueId id;
  if (rccl().get_unique_id(&id) != ncclSuccess) return DDDMR_ERR_HIP;
  std::memcpy(id_out, id.internal, DDDMR_COMM_ID_BYTES);
  return DDDMR_OK;
}

// slot vectors of the per-tick exchange: [2 * n_ranks] words to send (own pair written by k_score / k_finalize,
// INT64_MAX elsewhere: the other ranks' slots never change) and to receive
static int alloc_exchange_buffers(dddmr_rollout_ctx* ctx, int n_ranks) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, dev_realloc(ctx->mem, &ctx->slots_dev, (size_t)2 * n_ranks));      // (re-initialisation after comm_destroy)
  HIPCHK(ctx, dev_realloc(ctx->mem, &ctx->slots_red, (size_t)2 * n_ranks));
  HIPCHK(ctx, dev_realloc(ctx->mem, &ctx->local_result_dev, 1));
  std::vector<int64_t> none((size_t)2 * n_ranks, INT64_MAX);
  HIPCHK(ctx, hipMemcpy(ctx->slots_dev, none.data(), none.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(ctx->slots_red, none.data(), none.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  return DDDMR_OK;
}

int dddmr_rollout_comm_init(dddmr_rollout_ctx* ctx, const uint8_t id[DDDMR_COMM_ID_BYTES], int32_t rank, int32_t n_ranks) {
  if (!ctx || !id) return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "comm_init");
  if (ctx->comm) return fail(ctx, DDDMR_ERR_STATE, "comm_init: the context already has a communicator");
  const int world = std::max(1, ctx->cfg.world_size);
  if (n_ranks != world || rank != std::min(std::max(0, ctx->cfg.rank), world - 1))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "comm_init: rank %d of %d does not match the context's shard (rank %d of %d)", rank,
                n_ranks, ctx->cfg.rank, world);
  if (ctx->comm_loopback) return fail(ctx, DDDMR_ERR_STATE, "comm_init: the context is in loopback mode");
  if (!rccl().ok()) return fail(ctx, DDDMR_ERR_NO_DEVICE, "comm_init: %s", rccl().why.c_str());
  const int ab = alloc_exchange_buffers(ctx, n_ranks);
  if (ab != DDDMR_OK) return ab;
  ncclUniqueId uid;
  std::memcpy(uid.internal, id, DDDMR_COMM_ID_BYTES);
  ncclComm_t comm = nullptr;
  const ncclResult_t rc = rccl().comm_init_rank(&comm, n_ranks, uid, rank);     // collective: every rank calls it
  if (rc != ncclSuccess) return fail(ctx, DDDMR_ERR_HIP, "ncclCommInitRank failed: %s", rccl().error_string(rc));
  ctx->comm = comm;
  ctx->comm_ranks = n_ranks;
  return DDDMR_OK;
}

int dddmr_rollout_comm_destroy(dddmr_rollout_ctx* ctx) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "comm_destroy");
  if (!ctx->comm && !ctx->comm_loopback) return DDDMR_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->comm) (void)rccl().comm_destroy(ctx->comm);
  ctx->comm = nullptr;
  ctx->comm_loopback = false;
  ctx->comm_ranks = 0;
  return DDDMR_OK;
}

int dddmr_rollout_comm_ranks(dddmr_rollout_ctx* ctx, int32_t* n_ranks_out) {
  if (!ctx || !n_ranks_out) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  *n_ranks_out = 0;
  if (ctx->comm_loopback) { *n_ranks_out = ctx->comm_ranks; return DDDMR_OK; }
  if (!ctx->comm) return DDDMR_OK;
  int n = 0;
  const ncclResult_t rc = rccl().comm_count(ctx->comm, &n);      // what RCCL itself says, not what we asked for
  if (rc != ncclSuccess) return fail(ctx, DDDMR_ERR_HIP, "ncclCommCount failed: %s", rccl().error_string(rc));
  *n_ranks_out = n;
  return DDDMR_OK;
}

int dddmr_rollout_comm_loopback(dddmr_rollout_ctx* ctx) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  TICK_IDLE(ctx, "comm_loopback");
  if (ctx->comm || ctx->comm_loopback) return fail(ctx, DDDMR_ERR_STATE, "comm_loopback: the context already has an exchange");
  const int world = std::max(1, ctx->cfg.world_size);
  const int ab = alloc_exchange_buffers(ctx, world);
  if (ab != DDDMR_OK) return ab;
  ctx->comm_loopback = true;
  ctx->comm_ranks = world;
  return DDDMR_OK;
}

int dddmr_rollout_comm_loopback_set_peer(dddmr_rollout_ctx* ctx, int32_t peer_rank, const int64_t words[2]) {
  if (!ctx || !words) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> tk(ctx->tick_mu);
  if (!ctx->comm_loopback) return fail(ctx, DDDMR_ERR_STATE, "comm_loopback_set_peer: the context is not in loopback mode");
  if (ctx->pend.active) return refuse_pending(ctx, "comm_loopback_set_peer");
  const int world = ctx->comm_ranks, rank = std::min(std::max(0, ctx->cfg.rank), world - 1);
  if (peer_rank < 0 || peer_rank >= world || peer_rank == rank)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "comm_loopback_set_peer: peer %d of %d (own rank %d)", peer_rank, world, rank);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemcpy(ctx->slots_dev + 2 * peer_rank, words, 2 * sizeof(int64_t), hipMemcpyHostToDevice));
  return DDDMR_OK;
}

}  // extern "C"
