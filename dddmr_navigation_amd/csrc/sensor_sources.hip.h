// sensor_sources.hip.h -- the host half of the sensor sources: the entry points that configure and feed them (scans and
// stitchers, depth clouds and images, lidar sweeps and their features), read their products back, and the depth
// sources' frustums, point tests and clearing verdicts.  Included at the bottom of rollout_engine.hip, which keeps the
// cloud triple buffer (publish_cloud, acquire_back) the aggregate is published through.
//
// What a source is and how many points it has is written down in the context's SourceTable (source_table.hip.h); what it
// owns on the device in ctx->src[].  Everything here runs under producer_mu and does its device work on copy_stream.
// A new observation of any kind reaches the aggregate through commit_source().
#pragma once

namespace {

// The one check of a source id: "<what>: source <id> (at most <max> sensors)<suffix>".  others_ok false: an argument the
// caller reports with the same message (the suffix names it) is missing.
int source_arg(dddmr_rollout_ctx* ctx, const char* what, int id, const char* suffix = "", bool others_ok = true) {
  if (others_ok && SourceTable::valid(id)) return DDDMR_OK;
  return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: source %d (at most %d sensors)%s", what, id, dddmr_rollout_ctx::kMaxSources, suffix);
}

// Does the kind source id already has refuse the call?  producer_mu held.
int source_refused(dddmr_rollout_ctx* ctx, const char* what, SourceOp op, int id) {
  const Refusal r = ctx->sources.refuse(op, id);
  return r.code == DDDMR_OK ? DDDMR_OK : fail(ctx, r.code, "%s: source %d %s", what, id, r.why);
}

// the mounts of a feed: sensor -> base and base -> global, as rotation matrix and translation
template <typename Params>
void set_mounts(Params& p, const double T_base_sensor[7], const double T_gbl_base[7]) {
  quat_to_rot(T_base_sensor, p.Rbs);
  quat_to_rot(T_gbl_base, p.Rgb);
  for (int i = 0; i < 3; ++i) {
    p.tbs[i] = T_base_sensor[i];
    p.tgb[i] = T_gbl_base[i];
  }
}

// A getter's tail: report the count; with an output, check its capacity, copy on copy_stream and wait.  producer_mu held.
int read_back(dddmr_rollout_ctx* ctx, const char* what, void* out, const void* dev, uint32_t count, size_t elem_bytes, size_t capacity,
              size_t* n_out) {
  *n_out = count;
  if (!out) return DDDMR_OK;
  if (capacity < count) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu < %u", what, capacity, count);
  if (count) {                                         // (one enqueue and its wait: no exit lies between them)
    HIPCHK(ctx, hipMemcpyAsync(out, dev, (size_t)count * elem_bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  }
  return DDDMR_OK;
}

// How every module state below is made: in a unique_ptr of its own, which moves into its slot once the state is complete.
// One that could not be allocated in full frees what it got as the pointer goes out of scope (Owned, dev_memory.hip.h);
// resetting the slot is the whole teardown.

// the feed scratch (stitcher state, staging) of a scan source above 0, allocated on first use
int scan_scratch(dddmr_rollout_ctx* ctx, const char* what, int id, PerceptionScratch** out) {
  SourceOwned& own = ctx->src[id];
  if (!own.feed) {
    auto ps = std::make_unique<PerceptionScratch>();
    if (perception_alloc(*ps, ctx->cfg.max_points) != 0) return fail(ctx, DDDMR_ERR_HIP, "%s: scratch of source %d", what, id);
    own.feed = std::move(ps);
  }
  *out = own.feed.get();
  return DDDMR_OK;
}

// Tear a source of any kind down: its record is cleared (its points leave the next aggregate) and what it owns is freed,
// here and nowhere else.  The caller has synchronised copy_stream: no device work still reads the source's buffers.
void release_source(dddmr_rollout_ctx* ctx, int id) {
  ctx->src[id] = SourceOwned{};
  ctx->sources.release(id);
}

// The aggregate = every source's current observation in source order (aggregateObservations' loop over the plugins),
// into a back buffer, published.  producer_mu held; the counts fit max_points (commit_source has checked).
int publish_sources(dddmr_rollout_ctx* ctx, uint32_t* n_aggregate) {
  const int back = acquire_back(ctx);
  const SourceLayout L = ctx->sources.layout();
  Drain drain{ctx->copy_stream};                       // an error exit leaves no copy behind that reads a source's buffer
  for (int i = 0; i < SourceTable::kMax; ++i) {
    if (!L.n[i]) continue;
    HIPCHK(ctx, hipMemcpyAsync(ctx->cloud_dev[back] + L.at[i], ctx->src[i].obs, (size_t)L.n[i] * sizeof(float4), hipMemcpyDeviceToDevice, ctx->copy_stream));
  }
  // the tick's stream waits on this event, so the work that built the observations need not have retired yet
  HIPCHK(ctx, hipEventRecord(ctx->cloud_ready[back], ctx->copy_stream));
  drain.armed = false;                                 // (success never waits here)
  publish_cloud(ctx, back, L.total, L);
  *n_aggregate = L.total;
  return DDDMR_OK;
}

// The one way a source's new observation reaches the aggregate: obs / n are the candidate (built, not yet current).
// Refused with DDDMR_ERR_CAPACITY when it does not fit beside the other sources' observations; otherwise the source
// switches over and the aggregate is rebuilt and published.  After a failed copy the source is back to what the published
// aggregate holds.  Nothing of the source's own state has to be touched before this returns DDDMR_OK.  producer_mu held.
int commit_source(dddmr_rollout_ctx* ctx, const char* what, int id, float4* obs, size_t n, uint32_t* n_aggregate) {
  size_t total;
  if (!ctx->sources.would_fit(id, n, ctx->cfg.max_points, &total))
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: the sensors' observations together (%zu points) exceed max_points %u", what, total, ctx->cfg.max_points);
  float4* const old_obs = ctx->src[id].obs;
  const uint32_t old_n = ctx->sources.rec[id].n;
  ctx->src[id].obs = obs;
  ctx->sources.set_count(id, (uint32_t)n);
  const int rc = publish_sources(ctx, n_aggregate);
  if (rc != DDDMR_OK) {
    ctx->src[id].obs = old_obs;
    ctx->sources.rec[id].n = old_n;
  }
  return rc;
}

// The two halves of configuring a depth or sweep source.  Configuring a configured source empties it: what it owned is
// released once the device is done with it ...
int configure_begin(dddmr_rollout_ctx* ctx, int id, bool* had_points) {
  *had_points = ctx->sources.rec[id].n != 0;
  if (ctx->sources.rec[id].kind == SourceKind::kNone) return DDDMR_OK;
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  release_source(ctx, id);
  return DDDMR_OK;
}
// ... and, whether or not the new scratch could be allocated (rc), the aggregate loses the emptied source's segment.
int configure_end(dddmr_rollout_ctx* ctx, const char* what, int id, bool had_points, int rc) {
  if (!had_points) return rc;
  uint32_t n_all;
  const int prc = commit_source(ctx, what, id, ctx->src[id].obs, 0, &n_all);
  return rc == DDDMR_OK ? prc : rc;
}

}  // namespace

extern "C" {

// one sensor's scan through the feed; source < 0: the single-producer form (the result replaces the aggregate)
static int set_scan_impl(dddmr_rollout_ctx* ctx, int source, const float* xyz, size_t n_points, size_t stride_bytes,
                         const double T_base_sensor[7], const double T_gbl_base[7], double perception_window_size,
                         double marking_height, uint32_t* n_out_points, uint32_t* n_aggregate) {
  if (!ctx || !T_base_sensor || !T_gbl_base) return DDDMR_ERR_BAD_ARG;
  int rc;
  if (source >= 0 && (rc = source_arg(ctx, "set_scan", source)) != DDDMR_OK) return rc;
  if (!cloud_arg_ok(xyz, n_points, stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "set_scan: bad pointer/stride");
  if (n_points > ctx->cfg.max_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "set_scan: %zu points > max_points %u", n_points, ctx->cfg.max_points);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  SourceTable& table = ctx->sources;
  source = table.scan_source(source);                  // once several sensors feed, plain set_scan is sensor 0
  if ((rc = source_refused(ctx, "set_scan", SourceOp::kFeedScan, std::max(source, 0))) != DDDMR_OK) return rc;
  if (source < 0) table.note_scan(source);             // the single-producer form is the lidar of source 0
  PerceptionScratch* scratch = &ctx->feed;
  if (source > 0 && (rc = scan_scratch(ctx, "set_scan", source, &scratch)) != DDDMR_OK) return rc;
  if (scratch->stitcher_num > 0 && n_points == 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "set_scan: empty scan with the stitcher on");
  SourceOwned* own = source >= 0 ? &ctx->src[source] : nullptr;
  if (own) {
    table.note_scan(source);
    if (!own->obs) HIPCHK(ctx, dev_alloc(own->scan_obs.dev, &own->obs, std::max<uint32_t>(ctx->cfg.max_points, 1)));
  }
  const int back = own ? -1 : acquire_back(ctx);       // the single-producer form feeds straight into the back buffer
  FeedParams fp;
  set_mounts(fp, T_base_sensor, T_gbl_base);
  fp.n = (int)n_points;
  fp.window = (float)perception_window_size;
  fp.height = (float)marking_height;
  uint32_t n_out = 0, n_all = 0;
  rc = perception_feed(*scratch, fp, xyz, stride_bytes, own ? own->obs : ctx->cloud_dev[back], ctx->copy_stream, &n_out);
  if (rc == -2) return fail(ctx, DDDMR_ERR_CAPACITY, "set_scan: the (stitched) scan exceeds max_points %u", ctx->cfg.max_points);
  if (rc != 0) return fail(ctx, DDDMR_ERR_HIP, "set_scan: perception feed failed (%d)", rc);
  if (own) {
    rc = commit_source(ctx, "set_scan", source, own->obs, n_out, &n_all);
    if (rc == DDDMR_ERR_CAPACITY) {
      // A scan source has one observation buffer and the feed has overwritten it: the old count cannot come back.  The
      // source is left empty and the aggregate republished from the others, so they feed on and this one works again
      // as soon as its observation fits.
      table.set_count(source, 0);
      const int prc = publish_sources(ctx, &n_all);
      if (prc != DDDMR_OK) return prc;
    }
    if (rc != DDDMR_OK) return rc;
  } else {
    // the tick's stream waits on this event, so the feed kernels need not have retired yet
    HIPCHK(ctx, hipEventRecord(ctx->cloud_ready[back], ctx->copy_stream));
    publish_cloud(ctx, back, n_out, single_lidar_layout(n_out));
    n_all = n_out;
  }
  if (n_out_points) *n_out_points = n_out;
  if (n_aggregate) *n_aggregate = n_all;
  return DDDMR_OK;
}

int dddmr_rollout_set_scan(dddmr_rollout_ctx* ctx, const float* xyz, size_t n_points,
                           size_t stride_bytes, const double T_base_sensor[7],
                           const double T_gbl_base[7], double perception_window_size,
                           double marking_height, uint32_t* n_out_points) {
  return set_scan_impl(ctx, -1, xyz, n_points, stride_bytes, T_base_sensor, T_gbl_base, perception_window_size, marking_height, n_out_points, nullptr);
}

int dddmr_rollout_set_scan_source(dddmr_rollout_ctx* ctx, int32_t source_id, const float* xyz, size_t n_points,
                                  size_t stride_bytes, const double T_base_sensor[7], const double T_gbl_base[7],
                                  double perception_window_size, double marking_height, uint32_t* n_source_points,
                                  uint32_t* n_aggregate_points) {
  if (source_id < 0) return ctx ? fail(ctx, DDDMR_ERR_BAD_ARG, "set_scan_source: source %d", source_id) : DDDMR_ERR_BAD_ARG;
  return set_scan_impl(ctx, source_id, xyz, n_points, stride_bytes, T_base_sensor, T_gbl_base, perception_window_size, marking_height,
                       n_source_points, n_aggregate_points);
}

int dddmr_rollout_set_stitcher_source(dddmr_rollout_ctx* ctx, int32_t source_id, int32_t stitcher_num) {
  if (!ctx || stitcher_num < 0 || !SourceTable::valid(source_id)) return DDDMR_ERR_BAD_ARG;
  if (source_id > 0) HIPCHK(ctx, hipSetDevice(ctx->device));   // its scratch may have to be allocated
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  int rc = source_refused(ctx, "set_stitcher", SourceOp::kSetStitcher, source_id);
  if (rc != DDDMR_OK) return rc;
  PerceptionScratch* scratch = &ctx->feed;
  if (source_id > 0 && (rc = scan_scratch(ctx, "set_stitcher", source_id, &scratch)) != DDDMR_OK) return rc;
  scratch->stitcher_num = stitcher_num;
  scratch->stitched.clear();
  ctx->sources.note_stitcher(source_id, stitcher_num);
  return DDDMR_OK;
}

int dddmr_rollout_set_stitcher(dddmr_rollout_ctx* ctx, int32_t stitcher_num) {
  return dddmr_rollout_set_stitcher_source(ctx, 0, stitcher_num);
}

// ---------------------------------------------------------------------------
// Depth camera sources: DepthCameraLayer::getObservation in local mode (depth_feed.hip.h)
// ---------------------------------------------------------------------------
// icfg == nullptr: a source fed point clouds; otherwise one fed depth images
static int set_depth_source_impl(dddmr_rollout_ctx* ctx, const char* what, int32_t source_id, const dddmr_depth_source_config* cfg,
                                 const dddmr_depth_image_config* icfg) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  int rc = source_arg(ctx, what, source_id, " / null config", cfg != nullptr);
  if (rc != DDDMR_OK) return rc;
  if (!(cfg->min_obstacle_height <= cfg->max_obstacle_height) || cfg->observation_persistence_ns < 0 || cfg->max_frame_points == 0 ||
      cfg->max_frames == 0)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: bad height band / persistence / capacities", what);
  if (cfg->max_frame_points > (1u << 28)) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: max_frame_points %u", what, cfg->max_frame_points);
  DimgParams ip{};
  if (icfg) {
    if (icfg->width == 0 || icfg->height == 0 || icfg->width > 16384 || icfg->height > 16384 || icfg->sample_step == 0 ||
        (icfg->flags & ~DDDMR_DEPTH_IMAGE_DROP_ZERO) != 0)
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: image %u x %u, sample_step %u, flags %#x", what, icfg->width, icfg->height,
                  icfg->sample_step, icfg->flags);
    if (!std::isfinite(icfg->fx) || !std::isfinite(icfg->fy) || icfg->fx == 0.0 || icfg->fy == 0.0 || !std::isfinite(icfg->cx) ||
        !std::isfinite(icfg->cy) || !(icfg->max_distance > 0.0) || !(icfg->leaf_size > 0.0) || !std::isfinite(icfg->leaf_size))
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: bad intrinsics / max_distance / leaf_size", what);
    // cbDepthImg:111-114: float cx = K[2], cy = K[5], fx = 1.0f / K[0], fy = 1.0f / K[4] (double division, float result)
    ip.cx = (float)icfg->cx;
    ip.cy = (float)icfg->cy;
    ip.fx = (float)(1.0 / icfg->fx);
    ip.fy = (float)(1.0 / icfg->fy);
    ip.inv_leaf = 1.0f / (float)icfg->leaf_size;      // pcl::VoxelGrid::setLeafSize(float ...): inverse_leaf_size_ = 1 / leaf_size_
    ip.drop_zero = (icfg->flags & DDDMR_DEPTH_IMAGE_DROP_ZERO) ? 1u : 0u;
    ip.max_distance = icfg->max_distance;
    ip.width = icfg->width;
    ip.step = icfg->sample_step;
    ip.cols = (icfg->width + icfg->sample_step - 1) / icfg->sample_step;
    ip.rows = (icfg->height + icfg->sample_step - 1) / icfg->sample_step;
    if (!std::isfinite(ip.inv_leaf) || !std::isfinite(ip.fx) || !std::isfinite(ip.fy) || !dimg_box_ok(ip, icfg->height))
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: the frustum's voxel box (intrinsics, max_distance %g, leaf_size %g) could reach 2^31 cells",
                  what, icfg->max_distance, icfg->leaf_size);
    if ((uint64_t)ip.rows * ip.cols > cfg->max_frame_points)
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: max_frame_points %u < the %u x %u sampled pixels", what, cfg->max_frame_points, ip.rows, ip.cols);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if ((rc = source_refused(ctx, what, SourceOp::kConfigureDepth, source_id)) != DDDMR_OK) return rc;
  bool had_points;
  if ((rc = configure_begin(ctx, source_id, &had_points)) != DDDMR_OK) return rc;   // (the frustum leaves with the observations)
  auto ds = std::make_unique<DepthSource>();
  ds->zmin = cfg->min_obstacle_height;
  ds->zmax = cfg->max_obstacle_height;
  ds->persistence_ns = cfg->observation_persistence_ns;
  ds->max_frame_points = cfg->max_frame_points;
  ds->max_frames = cfg->max_frames;
  std::unique_ptr<DepthImage> di;
  if (icfg) {
    di = std::make_unique<DepthImage>();
    di->p = ip;
    di->height = icfg->height;
  }
  if (depth_alloc(*ds, ctx->cfg.max_points, icfg == nullptr) != 0 || (di && dimg_alloc(*di) != 0)) {
    rc = fail(ctx, DDDMR_ERR_HIP, "%s: scratch of source %d", what, source_id);
  } else {
    ctx->src[source_id].obs = ds->buf[ds->cur];
    ctx->sources.configure(source_id, di ? SourceKind::kDepthImage : SourceKind::kDepthCloud);
    ctx->src[source_id].depth = std::move(ds);
    ctx->src[source_id].dimg = std::move(di);
  }
  return configure_end(ctx, what, source_id, had_points, rc);
}

int dddmr_rollout_set_depth_source(dddmr_rollout_ctx* ctx, int32_t source_id, const dddmr_depth_source_config* cfg) {
  return set_depth_source_impl(ctx, "set_depth_source", source_id, cfg, nullptr);
}

int dddmr_rollout_set_depth_image_source(dddmr_rollout_ctx* ctx, int32_t source_id, const dddmr_depth_source_config* cfg,
                                         const dddmr_depth_image_config* image_cfg) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!image_cfg) return fail(ctx, DDDMR_ERR_BAD_ARG, "set_depth_image_source: null image config");
  return set_depth_source_impl(ctx, "set_depth_image_source", source_id, cfg, image_cfg);
}

// One frame of either kind: xyz (a cloud source) or depth_mm (an image source) is set.  bufferCloud's bookkeeping around
// the device work is the same for both.
static int set_depth_impl(dddmr_rollout_ctx* ctx, const char* what, int32_t source_id, const float* xyz, size_t n_points,
                          const uint16_t* depth_mm, size_t stride_bytes, const double T_base_sensor[7], const double T_gbl_base[7],
                          int64_t stamp_ns, uint32_t* n_camera_points, uint32_t* n_frame_points, uint32_t* n_source_points,
                          uint32_t* n_aggregate_points) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  int rc = source_refused(ctx, what, depth_mm ? SourceOp::kFeedImage : SourceOp::kFeedFrame, source_id);
  if (rc != DDDMR_OK) return rc;
  DepthSource* ds = ctx->src[source_id].depth.get();
  DepthImage* di = ctx->src[source_id].dimg.get();
  if (depth_mm && stride_bytes < 2 * (size_t)di->p.width)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: row stride %zu < 2 * width %u", what, stride_bytes, di->p.width);
  if (n_points > ds->max_frame_points)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu points > max_frame_points %u", what, n_points, ds->max_frame_points);
  // purgeStaleObservations (depth_camera_observation_buffer.cpp:203-231) with last_updated_ = stamp_ns decides from
  // the stamps alone, so which observations stay is known before the frame is processed
  const int64_t stamp_us = stamp_ns / 1000;          // pcl_conversions::toPCL keeps whole microseconds
  auto stays = [&](int64_t us, bool newest) {
    if (ds->persistence_ns == 0) return newest;      // "keeping observations for no time": only the newest one
    return !(stamp_ns - us * 1000 > ds->persistence_ns);
  };
  std::vector<DepthFrame> kept;
  size_t kept_points = 0;
  for (const DepthFrame& fr : ds->frames)
    if (stays(fr.stamp_us, false)) { kept.push_back(fr); kept_points += fr.n; }
  const bool none_leaves = kept.size() == ds->frames.size();
  const bool new_alive = stays(stamp_us, true);
  if (kept.size() + (new_alive ? 1 : 0) > ds->max_frames)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: %zu observations alive > max_frames %u", what, kept.size() + 1, ds->max_frames);
  // Nothing leaves: the frame is appended behind the alive ones.  Otherwise the ones that stay are copied to the
  // other buffer (device to device) and the frame is built behind them; the buffers swap on success only.
  const int dst_buf = none_leaves ? ds->cur : ds->cur ^ 1;
  // From the first copy on, an error exit waits for what is enqueued (the feed's -2 and a refused commit leave the copies
  // behind).  Disarmed once the source is committed: the feed has waited, and the aggregate's copies are ordered by event.
  Drain drain{ctx->copy_stream, false};
  if (!none_leaves) {
    drain.armed = true;
    size_t src_at = 0, dst_at = 0;
    for (const DepthFrame& fr : ds->frames) {        // the caller's stamps need not be monotonic: any frame may be the one to leave
      if (stays(fr.stamp_us, false) && fr.n) {
        HIPCHK(ctx, hipMemcpyAsync(ds->buf[dst_buf] + dst_at, ds->buf[ds->cur] + src_at, (size_t)fr.n * sizeof(float4), hipMemcpyDeviceToDevice, ctx->copy_stream));
        dst_at += fr.n;
      }
      src_at += fr.n;
    }
  }
  DepthParams dp;
  set_mounts(dp, T_base_sensor, T_gbl_base);
  dp.zmin = ds->zmin;
  dp.zmax = ds->zmax;
  dp.n = (int)n_points;
  uint32_t n_out = 0, n_camera = 0;
  rc = di ? depth_image_feed(*ds, *di, dp, depth_mm, stride_bytes, ds->buf[dst_buf] + kept_points, ctx->copy_stream, &n_camera, &n_out)
          : depth_feed(*ds, dp, xyz, stride_bytes, ds->buf[dst_buf] + kept_points, ctx->copy_stream, &n_out);
  if (rc != 0) return fail(ctx, DDDMR_ERR_HIP, "%s: depth feed failed (%d)", what, rc);
  const size_t n_source = kept_points + (new_alive ? n_out : 0);
  uint32_t n_all = 0;
  if ((rc = commit_source(ctx, what, source_id, ds->buf[dst_buf], n_source, &n_all)) != DDDMR_OK) return rc;
  drain.armed = false;
  // committed (the clearing verdicts' grid is rebuilt by the next call that needs it): the source's frames follow
  if (new_alive) kept.push_back(DepthFrame{n_out, stamp_us});
  ds->frames.swap(kept);
  ds->cur = dst_buf;
  if (di) {                                          // the stage-one cloud of an accepted image becomes the source's latest
    di->cur ^= 1;
    di->n_cloud = n_camera;
  }
  if (n_camera_points) *n_camera_points = n_camera;
  if (n_frame_points) *n_frame_points = n_out;
  if (n_source_points) *n_source_points = (uint32_t)n_source;
  if (n_aggregate_points) *n_aggregate_points = n_all;
  return DDDMR_OK;
}

int dddmr_rollout_set_depth_frame(dddmr_rollout_ctx* ctx, int32_t source_id, const float* xyz, size_t n_points,
                                  size_t stride_bytes, const double T_base_sensor[7], const double T_gbl_base[7],
                                  int64_t stamp_ns, uint32_t* n_frame_points, uint32_t* n_source_points,
                                  uint32_t* n_aggregate_points) {
  if (!ctx || !T_base_sensor || !T_gbl_base) return DDDMR_ERR_BAD_ARG;
  if (const int arc = source_arg(ctx, "set_depth_frame", source_id)) return arc;
  if (!cloud_arg_ok(xyz, n_points, stride_bytes))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "set_depth_frame: bad pointer/stride");
  return set_depth_impl(ctx, "set_depth_frame", source_id, xyz, n_points, nullptr, stride_bytes, T_base_sensor, T_gbl_base, stamp_ns,
                        nullptr, n_frame_points, n_source_points, n_aggregate_points);
}

int dddmr_rollout_set_depth_image(dddmr_rollout_ctx* ctx, int32_t source_id, const uint16_t* depth_mm, size_t row_stride_bytes,
                                  const double T_base_optical[7], const double T_gbl_base[7], int64_t stamp_ns,
                                  uint32_t* n_camera_points, uint32_t* n_frame_points, uint32_t* n_source_points,
                                  uint32_t* n_aggregate_points) {
  if (!ctx || !T_base_optical || !T_gbl_base) return DDDMR_ERR_BAD_ARG;
  if (const int arc = source_arg(ctx, "set_depth_image", source_id)) return arc;
  if (!depth_mm) return fail(ctx, DDDMR_ERR_BAD_ARG, "set_depth_image: null image");
  return set_depth_impl(ctx, "set_depth_image", source_id, nullptr, 0, depth_mm, row_stride_bytes, T_base_optical, T_gbl_base, stamp_ns,
                        n_camera_points, n_frame_points, n_source_points, n_aggregate_points);
}

int dddmr_rollout_get_depth_image_cloud(dddmr_rollout_ctx* ctx, int32_t source_id, float* xyz_out, size_t capacity, size_t* n_points) {
  if (!ctx || !n_points) return DDDMR_ERR_BAD_ARG;
  if (const int arc = source_arg(ctx, "get_depth_image_cloud", source_id)) return arc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if (const int rc = source_refused(ctx, "get_depth_image_cloud", SourceOp::kImageCloudGetter, source_id)) return rc;
  const DepthImage* di = ctx->src[source_id].dimg.get();
  return read_back(ctx, "get_depth_image_cloud", xyz_out, di->cloud[di->cur], di->n_cloud, 3 * sizeof(float), capacity, n_points);
}

// ---------------------------------------------------------------------------
// Lidar sweep sources: the front half of ImageProjection::cloudHandler, then cbSensor (lidar_sweep.hip.h)
// ---------------------------------------------------------------------------
int dddmr_rollout_set_lidar_sweep_source(dddmr_rollout_ctx* ctx, int32_t source_id, const dddmr_lidar_sweep_config* cfg) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "set_lidar_sweep_source";
  int rc = source_arg(ctx, what, source_id, " / null config", cfg != nullptr);
  if (rc != DDDMR_OK) return rc;
  const uint32_t V = cfg->num_vertical_scans, H = cfg->num_horizontal_scans;
  if (V < 2 || H < 4 || cfg->ground_scan_index >= V || !(cfg->vertical_angle_top > cfg->vertical_angle_bottom) ||
      !(cfg->minimum_detection_range < cfg->maximum_detection_range) || cfg->flags != 0)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: image %u x %u, ground_scan_index %u, angles %g .. %g, range %g .. %g, flags %#x", what, V, H,
                cfg->ground_scan_index, cfg->vertical_angle_bottom, cfg->vertical_angle_top, cfg->minimum_detection_range,
                cfg->maximum_detection_range, cfg->flags);
  if (!std::isfinite(cfg->vertical_angle_bottom) || !std::isfinite(cfg->vertical_angle_top) || !std::isfinite(cfg->segment_theta) ||
      !std::isfinite(cfg->minimum_detection_range) || !std::isfinite(cfg->maximum_detection_range) || !std::isfinite(cfg->sensor_mount_angle))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: non-finite parameter", what);
  if (V > kSweepMaxRows || H > kSweepMaxCols || (uint64_t)V * H > kSweepMaxPixels || cfg->max_sweep_points > kSweepMaxPoints)
    return fail(ctx, DDDMR_ERR_CAPACITY, "%s: image %u x %u (at most %u x %u, %u pixels), max_sweep_points %u (at most %u)", what, V, H,
                kSweepMaxRows, kSweepMaxCols, kSweepMaxPixels, cfg->max_sweep_points, kSweepMaxPoints);
  // the constructor's conversions (imageProjection.cpp:67-125 into the members of imageProjection.h:67-107)
  const double kDegToRad = M_PI / 180.0;                         // utility.h:51
  SweepParams k{};
  const float bottom = (float)cfg->vertical_angle_bottom, top = (float)cfg->vertical_angle_top;
  k.V = V;
  k.H = H;
  k.gsi = cfg->ground_scan_index;
  k.res_x = (float)((M_PI * 2) / (int)H);
  k.res_y = (float)(kDegToRad * (double)(top - bottom) / (double)(float)((int)V - 1));
  k.ang_bottom = (float)(-((double)bottom - 0.1) * kDegToRad);
  float theta = (float)cfg->segment_theta;
  theta = (float)((double)theta * kDegToRad);
  k.tan_theta = std::tan(theta);                                 // float overloads on float arguments
  k.sin_x = std::sin(k.res_x);
  k.cos_x = std::cos(k.res_x);
  k.sin_y = std::sin(k.res_y);
  k.cos_y = std::cos(k.res_y);
  k.min_range = (float)cfg->minimum_detection_range;
  k.max_range = (float)cfg->maximum_detection_range;
  k.valid_points = cfg->segment_valid_point_num;
  k.valid_lines = cfg->segment_valid_line_num;
  k.mount = cfg->sensor_mount_angle;
  k.ground_limit = 10 * kDegToRad;
  {
    // tf2::Quaternion::setRPY(0, mount, 0) = (0, sin(mount / 2), 0, cos(mount / 2)), through transformToEigen
    const double q[7] = {0, 0, 0, 0, std::sin(cfg->sensor_mount_angle * 0.5), 0, std::cos(cfg->sensor_mount_angle * 0.5)};
    quat_to_rot(q, k.Rp);
  }
  if (!(k.res_y > 0.f) || !std::isfinite(k.max_range))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: the vertical resolution or the maximum range does not fit a float", what);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if ((rc = source_refused(ctx, what, SourceOp::kConfigureSweep, source_id)) != DDDMR_OK) return rc;
  bool had_points;
  if ((rc = configure_begin(ctx, source_id, &had_points)) != DDDMR_OK) return rc;   // (which turns the features off)
  auto sw = std::make_unique<LidarSweep>();
  sw->p = k;
  sw->max_points = cfg->max_sweep_points;
  if (sweep_alloc(*sw) != 0) {
    rc = fail(ctx, DDDMR_ERR_HIP, "%s: scratch of source %d", what, source_id);
  } else {
    ctx->src[source_id].obs = sw->obs[sw->cur];
    ctx->sources.configure(source_id, SourceKind::kSweep);
    ctx->src[source_id].sweep = std::move(sw);
  }
  return configure_end(ctx, what, source_id, had_points, rc);
}

int dddmr_rollout_set_lidar_sweep(dddmr_rollout_ctx* ctx, int32_t source_id, const float* xyz, size_t n_points, size_t stride_bytes,
                                  const double T_base_sensor[7], const double T_gbl_base[7], double perception_window_size,
                                  double marking_height, uint32_t* n_segmented, uint32_t* n_source_points, uint32_t* n_aggregate_points) {
  if (!ctx || !T_base_sensor || !T_gbl_base) return DDDMR_ERR_BAD_ARG;
  if (const int arc = source_arg(ctx, "set_lidar_sweep", source_id)) return arc;
  if (!cloud_arg_ok(xyz, n_points, stride_bytes)) return fail(ctx, DDDMR_ERR_BAD_ARG, "set_lidar_sweep: bad pointer/stride");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  int rc = source_refused(ctx, "set_lidar_sweep", SourceOp::kFeedSweep, source_id);
  if (rc != DDDMR_OK) return rc;
  LidarSweep* sw = ctx->src[source_id].sweep.get();
  if (n_points > sw->max_points) return fail(ctx, DDDMR_ERR_CAPACITY, "set_lidar_sweep: %zu points > max_sweep_points %u", n_points, sw->max_points);
  FeedParams fp;
  set_mounts(fp, T_base_sensor, T_gbl_base);
  fp.n = 0;                                            // the device knows the count
  fp.window = (float)perception_window_size;
  fp.height = (float)marking_height;
  uint32_t n_seg = 0, n_out = 0;
  rc = sweep_feed(*sw, fp, xyz, n_points, stride_bytes, ctx->copy_stream, &n_seg, &n_out);
  if (rc != 0) return fail(ctx, DDDMR_ERR_HIP, "set_lidar_sweep: sweep feed failed (%d)", rc);
  FeatResult feat_counts{};
  if (sw->features) std::memcpy(&feat_counts, sw->features->res_host, sizeof(feat_counts));   // written before the feed's release
  AssocResult assoc_res{};
  if (sw->features && sw->features->assoc) std::memcpy(&assoc_res, sw->features->assoc->res_host, sizeof(assoc_res));
  uint32_t n_all = 0;
  if ((rc = commit_source(ctx, "set_lidar_sweep", source_id, sw->obs[sw->cur ^ 1], n_out, &n_all)) != DDDMR_OK) return rc;
  sw->cur ^= 1;                                        // committed: the buffers the sweep was built in become the current ones
  sw->n_cloud = n_seg;
  sw->have_sweep = true;
  if (LidarFeatures* lf = sw->features.get()) {        // the features were built beside the sweep: they are current with it
    lf->n_seg[sw->cur] = feat_counts.n_seg;
    for (int w = 0; w < 3; ++w) lf->n_feat[sw->cur][w] = feat_counts.n_feat[w];
    lf->have_sweep = true;
    if (SweepAssoc* a = lf->assoc.get()) {
      a->n_less_flat[sw->cur] = assoc_res.n_less_flat;
      a->n_outliers[sw->cur] = assoc_res.n_outliers;
      a->half_index[sw->cur] = assoc_res.i0;
      a->have[sw->cur] = true;
      for (int w = 0; w < 3; ++w) a->orientation[sw->cur][w] = assoc_res.orient[w];
    }
  }
  if (n_segmented) *n_segmented = n_seg;
  if (n_source_points) *n_source_points = n_out;
  if (n_aggregate_points) *n_aggregate_points = n_all;
  return DDDMR_OK;
}

int dddmr_rollout_get_lidar_sweep_cloud(dddmr_rollout_ctx* ctx, int32_t source_id, float* xyzl_out, size_t capacity, size_t* n_points) {
  if (!ctx || !n_points) return DDDMR_ERR_BAD_ARG;
  if (const int arc = source_arg(ctx, "get_lidar_sweep_cloud", source_id)) return arc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if (const int rc = source_refused(ctx, "get_lidar_sweep_cloud", SourceOp::kSweepGetter, source_id)) return rc;
  const LidarSweep* sw = ctx->src[source_id].sweep.get();
  return read_back(ctx, "get_lidar_sweep_cloud", xyzl_out, sw->cloud[sw->cur], sw->n_cloud, sizeof(float4), capacity, n_points);
}

int dddmr_rollout_get_lidar_sweep_image(dddmr_rollout_ctx* ctx, int32_t source_id, float* range_out, int32_t* label_out, int8_t* ground_out,
                                        size_t capacity_pixels) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (const int arc = source_arg(ctx, "get_lidar_sweep_image", source_id)) return arc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if (const int rc = source_refused(ctx, "get_lidar_sweep_image", SourceOp::kSweepGetter, source_id)) return rc;
  const LidarSweep* sw = ctx->src[source_id].sweep.get();
  const size_t px = (size_t)sw->p.V * sw->p.H;
  if (capacity_pixels < px) return fail(ctx, DDDMR_ERR_CAPACITY, "get_lidar_sweep_image: capacity %zu < %zu pixels", capacity_pixels, px);
  if (!sw->have_sweep) {                               // resetParameters' image: nothing projected yet
    for (size_t i = 0; i < px; ++i) {
      if (range_out) range_out[i] = FLT_MAX;
      if (label_out) label_out[i] = -1;
      if (ground_out) ground_out[i] = 0;
    }
    return DDDMR_OK;
  }
  Drain drain{ctx->copy_stream};                       // an error exit leaves no copy behind that writes the caller's memory
  if (range_out) HIPCHK(ctx, hipMemcpyAsync(range_out, sw->range_img[sw->cur], px * sizeof(float), hipMemcpyDeviceToHost, ctx->copy_stream));
  if (label_out) HIPCHK(ctx, hipMemcpyAsync(label_out, sw->label_img[sw->cur], px * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->copy_stream));
  if (ground_out) HIPCHK(ctx, hipMemcpyAsync(ground_out, sw->ground_img[sw->cur], px, hipMemcpyDeviceToHost, ctx->copy_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  drain.armed = false;
  return DDDMR_OK;
}

// ---------------------------------------------------------------------------
// Lidar sweep features: the feature half of mcl_feature_node on a sweep source (lidar_features.hip.h)
// ---------------------------------------------------------------------------
int dddmr_rollout_set_lidar_sweep_features(dddmr_rollout_ctx* ctx, int32_t source_id, const dddmr_lidar_features_config* cfg) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "set_lidar_sweep_features";
  if (const int arc = source_arg(ctx, what, source_id)) return arc;
  if (cfg) {
    if (!std::isfinite(cfg->edge_threshold) || !std::isfinite(cfg->surf_threshold) || cfg->edge_threshold < 0.0 || cfg->surf_threshold < 0.0 ||
        cfg->flags != 0)
      return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: thresholds %g / %g, flags %#x", what, cfg->edge_threshold, cfg->surf_threshold, cfg->flags);
    for (int i = 0; i < 12; ++i)
      if (!std::isfinite(cfg->T_out[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: T_out[%d] is not finite", what, i);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if (const int rc = source_refused(ctx, what, SourceOp::kSweepGetter, source_id)) return rc;
  LidarSweep* sw = ctx->src[source_id].sweep.get();
  FeatParams k{};
  if (cfg) {
    k.edge_threshold = (float)cfg->edge_threshold;     // float members (featureAssociation.h:62-63)
    k.surf_threshold = (float)cfg->surf_threshold;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) k.R[3 * r + c] = cfg->T_out[4 * r + c];
      k.t[r] = cfg->T_out[4 * r + 3];
    }
    k.V = sw->p.V;
    k.H = sw->p.H;
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  if (!cfg) {
    sw->features.reset();
    return DDDMR_OK;
  }
  if (sw->features) {                                  // new parameters: they hold from the next sweep on; what the getters
    sw->features->p = k;                               // return stays the latest accepted sweep's
    return DDDMR_OK;
  }
  auto lf = std::make_unique<LidarFeatures>();
  lf->p = k;
  if (features_alloc(*lf) != 0) return fail(ctx, DDDMR_ERR_HIP, "%s: scratch of source %d", what, source_id);
  sw->features.reset(lf.release());
  return DDDMR_OK;
}

static int sweep_features_of(dddmr_rollout_ctx* ctx, int32_t source_id, const char* what, LidarSweep** out) {
  if (const int arc = source_arg(ctx, what, source_id)) return arc;
  if (const int rc = source_refused(ctx, what, SourceOp::kSweepGetter, source_id)) return rc;
  LidarSweep* sw = ctx->src[source_id].sweep.get();
  if (!sw->features) return fail(ctx, DDDMR_ERR_STATE, "%s: the features of source %d are off", what, source_id);
  *out = sw;
  return DDDMR_OK;
}

int dddmr_rollout_get_lidar_sweep_segmented(dddmr_rollout_ctx* ctx, int32_t source_id, float* xyz, float* range, int32_t* col_ind,
                                            uint8_t* ground_flag, int32_t* start_ring_index, int32_t* end_ring_index, size_t capacity,
                                            size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  LidarSweep* sw = nullptr;
  const int rc = sweep_features_of(ctx, source_id, "get_lidar_sweep_segmented", &sw);
  if (rc != DDDMR_OK) return rc;
  const LidarFeatures& lf = *sw->features;
  const int b = sw->cur;
  const size_t count = lf.n_seg[b], V = sw->p.V;
  const bool points = xyz || range || col_ind || ground_flag;
  if (points && capacity < count) return fail(ctx, DDDMR_ERR_CAPACITY, "get_lidar_sweep_segmented: capacity %zu < %zu", capacity, count);
  *n = count;
  std::vector<float4> pt;
  std::vector<uint32_t> cr;
  std::vector<int32_t> ring(2 * V);
  Drain drain{ctx->copy_stream};                       // declared behind the vectors: an error exit waits before they die
  if (points && count) {
    pt.resize(count);
    cr.resize(count);
    HIPCHK(ctx, hipMemcpyAsync(pt.data(), lf.seg_pt[b], count * sizeof(float4), hipMemcpyDeviceToHost, ctx->copy_stream));
    HIPCHK(ctx, hipMemcpyAsync(cr.data(), lf.seg_cr[b], count * 4, hipMemcpyDeviceToHost, ctx->copy_stream));
  }
  if (start_ring_index || end_ring_index)
    HIPCHK(ctx, hipMemcpyAsync(ring.data(), lf.ring[b], 2 * V * 4, hipMemcpyDeviceToHost, ctx->copy_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  drain.armed = false;
  for (size_t i = 0; i < pt.size(); ++i) {
    if (xyz) { xyz[3 * i] = pt[i].x; xyz[3 * i + 1] = pt[i].y; xyz[3 * i + 2] = pt[i].z; }
    if (range) range[i] = pt[i].w;
    if (col_ind) col_ind[i] = (int32_t)(cr[i] & 0xFFFFu);
    if (ground_flag) ground_flag[i] = (uint8_t)(cr[i] >> 31);
  }
  for (size_t r = 0; r < V; ++r) {                     // before the first sweep: the indices of an empty cloud
    const bool have = lf.have_sweep;
    if (start_ring_index) start_ring_index[r] = have ? ring[r] : 4;
    if (end_ring_index) end_ring_index[r] = have ? ring[V + r] : -6;
  }
  return DDDMR_OK;
}

int dddmr_rollout_get_lidar_sweep_features(dddmr_rollout_ctx* ctx, int32_t source_id, int which, float* xyzr_out, uint32_t* seg_index_out,
                                           size_t capacity, size_t* n_points) {
  if (!ctx || !n_points) return DDDMR_ERR_BAD_ARG;
  if (which < 0 || which > 2) return fail(ctx, DDDMR_ERR_BAD_ARG, "get_lidar_sweep_features: which %d (0 sharp, 1 less sharp, 2 flat)", which);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  LidarSweep* sw = nullptr;
  const int rc = sweep_features_of(ctx, source_id, "get_lidar_sweep_features", &sw);
  if (rc != DDDMR_OK) return rc;
  const LidarFeatures& lf = *sw->features;
  const int b = sw->cur;
  const size_t count = lf.n_feat[b][which], off = feat_offset(sw->p.V, which);
  if ((xyzr_out || seg_index_out) && capacity < count)
    return fail(ctx, DDDMR_ERR_CAPACITY, "get_lidar_sweep_features: capacity %zu < %zu", capacity, count);
  *n_points = count;
  Drain drain{ctx->copy_stream};
  if (count && xyzr_out) HIPCHK(ctx, hipMemcpyAsync(xyzr_out, lf.feat[b] + off, count * sizeof(float4), hipMemcpyDeviceToHost, ctx->copy_stream));
  if (count && seg_index_out) HIPCHK(ctx, hipMemcpyAsync(seg_index_out, lf.feat_idx[b] + off, count * 4, hipMemcpyDeviceToHost, ctx->copy_stream));
  if (count && (xyzr_out || seg_index_out)) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  drain.armed = false;
  return DDDMR_OK;
}

// ---------------------------------------------------------------------------
// Lidar sweep association: the rest of the feature node's front half (sweep_association.hip.h)
// ---------------------------------------------------------------------------
int dddmr_rollout_set_lidar_sweep_association(dddmr_rollout_ctx* ctx, int32_t source_id, int32_t enable, double scan_period) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  const char* what = "set_lidar_sweep_association";
  if (const int arc = source_arg(ctx, what, source_id)) return arc;
  if (enable && (!std::isfinite(scan_period) || scan_period < 0.0)) return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: scan_period %g", what, scan_period);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  LidarSweep* sw = nullptr;
  if (const int rc = sweep_features_of(ctx, source_id, what, &sw)) return rc;
  LidarFeatures& lf = *sw->features;
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  if (!enable) {
    lf.assoc.reset();
    return DDDMR_OK;
  }
  if (lf.assoc) {                                      // a new period holds from the next sweep on
    lf.assoc->scan_period = scan_period;
    return DDDMR_OK;
  }
  auto a = std::make_unique<SweepAssoc>();
  a->scan_period = scan_period;
  if (association_alloc(*a, sw->p.V, sw->p.H) != 0) return fail(ctx, DDDMR_ERR_HIP, "%s: scratch of source %d", what, source_id);
  lf.assoc.reset(a.release());
  return DDDMR_OK;
}

static int sweep_association_of(dddmr_rollout_ctx* ctx, int32_t source_id, const char* what, LidarSweep** out) {
  if (const int rc = sweep_features_of(ctx, source_id, what, out)) return rc;
  if (!(*out)->features->assoc) return fail(ctx, DDDMR_ERR_STATE, "%s: the association of source %d is off", what, source_id);
  return DDDMR_OK;
}

int dddmr_rollout_get_lidar_sweep_orientation(dddmr_rollout_ctx* ctx, int32_t source_id, float out[3], int32_t* half_index) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  LidarSweep* sw = nullptr;
  if (const int rc = sweep_association_of(ctx, source_id, "get_lidar_sweep_orientation", &sw)) return rc;
  const SweepAssoc& a = *sw->features->assoc;
  for (int w = 0; w < 3 && out; ++w) out[w] = a.orientation[sw->cur][w];
  if (half_index) *half_index = (int32_t)a.half_index[sw->cur];
  return DDDMR_OK;
}

// the tail of the association's getters: `count` records of the device arrays into the caller's, either of which may be null
static int association_read(dddmr_rollout_ctx* ctx, const char* what, const void* rec, float* rec_out, const uint32_t* idx, uint32_t* idx_out,
                            size_t count, size_t rec_bytes, size_t capacity, size_t* n) {
  if ((rec_out || idx_out) && capacity < count) return fail(ctx, DDDMR_ERR_CAPACITY, "%s: capacity %zu < %zu", what, capacity, count);
  *n = count;
  Drain drain{ctx->copy_stream};
  if (count && rec_out) HIPCHK(ctx, hipMemcpyAsync(rec_out, rec, count * rec_bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
  if (count && idx_out) HIPCHK(ctx, hipMemcpyAsync(idx_out, idx, count * 4, hipMemcpyDeviceToHost, ctx->copy_stream));
  if (count && (rec_out || idx_out)) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  drain.armed = false;
  return DDDMR_OK;
}

int dddmr_rollout_get_lidar_sweep_times(dddmr_rollout_ctx* ctx, int32_t source_id, float* intensity_out, size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  LidarSweep* sw = nullptr;
  if (const int rc = sweep_association_of(ctx, source_id, "get_lidar_sweep_times", &sw)) return rc;
  const LidarFeatures& lf = *sw->features;
  const int b = sw->cur;
  const size_t count = lf.assoc->have[b] ? lf.n_seg[b] : 0;      // (the current sweep may be older than the association)
  return association_read(ctx, "get_lidar_sweep_times", lf.assoc->times[b], intensity_out, nullptr, nullptr, count, sizeof(float), capacity, n);
}

int dddmr_rollout_get_lidar_sweep_association(dddmr_rollout_ctx* ctx, int32_t source_id, int which, int frame, float* xyzi_out,
                                              uint32_t* seg_index_out, size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  const char* what = "get_lidar_sweep_association";
  if (which < 0 || which > 3 || frame < 0 || frame > 1)
    return fail(ctx, DDDMR_ERR_BAD_ARG, "%s: which %d (0 sharp, 1 less sharp, 2 flat, 3 less flat), frame %d (0 association, 1 through T_out)", what,
                which, frame);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  LidarSweep* sw = nullptr;
  if (const int rc = sweep_association_of(ctx, source_id, what, &sw)) return rc;
  const LidarFeatures& lf = *sw->features;
  const SweepAssoc& a = *lf.assoc;
  const int b = sw->cur;
  if (which == 3) return association_read(ctx, what, a.less_flat[b][frame], xyzi_out, a.less_flat_idx[b], seg_index_out, a.n_less_flat[b], sizeof(float4), capacity, n);
  const size_t off = feat_offset(sw->p.V, which);
  return association_read(ctx, what, a.list[b][frame] + off, xyzi_out, lf.feat_idx[b] + off, seg_index_out, a.have[b] ? lf.n_feat[b][which] : 0, sizeof(float4),
                          capacity, n);
}

int dddmr_rollout_get_lidar_sweep_outliers(dddmr_rollout_ctx* ctx, int32_t source_id, float* xyzi_out, size_t capacity, size_t* n) {
  if (!ctx || !n) return DDDMR_ERR_BAD_ARG;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  LidarSweep* sw = nullptr;
  if (const int rc = sweep_association_of(ctx, source_id, "get_lidar_sweep_outliers", &sw)) return rc;
  const SweepAssoc& a = *sw->features->assoc;
  return association_read(ctx, "get_lidar_sweep_outliers", a.outliers[sw->cur], xyzi_out, nullptr, nullptr, a.n_outliers[sw->cur], sizeof(float4), capacity, n);
}

// ---------------------------------------------------------------------------
// Depth camera frustums, point tests and selfClear's clearing verdicts (depth_clear.hip.h)
// ---------------------------------------------------------------------------
int dddmr_rollout_set_depth_frustum(dddmr_rollout_ctx* ctx, int32_t source_id, const dddmr_depth_frustum_config* cfg,
                                    const double T_gbl_sensor[7]) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (const int arc = source_arg(ctx, "set_depth_frustum", source_id, " / null argument", cfg && T_gbl_sensor)) return arc;
  const double kPi = 3.14159265358979323846;
  if (!(cfg->FOV_W > 0.0 && cfg->FOV_W < kPi) || !(cfg->FOV_V > 0.0 && cfg->FOV_V < kPi) || !(cfg->obstacle_min_range > 0.0) ||
      !(cfg->obstacle_max_range > cfg->obstacle_min_range) || !std::isfinite(cfg->obstacle_max_range))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "set_depth_frustum: FOV %g x %g rad, range %g .. %g m", cfg->FOV_W, cfg->FOV_V, cfg->obstacle_min_range,
                cfg->obstacle_max_range);
  for (int i = 0; i < 7; ++i)
    if (!std::isfinite(T_gbl_sensor[i])) return fail(ctx, DDDMR_ERR_BAD_ARG, "set_depth_frustum: non-finite transform");
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if (const int rc = source_refused(ctx, "set_depth_frustum", SourceOp::kSetFrustum, source_id)) return rc;
  double R[9];
  quat_to_rot(T_gbl_sensor, R);
  frustum_build(ctx->src[source_id].frustum, cfg->FOV_W, cfg->FOV_V, cfg->obstacle_min_range, cfg->obstacle_max_range, R, T_gbl_sensor);
  ctx->sources.set_frustum(source_id);
  return DDDMR_OK;
}

int dddmr_rollout_get_depth_frustum(dddmr_rollout_ctx* ctx, int32_t source_id, float vertices[8][3], float normals[6][3],
                                    float planes[6][4], float origin[3]) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (const int arc = source_arg(ctx, "get_depth_frustum", source_id)) return arc;
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  if (const int rc = source_refused(ctx, "get_depth_frustum", SourceOp::kGetFrustum, source_id)) return rc;
  const DcFrustum& F = ctx->src[source_id].frustum;
  if (vertices) std::memcpy(vertices, F.vtx, sizeof(F.vtx));
  if (normals) std::memcpy(normals, F.nrm, sizeof(F.nrm));
  if (planes) std::memcpy(planes, F.pl, sizeof(F.pl));
  if (origin)
    for (int a = 0; a < 3; ++a) origin[a] = (float)F.origin[a];
  return DDDMR_OK;
}

// The frustums of all depth sources in source order; every depth source must have one.  producer_mu held.
static int depth_frustums(dddmr_rollout_ctx* ctx, const char* what, DcFrustums* S) {
  const SourceTable& table = ctx->sources;
  const int missing = table.first_depth_without_frustum();
  if (missing >= 0) return fail(ctx, DDDMR_ERR_STATE, "%s: depth source %d has no frustum yet", what, missing);
  if (!table.any_depth()) return fail(ctx, DDDMR_ERR_STATE, "%s: the context has no depth camera source", what);
  S->n = 0;
  for (int i = 0; i < SourceTable::kMax; ++i)
    if (is_depth(table.rec[i].kind)) S->f[S->n++] = ctx->src[i].frustum;
  return DDDMR_OK;
}

static int depth_clear_scratch(dddmr_rollout_ctx* ctx, const char* what) {
  if (ctx->dclear) return DDDMR_OK;
  size_t temp_bytes = 0;                               // of the grid builder's scan: rocPRIM asks the device
  uint32_t* cells = nullptr;
  auto d = std::make_unique<DepthClear>();
  if (rocprim::exclusive_scan(nullptr, temp_bytes, cells, cells, 0u, (size_t)kDcCapCells + 1, rocprim::plus<uint32_t>(), nullptr) != hipSuccess ||
      dc_alloc(*d, ctx->cfg.max_points, temp_bytes) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "%s: scratch allocation failed", what);
  ctx->dclear = std::move(d);
  return DDDMR_OK;
}

// The grid over the depth sources' observation (n_obs points in all), rebuilt only when a depth source has published
// since it was last built: the clearing verdicts and selfMark's clusters share it.  producer_mu held.
static int depth_observation_grid(dddmr_rollout_ctx* ctx, DepthClear& d, size_t n_obs, hipStream_t st, uint32_t* ops) {
  if (d.built && d.built_epoch == ctx->sources.depth_epoch) return DDDMR_OK;
  size_t at = 0;
  Drain drain{st};                                     // an error exit leaves no half-built grid running
  for (int i = 0; i < dddmr_rollout_ctx::kMaxSources; ++i) {
    const SourceRecord& r = ctx->sources.rec[i];
    if (!is_depth(r.kind) || !r.n) continue;
    HIPCHK(ctx, hipMemcpyAsync(d.pts + at, ctx->src[i].obs, (size_t)r.n * sizeof(float4), hipMemcpyDeviceToDevice, st));
    at += r.n;
    ++*ops;
  }
  d.built = false;
  const int b = dc_build_grid(d, (uint32_t)n_obs, st);
  if (b < 0) return fail(ctx, DDDMR_ERR_HIP, "depth observation grid: build failed");
  *ops += (uint32_t)b;
  drain.armed = false;                                 // (the caller's one wait follows its own launches)
  d.built = true;
  d.built_epoch = ctx->sources.depth_epoch;
  return DDDMR_OK;
}

int dddmr_rollout_depth_frustum_test(dddmr_rollout_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes,
                                     uint8_t* in_frustums_out, uint8_t* attach_out) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!cloud_arg_ok(xyz, n, stride_bytes)) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_frustum_test: bad pointer/stride");
  if (n > (1u << 28)) return fail(ctx, DDDMR_ERR_CAPACITY, "depth_frustum_test: %zu points", n);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DcFrustums S;
  int rc = depth_frustums(ctx, "depth_frustum_test", &S);
  if (rc != DDDMR_OK) return rc;
  if (n == 0) return DDDMR_OK;
  if ((rc = depth_clear_scratch(ctx, "depth_frustum_test")) != DDDMR_OK) return rc;
  DepthClear& d = *ctx->dclear;
  if (host_mapped_reserve(d.mem.host, &d.in_host, &d.in_dev, &d.in_cap, n * 12) != 0 ||
      host_mapped_reserve(d.mem.host, &d.out_host, &d.out_dev, &d.out_cap, n) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "depth_frustum_test: staging for %zu points", n);
  float* st = static_cast<float*>(d.in_host);
  if (stride_bytes == 12) {
    std::memcpy(st, xyz, n * 12);
  } else {
    const size_t sf = stride_bytes / 4;
    for (size_t i = 0; i < n; ++i) {
      st[3 * i + 0] = xyz[i * sf + 0];
      st[3 * i + 1] = xyz[i * sf + 1];
      st[3 * i + 2] = xyz[i * sf + 2];
    }
  }
  hipLaunchKernelGGL(k_dc_frustum_test, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->copy_stream, S,
                     static_cast<const float*>(d.in_dev), (uint32_t)n, static_cast<uint8_t*>(d.out_dev));
  Drain drain{ctx->copy_stream};
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  drain.armed = false;
  const uint8_t* o = static_cast<const uint8_t*>(d.out_host);
  for (size_t i = 0; i < n; ++i) {
    if (in_frustums_out) in_frustums_out[i] = o[i] & 1u;
    if (attach_out) attach_out[i] = (o[i] >> 1) & 1u;
  }
  return DDDMR_OK;
}

int dddmr_rollout_depth_clear_verdicts(dddmr_rollout_ctx* ctx, double xy_resolution, double height_resolution,
                                       const int32_t* voxel_xyz, const uint32_t* offsets, const float* cluster_xyz, size_t m,
                                       uint8_t* verdict_out, uint32_t* engaged_out) {
  if (!ctx) return DDDMR_ERR_BAD_ARG;
  if (!(xy_resolution > 0.0) || !(height_resolution > 0.0) || !std::isfinite(xy_resolution) || !std::isfinite(height_resolution))
    return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_clear_verdicts: resolutions %g / %g", xy_resolution, height_resolution);
  if (m > 0 && (!voxel_xyz || !offsets || !verdict_out)) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_clear_verdicts: null argument");
  if (m > (1u << 24)) return fail(ctx, DDDMR_ERR_CAPACITY, "depth_clear_verdicts: %zu markings", m);
  if (m > 0) {
    if (offsets[0] != 0) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_clear_verdicts: offsets[0] = %u", offsets[0]);
    for (size_t i = 0; i < m; ++i)
      if (offsets[i + 1] < offsets[i]) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_clear_verdicts: offsets decrease at marking %zu", i);
    if (offsets[m] > 0 && !cluster_xyz) return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_clear_verdicts: null cluster points");
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  DcFrustums S;
  int rc = depth_frustums(ctx, "depth_clear_verdicts", &S);
  if (rc != DDDMR_OK) return rc;
  if (m == 0) return DDDMR_OK;
  if ((rc = depth_clear_scratch(ctx, "depth_clear_verdicts")) != DDDMR_OK) return rc;
  DepthClear& d = *ctx->dclear;
  hipStream_t st = ctx->copy_stream;      // the stream the depth feeds ran on: their frames are complete before this work
  uint32_t ops = 0;
  // aggregatePointCloudFromObservations: the depth sources' alive frames, in source order (lidar sources stay out)
  const size_t n_obs = ctx->sources.depth_points();
  const bool observation_clear = !(n_obs > 5);       // depth_camera_layer.cpp:258-264
  Drain drain{st};                                   // from the grid's launches on: an error exit below waits for them
  if (!observation_clear && (rc = depth_observation_grid(ctx, d, n_obs, st, &ops)) != DDDMR_OK) return rc;
  const size_t total = offsets[m];
  const size_t vox_bytes = m * 3 * sizeof(int32_t), off_bytes = (m + 1) * sizeof(uint32_t);
  if (host_mapped_reserve(d.mem.host, &d.in_host, &d.in_dev, &d.in_cap, vox_bytes + off_bytes + total * 12) != 0 ||
      host_mapped_reserve(d.mem.host, &d.out_host, &d.out_dev, &d.out_cap, m * sizeof(uint2)) != 0)
    return fail(ctx, DDDMR_ERR_HIP, "depth_clear_verdicts: staging for %zu markings, %zu cluster points", m, total);
  char* in = static_cast<char*>(d.in_host);
  std::memcpy(in, voxel_xyz, vox_bytes);
  std::memcpy(in + vox_bytes, offsets, off_bytes);
  if (total) std::memcpy(in + vox_bytes + off_bytes, cluster_xyz, total * 12);
  const char* dev = static_cast<const char*>(d.in_dev);
  DcVerdictParams k;
  k.res = xy_resolution;
  k.hres = height_resolution;
  k.m = (uint32_t)m;
  k.observation_clear = observation_clear ? 1u : 0u;
  hipLaunchKernelGGL(k_dc_verdicts, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, k, S, d.hdr, reinterpret_cast<const int32_t*>(dev),
                     reinterpret_cast<const uint32_t*>(dev + vox_bytes), reinterpret_cast<const float*>(dev + vox_bytes + off_bytes),
                     static_cast<uint2*>(d.out_dev));
  ++ops;
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));           // the call's one host wait
  drain.armed = false;
  d.launches_last = ops;
  const uint2* o = static_cast<const uint2*>(d.out_host);
  for (size_t i = 0; i < m; ++i)
    if (o[i].x & kDcEmptyCluster)
      return fail(ctx, DDDMR_ERR_BAD_ARG, "depth_clear_verdicts: marking %zu reaches the engagement ratio with an empty cluster", i);
  for (size_t i = 0; i < m; ++i) {
    verdict_out[i] = (uint8_t)o[i].x;
    if (engaged_out) engaged_out[i] = o[i].y;
  }
  return DDDMR_OK;
}

int dddmr_rollout_depth_clear_launches(dddmr_rollout_ctx* ctx, uint32_t* launches_last_call) {
  if (!ctx || !launches_last_call) return DDDMR_ERR_BAD_ARG;
  std::lock_guard<std::mutex> prod(ctx->producer_mu);
  *launches_last_call = ctx->dclear ? ctx->dclear->launches_last : 0u;
  return DDDMR_OK;
}

}  // extern "C"
