// source_table.hip.h -- what the context knows about its sensor sources, as arithmetic alone: one record per source id
// (what kind of source it is, how many points its current observation has, the few flags the rules need), the rules
// that decide whether a call is refused because of the kind a source already has, the fit of a candidate observation
// beside the others, the layout of the aggregate and the queries over the depth sources.  Host code only -- no HIP call,
// no HIP type, no context -- so that tests/cpp/source_table_test.cpp builds it with a plain host compiler.
//
// The owning pointers of a source (its scratch, its buffers, its frustum) live beside the table in the context
// (SourceOwned in rollout_engine.hip); sensor_sources.hip.h keeps the two in step under producer_mu.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/dddmr_rollout.h"

namespace dddmr {

enum class SourceKind : uint8_t { kNone, kScan, kDepthCloud, kDepthImage, kSweep };

// the calls whose outcome depends on the kind a source already has
enum class SourceOp : uint8_t {
  kConfigureDepth,    // set_depth_source, set_depth_image_source
  kConfigureSweep,    // set_lidar_sweep_source
  kFeedScan,          // set_scan, set_scan_source
  kFeedFrame,         // set_depth_frame
  kFeedImage,         // set_depth_image
  kFeedSweep,         // set_lidar_sweep
  kSetStitcher,       // set_stitcher, set_stitcher_source
  kSetFrustum,        // set_depth_frustum
  kGetFrustum,        // get_depth_frustum
  kSweepGetter,       // get_lidar_sweep_cloud / _image, set_lidar_sweep_features and the feature getters
  kImageCloudGetter,  // get_depth_image_cloud
};

// code DDDMR_OK: accepted.  Otherwise the call fails with code and the message "<call>: source <id> <why>".
struct Refusal {
  int code;
  const char* why;
};

struct SourceRecord {
  SourceKind kind = SourceKind::kNone;
  uint32_t n = 0;            // points of the current observation
  bool scan_fed = false;     // a scan has been fed under this id (it stays set when that feed fails)
  bool stitcher = false;     // source 0: its stitcher count is above 0; a source above 0: it has had a set_stitcher_source
  bool has_frustum = false;  // depth sources: set_depth_frustum since the source was configured
};

// Where the sources' observations lie in an aggregate: publish_cloud records one per cloud buffer, stack_update cuts the
// lidar runs out of a pinned aggregate with it.
struct SourceLayout {
  uint32_t n[DDDMR_MAX_SOURCES] = {};
  uint32_t at[DDDMR_MAX_SOURCES] = {};   // offset of source i's points: the sum of n[0 .. i)
  uint32_t total = 0;
  uint8_t lidar_mask = 0;                // bit i: source i's points are a lidar's
  bool from_sources = true;              // false: a cloud handed over with set_cloud, nothing above holds
};

inline bool is_depth(SourceKind k) { return k == SourceKind::kDepthCloud || k == SourceKind::kDepthImage; }

// the aggregate of the single-producer set_scan: all of it is the lidar of source 0
inline SourceLayout single_lidar_layout(uint32_t n) {
  SourceLayout L;
  L.n[0] = L.total = n;
  L.lidar_mask = 1;
  return L;
}
inline SourceLayout foreign_layout() {
  SourceLayout L;
  L.from_sources = false;
  return L;
}

struct SourceTable {
  static constexpr int kMax = DDDMR_MAX_SOURCES;
  SourceRecord rec[kMax];
  bool multi_source = false;     // a per-source call has been made: plain set_scan then means source 0
  uint64_t depth_epoch = 1;      // bumped whenever a depth source's observation changes

  static bool valid(int id) { return id >= 0 && id < kMax; }

  // ---- kind refusals ----
  Refusal refuse(SourceOp op, int id) const {
    const SourceRecord& r = rec[id];
    const bool depth = is_depth(r.kind), sweep = r.kind == SourceKind::kSweep, scan = r.kind == SourceKind::kScan;
    const int bad = DDDMR_ERR_BAD_ARG, state = DDDMR_ERR_STATE;
    switch (op) {
      case SourceOp::kConfigureDepth:      // a configured depth source is configured again (which empties it)
        if (scan || sweep) return {bad, "is a lidar source"};
        break;
      case SourceOp::kConfigureSweep:      // likewise a sweep source
        if (depth) return {bad, "is a depth camera source"};
        if (scan) return {bad, "is a scan source"};
        break;
      case SourceOp::kFeedScan:
        if (depth) return {bad, "is a depth camera source"};
        if (sweep) return {bad, "is a lidar sweep source"};
        break;
      case SourceOp::kFeedFrame:
        if (!depth) return {bad, "is not a configured depth source"};
        if (r.kind == SourceKind::kDepthImage) return {bad, "is configured for depth images"};
        break;
      case SourceOp::kFeedImage:
        if (!depth) return {bad, "is not a configured depth source"};
        if (r.kind == SourceKind::kDepthCloud) return {bad, "is configured for point clouds"};
        break;
      case SourceOp::kFeedSweep:
        if (!sweep) return {bad, "is not a configured lidar sweep source"};
        break;
      case SourceOp::kSetStitcher:
        if (depth) return {bad, "is a depth camera source"};
        if (sweep) return {bad, "is a lidar sweep source (no stitcher on sweeps)"};
        break;
      case SourceOp::kSetFrustum:
        if (!depth) return {state, "is not a depth camera source"};
        break;
      case SourceOp::kGetFrustum:
        if (!depth || !r.has_frustum) return {state, "has no frustum"};
        break;
      case SourceOp::kSweepGetter:
        if (!sweep) return {state, "is not a lidar sweep source"};
        break;
      case SourceOp::kImageCloudGetter:
        if (r.kind != SourceKind::kDepthImage) return {bad, "is not a depth image source"};
        break;
    }
    return {DDDMR_OK, ""};
  }

  // ---- scan sources: they are never configured, they become one by being used ----
  // the source a scan call means: plain set_scan (source < 0) is source 0 once a per-source call has been made
  int scan_source(int source) const { return source < 0 && multi_source ? 0 : source; }
  // A scan is about to be fed (source as scan_source() gave it; below 0: the single-producer form, the lidar of source 0).
  // Not undone when the feed fails.
  void note_scan(int source) {
    if (source >= 0) multi_source = true;
    SourceRecord& r = rec[source < 0 ? 0 : source];
    r.scan_fed = true;
    r.kind = SourceKind::kScan;
  }
  // set_stitcher / set_stitcher_source was accepted.  Source 0 counts as a scan source while its stitcher count is above
  // 0, even before any scan; a source above 0 from its first such call on, whatever the count.
  void note_stitcher(int id, int stitcher_num) {
    SourceRecord& r = rec[id];
    r.stitcher = id > 0 || stitcher_num > 0;
    r.kind = r.scan_fed || r.stitcher ? SourceKind::kScan : SourceKind::kNone;
  }

  // ---- configured sources ----
  void configure(int id, SourceKind kind) {          // on a released (or never used) id
    rec[id] = SourceRecord{};
    rec[id].kind = kind;
    multi_source = true;
  }
  void release(int id) {                             // its observation and its frustum leave with it
    if (is_depth(rec[id].kind)) ++depth_epoch;
    rec[id] = SourceRecord{};
  }
  void set_frustum(int id) { rec[id].has_frustum = true; }
  void set_count(int id, uint32_t n) {               // a new observation of the source
    rec[id].n = n;
    if (is_depth(rec[id].kind)) ++depth_epoch;
  }

  // ---- candidate fit ----
  // *total: the aggregate's size with source id's count replaced by candidate_n.  The table is not touched.
  bool would_fit(int id, size_t candidate_n, size_t max_points, size_t* total) const {
    size_t t = candidate_n;
    for (int i = 0; i < kMax; ++i)
      if (i != id) t += rec[i].n;
    *total = t;
    return t <= max_points;
  }

  // ---- layout of the aggregate built from the sources now ----
  bool is_lidar(int id) const { return rec[id].scan_fed || rec[id].kind == SourceKind::kSweep; }
  SourceLayout layout() const {
    SourceLayout L;
    for (int i = 0; i < kMax; ++i) {
      L.n[i] = rec[i].n;
      L.at[i] = L.total;
      L.total += rec[i].n;
      if (is_lidar(i)) L.lidar_mask |= (uint8_t)(1u << i);
    }
    return L;
  }

  // ---- the depth sources ----
  size_t depth_points() const {
    size_t n = 0;
    for (int i = 0; i < kMax; ++i)
      if (is_depth(rec[i].kind)) n += rec[i].n;
    return n;
  }
  bool any_depth() const {
    for (int i = 0; i < kMax; ++i)
      if (is_depth(rec[i].kind)) return true;
    return false;
  }
  int first_depth_without_frustum() const {          // -1: every depth source has one
    for (int i = 0; i < kMax; ++i)
      if (is_depth(rec[i].kind) && !rec[i].has_frustum) return i;
    return -1;
  }
  bool depth_frustums_ready() const { return any_depth() && first_depth_without_frustum() < 0; }
};

}  // namespace dddmr
