// The sensor sources' bookkeeping (csrc/source_table.hip.h) on the CPU: which calls a source's kind refuses, the scan
// sources' rules, the fit of a candidate observation, the aggregate's layout and the queries over the depth sources.
// The header makes no HIP call and uses no HIP type: this program is built with a plain host compiler.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "source_table.hip.h"

using namespace dddmr;

namespace {

int checks = 0, failures = 0;

#define CHECK(cond)                                                         \
  do {                                                                      \
    ++checks;                                                               \
    if (!(cond)) {                                                          \
      ++failures;                                                           \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
    }                                                                       \
  } while (0)

const char* kKindName[] = {"none", "scan", "depth cloud", "depth image", "sweep"};
const SourceKind kKinds[] = {SourceKind::kNone, SourceKind::kScan, SourceKind::kDepthCloud, SourceKind::kDepthImage, SourceKind::kSweep};

// a table whose source id has become the given kind the way the engine makes it one
SourceTable table_with(int id, SourceKind kind) {
  SourceTable t;
  if (kind == SourceKind::kScan) t.note_scan(id);
  else if (kind != SourceKind::kNone) t.configure(id, kind);
  return t;
}

bool same(const SourceTable& a, const SourceTable& b) {
  for (int i = 0; i < SourceTable::kMax; ++i) {
    const SourceRecord &x = a.rec[i], &y = b.rec[i];
    if (x.kind != y.kind || x.n != y.n || x.scan_fed != y.scan_fed || x.stitcher != y.stitcher || x.has_frustum != y.has_frustum) return false;
  }
  return a.multi_source == b.multi_source && a.depth_epoch == b.depth_epoch;
}

constexpr int OK = DDDMR_OK, ARG = DDDMR_ERR_BAD_ARG, STATE = DDDMR_ERR_STATE;

// What each call answers on a source of each kind, read off the entry points as they were before the table existed
// (the checks on depth[] / dimg[] / sweep[] / src_is_lidar[] / src_feed[] of rollout_engine.hip).
struct Row {
  SourceOp op;
  const char* name;
  int want[5];              // none, scan, depth cloud, depth image, sweep
  const char* why[5];       // the message's tail where refused
};
const Row kMatrix[] = {
    {SourceOp::kConfigureDepth, "configure as depth", {OK, ARG, OK, OK, ARG},
     {"", "is a lidar source", "", "", "is a lidar source"}},
    {SourceOp::kConfigureSweep, "configure as sweep", {OK, ARG, ARG, ARG, OK},
     {"", "is a scan source", "is a depth camera source", "is a depth camera source", ""}},
    {SourceOp::kFeedScan, "feed a scan", {OK, OK, ARG, ARG, ARG},
     {"", "", "is a depth camera source", "is a depth camera source", "is a lidar sweep source"}},
    {SourceOp::kFeedFrame, "feed a frame", {ARG, ARG, OK, ARG, ARG},
     {"is not a configured depth source", "is not a configured depth source", "", "is configured for depth images", "is not a configured depth source"}},
    {SourceOp::kFeedImage, "feed an image", {ARG, ARG, ARG, OK, ARG},
     {"is not a configured depth source", "is not a configured depth source", "is configured for point clouds", "", "is not a configured depth source"}},
    {SourceOp::kFeedSweep, "feed a sweep", {ARG, ARG, ARG, ARG, OK},
     {"is not a configured lidar sweep source", "is not a configured lidar sweep source", "is not a configured lidar sweep source",
      "is not a configured lidar sweep source", ""}},
    {SourceOp::kSetStitcher, "set a stitcher", {OK, OK, ARG, ARG, ARG},
     {"", "", "is a depth camera source", "is a depth camera source", "is a lidar sweep source (no stitcher on sweeps)"}},
    {SourceOp::kSetFrustum, "set a frustum", {STATE, STATE, OK, OK, STATE},
     {"is not a depth camera source", "is not a depth camera source", "", "", "is not a depth camera source"}},
    {SourceOp::kGetFrustum, "read a frustum (none set)", {STATE, STATE, STATE, STATE, STATE},
     {"has no frustum", "has no frustum", "has no frustum", "has no frustum", "has no frustum"}},
    {SourceOp::kSweepGetter, "sweep and feature getters", {STATE, STATE, STATE, STATE, OK},
     {"is not a lidar sweep source", "is not a lidar sweep source", "is not a lidar sweep source", "is not a lidar sweep source", ""}},
    {SourceOp::kImageCloudGetter, "read the image cloud", {ARG, ARG, ARG, OK, ARG},
     {"is not a depth image source", "is not a depth image source", "is not a depth image source", "", "is not a depth image source"}},
};

void refusal_matrix() {
  for (const Row& row : kMatrix)
    for (int k = 0; k < 5; ++k)
      for (int id : {0, 2}) {
        const SourceTable t = table_with(id, kKinds[k]);
        const Refusal r = t.refuse(row.op, id);
        ++checks;
        if (r.code != row.want[k] || std::strcmp(r.why, row.why[k]) != 0) {
          ++failures;
          std::printf("FAILED: %s on a %s source (id %d): code %d \"%s\", expected %d \"%s\"\n", row.name, kKindName[k], id, r.code, r.why,
                      row.want[k], row.why[k]);
        }
        // the other ids are untouched: whatever an unused id answers
        CHECK(t.refuse(row.op, 1).code == row.want[0]);
      }
  // a frustum can be read once it is set, on either kind of depth source
  for (SourceKind kind : {SourceKind::kDepthCloud, SourceKind::kDepthImage}) {
    SourceTable t = table_with(1, kind);
    t.set_frustum(1);
    CHECK(t.refuse(SourceOp::kGetFrustum, 1).code == OK);
  }
}

void scan_source_quirks() {
  {  // source 0 counts as a scan source while its stitcher count is above 0, even before any scan
    SourceTable t;
    t.note_stitcher(0, 2);
    CHECK(t.rec[0].kind == SourceKind::kScan && !t.rec[0].scan_fed);
    CHECK(t.refuse(SourceOp::kConfigureDepth, 0).code == ARG);
    CHECK(t.refuse(SourceOp::kConfigureSweep, 0).code == ARG);
    CHECK(!t.is_lidar(0));                              // ... but its (empty) segment is no lidar's before a scan
    t.note_stitcher(0, 0);                              // stitcher off again: nothing says scan source any more
    CHECK(t.rec[0].kind == SourceKind::kNone);
    CHECK(t.refuse(SourceOp::kConfigureDepth, 0).code == OK);
    t.note_scan(0);                                     // once fed, switching the stitcher off changes nothing
    t.note_stitcher(0, 0);
    CHECK(t.refuse(SourceOp::kConfigureDepth, 0).code == ARG);
  }
  {  // a source above 0 counts as one from its first set_stitcher_source, whatever the count
    SourceTable t;
    t.note_stitcher(2, 0);
    CHECK(t.rec[2].kind == SourceKind::kScan);
    CHECK(t.refuse(SourceOp::kConfigureDepth, 2).code == ARG);
    CHECK(t.refuse(SourceOp::kConfigureSweep, 2).code == ARG);
    CHECK(!t.multi_source);                             // a stitcher call alone does not switch plain set_scan over
  }
  {  // plain set_scan means source 0 once any per-source call has been made
    SourceTable t;
    CHECK(t.scan_source(-1) == -1 && t.scan_source(3) == 3);
    t.note_scan(-1);                                    // the single-producer form: the lidar of source 0, no switch
    CHECK(t.scan_source(-1) == -1 && t.rec[0].scan_fed && t.is_lidar(0) && !t.multi_source);
    CHECK(t.refuse(SourceOp::kConfigureDepth, 0).code == ARG);
    t.note_scan(1);
    CHECK(t.scan_source(-1) == 0 && t.scan_source(1) == 1);
    for (SourceKind kind : {SourceKind::kDepthCloud, SourceKind::kDepthImage, SourceKind::kSweep}) {
      SourceTable u;
      u.configure(3, kind);
      CHECK(u.scan_source(-1) == 0);
    }
  }
  {  // the lidar flag is set before the feed runs and stays when the feed fails: no count is needed for it
    SourceTable t;
    t.note_scan(1);
    CHECK(t.rec[1].n == 0 && t.is_lidar(1) && (t.layout().lidar_mask & 2u));
  }
}

void candidate_fit() {
  SourceTable t;
  t.note_scan(0);
  t.configure(2, SourceKind::kDepthCloud);
  t.configure(3, SourceKind::kSweep);
  const uint32_t counts[4] = {3, 0, 5, 2};
  for (int i = 0; i < 4; ++i) t.set_count(i, counts[i]);
  const SourceTable before = t;
  size_t total = 0;
  CHECK(t.would_fit(1, 0, 10, &total) && total == 10);
  CHECK(same(t, before));
  CHECK(!t.would_fit(1, 1, 10, &total) && total == 11);
  CHECK(same(t, before));
  CHECK(!t.would_fit(0, 4, 10, &total) && total == 11);
  CHECK(same(t, before));
  CHECK(t.would_fit(0, 3, 10, &total) && total == 10);
  CHECK(same(t, before));
}

void layout_and_depth_queries() {
  SourceTable t;
  CHECK(!t.any_depth() && !t.depth_frustums_ready() && t.depth_points() == 0);
  t.note_scan(0);                                       // scan, nothing, depth cloud, sweep
  t.configure(2, SourceKind::kDepthCloud);
  t.configure(3, SourceKind::kSweep);
  t.set_count(0, 3);
  t.set_count(2, 5);
  t.set_count(3, 2);
  const SourceLayout L = t.layout();
  const uint32_t want_n[4] = {3, 0, 5, 2}, want_at[4] = {0, 3, 3, 8};
  for (int i = 0; i < 4; ++i) CHECK(L.n[i] == want_n[i] && L.at[i] == want_at[i]);
  CHECK(L.total == 10 && L.lidar_mask == 0x9 && L.from_sources);
  const SourceLayout one = single_lidar_layout(7);
  CHECK(one.n[0] == 7 && one.total == 7 && one.lidar_mask == 1 && one.from_sources && one.n[1] == 0 && one.at[3] == 0);
  CHECK(!foreign_layout().from_sources);

  CHECK(t.any_depth() && t.depth_points() == 5);
  CHECK(!t.depth_frustums_ready() && t.first_depth_without_frustum() == 2);
  const uint64_t epoch = t.depth_epoch;
  t.set_frustum(2);
  CHECK(t.depth_frustums_ready() && t.first_depth_without_frustum() == -1);
  CHECK(t.depth_epoch == epoch);
  t.configure(1, SourceKind::kDepthImage);              // a second depth source: all of them must have one
  CHECK(!t.depth_frustums_ready() && t.first_depth_without_frustum() == 1);
  t.set_frustum(1);
  CHECK(t.depth_frustums_ready());
  t.set_count(1, 4);
  CHECK(t.depth_points() == 9 && t.depth_epoch == epoch + 1);   // a depth observation changed
  t.set_count(3, 1);
  CHECK(t.depth_epoch == epoch + 1);                    // a sweep's does not count

  // reconfiguring a depth source: its points and its frustum leave, the observation grid is stale
  t.release(2);
  CHECK(t.rec[2].kind == SourceKind::kNone && t.depth_epoch == epoch + 2);
  t.configure(2, SourceKind::kDepthCloud);
  CHECK(t.rec[2].n == 0 && !t.rec[2].has_frustum);
  CHECK(t.depth_points() == 4 && !t.depth_frustums_ready() && t.first_depth_without_frustum() == 2);
  CHECK(t.refuse(SourceOp::kGetFrustum, 2).code == STATE);
  const SourceLayout M = t.layout();
  CHECK(M.n[2] == 0 && M.at[3] == 7 && M.total == 8 && M.lidar_mask == 0x9);
  // releasing a sweep source clears its lidar flag with it
  t.release(3);
  CHECK(t.layout().lidar_mask == 0x1 && t.depth_epoch == epoch + 2);
}

}  // namespace

int main() {
  refusal_matrix();
  scan_source_quirks();
  candidate_fit();
  layout_and_depth_queries();
  if (failures) {
    std::printf("source table: %d of %d checks FAILED\n", failures, checks);
    return 1;
  }
  std::printf("source table OK: %d checks\n", checks);
  return 0;
}
