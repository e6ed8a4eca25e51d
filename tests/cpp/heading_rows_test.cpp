// The class-major deal of the rollout (csrc/rollout_kernels.hip.h): class_major_position() and heading_rows_shared()
// on the CPU.  For every shard shape below the position -> li function must be a permutation of [0, n_local), classes
// must ascend along it (members in ascending li), and where the predicate holds no window of rt positions may span more
// than two classes.  Then plan_tick()'s use of the predicate (csrc/tick_plan.hip.h): named ticks, one per branch of its
// LDS budget rule, against the row decision and the launch's dynamic LDS worked out by hand.  The program makes no HIP
// call.
#include <cstdio>
#include <cstring>
#include <vector>

#include "tick_plan.hip.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                             \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (++failures <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                \
  } while (0)

DevTick grid_tick(int begin, int n_local, int nth, int rt, int fixed_steps) {
  DevTick k;
  std::memset(&k, 0, sizeof(k));
  k.begin = begin;
  k.n_local = n_local;
  k.nth = nth;
  k.rt = rt;
  k.fixed_steps = fixed_steps;
  k.list_mode = 0;
  return k;
}

long check_shape(int begin, int n_local, int nth) {
  std::vector<int> seen((size_t)n_local, 0);
  std::vector<int> cls((size_t)n_local, 0);
  int last_cls = -1, last_li = -1, last_member = -1;
  for (int pos = 0; pos < n_local; ++pos) {
    const ClassPos cp = class_major_position(begin, n_local, nth, pos);
    CHECK(cp.li >= 0 && cp.li < n_local, "begin %d n_local %d nth %d pos %d -> li %d", begin, n_local, nth, pos, cp.li);
    if (cp.li < 0 || cp.li >= n_local) return 0;
    CHECK(seen[(size_t)cp.li]++ == 0, "begin %d n_local %d nth %d: li %d dealt twice", begin, n_local, nth, cp.li);
    CHECK(cp.cls == (begin + cp.li) % nth, "begin %d n_local %d nth %d pos %d: class %d of li %d", begin, n_local, nth, pos, cp.cls, cp.li);
    CHECK(cp.cls >= 0 && cp.cls < nth, "class %d out of [0, %d)", cp.cls, nth);
    if (cp.cls == last_cls) {
      CHECK(cp.li == last_li + nth && cp.member == last_member + 1, "begin %d n_local %d nth %d pos %d: members not ascending", begin, n_local, nth, pos);
    } else {
      CHECK(cp.cls > last_cls && cp.member == 0 && cp.li < nth, "begin %d n_local %d nth %d pos %d: class %d after %d, member %d", begin, n_local,
            nth, pos, cp.cls, last_cls, cp.member);
    }
    last_cls = cp.cls; last_li = cp.li; last_member = cp.member;
    cls[(size_t)pos] = cp.cls;
  }
  for (int li = 0; li < n_local; ++li) CHECK(seen[(size_t)li] == 1, "begin %d n_local %d nth %d: li %d never dealt", begin, n_local, nth, li);
  // windows of rt positions, as the rollout workgroups cut them, wherever the predicate holds
  long windows = 0;
  for (int rt = 1; rt <= kRolloutMax; ++rt) {
    const DevTick k = grid_tick(begin, n_local, nth, rt, 20);
    const bool holds = heading_rows_shared(k);
    CHECK(holds == (n_local / nth >= rt), "predicate %d for n_local %d nth %d rt %d", (int)holds, n_local, nth, rt);
    if (!holds) continue;
    for (int p0 = 0; p0 < n_local; p0 += rt) {
      const int p1 = std::min(p0 + rt, n_local) - 1;
      CHECK(cls[(size_t)p1] - cls[(size_t)p0] <= 1, "begin %d n_local %d nth %d rt %d: positions %d..%d span classes %d..%d", begin, n_local, nth, rt,
            p0, p1, cls[(size_t)p0], cls[(size_t)p1]);
      ++windows;
    }
  }
  return windows;
}

// ---- plan_tick()'s decision: shared rows or not, and the dynamic LDS of the launch that rolls out ----
// The rule (tick_plan.hip.h): with A = rollout_lds_bytes(rt, steps) = rt * (steps + 1) * 16 + 16 and
// H = heading_rows_lds_bytes(steps, omni) = 2 * (steps + 1) * (omni ? 32 : 16), a tick whose shape shares rows
// (heading_rows_shared) takes them when A + H <= 150 KB (153600, kScoreLdsMax) and either A + H <= 72 KB (73728: two
// rollout workgroups per CU) or A alone is already beyond 72 KB.  Every number below is worked out by hand from those
// two formulas; rt is what plan_tick's rollout tile rule gives (worked out in the case's comment).
struct RowsCase {
  const char* name;
  int kind, nx, ny, nth, steps;     // a grid tick of nx * ny * nth samples with bench_fixed_steps = steps
  int rt_override;                  // DDDMR_RT (0: the plan's own tile)
  bool knob, list_mode;             // DDDMR_HEADING_ROWS; the samples as an explicit list
  int world;                        // rank 0 of `world` ranks
  int want_rt, want_rows;
  size_t want_roll_lds, want_launch_lds;
};

void check_rows_case(const RowsCase& c) {
  dddmr_theory_config th;
  std::memset(&th, 0, sizeof(th));
  std::snprintf(th.name, sizeof(th.name), "rows");
  th.kind = c.kind;
  th.sim_time = 2.0;
  th.sim_granularity = 0.025;
  th.angular_sim_granularity = 0.1;
  th.controller_frequency = 10.0;
  th.bench_fixed_steps = c.steps;
  // a 0.1 m cube in the reference's push order (blb brb blt flb brt frt flt frb); no critics: k_score's LDS stays small
  const float lo = -0.05f, hi = 0.05f;
  const float cube[8][3] = {{lo, lo, lo}, {lo, hi, lo}, {lo, lo, hi}, {hi, lo, lo}, {lo, hi, hi}, {hi, hi, hi}, {hi, lo, hi}, {hi, hi, lo}};
  std::memcpy(th.cuboid, cube, sizeof(cube));
  Window w;
  for (int i = 0; i < c.nx; ++i) w.ax.push_back(0.1f + 0.4f * (float)i / (float)std::max(c.nx - 1, 1));
  for (int i = 0; i < c.ny; ++i) w.ay.push_back(c.ny > 1 ? -0.1f + 0.2f * (float)i / (float)(c.ny - 1) : 0.f);
  for (int i = 0; i < c.nth; ++i) w.ath.push_back(c.nth > 1 ? -0.5f + 1.0f * (float)i / (float)(c.nth - 1) : 0.f);
  if (c.list_mode) {
    w.list_mode = true;
    for (float x : w.ax) for (float y : w.ay) for (float t : w.ath) w.list.push_back(make_float4(x, y, t, 0.f));
  }
  dddmr_rollout_config cfg{};
  cfg.abi_version = DDDMR_ROLLOUT_ABI_VERSION;
  cfg.max_points = 16;
  cfg.max_trajectories = 1u << 20;
  cfg.max_steps = 4096;             // what create accepts at most
  cfg.max_plan_poses = 1;
  cfg.rank = 0;
  cfg.world_size = c.world;
  dddmr_tick_input in{};
  in.robot_pose[6] = 1.0;
  const double plan_last[7] = {0, 0, 0, 0, 0, 0, 1};
  TickKnobs kn;
  kn.rt_override = c.rt_override;
  kn.heading_rows = c.knob;
  TickPlan p;
  std::string err;
  const int rc = plan_tick(kn, TickFeedback{}, cfg, th, 0, in, w, 0, 0, plan_last, false, &p, &err);
  CHECK(rc == DDDMR_OK, "%s: plan_tick returned %d (%s)", c.name, rc, err.c_str());
  if (rc != DDDMR_OK) return;
  CHECK(p.s_tick == c.steps, "%s: horizon %d", c.name, p.s_tick);
  CHECK(p.k.rt == c.want_rt, "%s: rt %d, expected %d", c.name, p.k.rt, c.want_rt);
  CHECK(p.roll_lds == c.want_roll_lds, "%s: roll_lds %zu, expected %zu", c.name, p.roll_lds, c.want_roll_lds);
  CHECK(p.heading_rows == c.want_rows, "%s: heading_rows %d, expected %d", c.name, p.heading_rows, c.want_rows);
  CHECK(p.roll_launch_lds == c.want_launch_lds, "%s: launch LDS %zu, expected %zu", c.name, p.roll_launch_lds, c.want_launch_lds);
}

int check_rows_plan() {
  const int DD = DDDMR_THEORY_DD_SIMPLE, OMNI = DDDMR_THEORY_OMNI_SIMPLE;
  const RowsCase cases[] = {
      // BASELINE C1: 64 samples, rt = max(ceil(64 / 128), 4) = 4.  A = 4 * 21 * 16 + 16 = 1360, H = 2 * 21 * 16 = 672.
      {"C1 grid: rows on, far below 72 KB", DD, 8, 1, 8, 20, 0, true, false, 1, 4, 1, 1360, 2032},
      // BASELINE C3: 16384 samples x 80 steps, omni.  The tile rule: floor((74 * 1024 - 16) / (81 * 16)) = 58 rows fit
      // 74 KB, and of 58 .. 44 rows 50 fill the 1024-lane passes best (4050 of 4096).  A = 50 * 81 * 16 + 16 = 64816,
      // H = 2 * 81 * 32 = 5184, together 70000 <= 73728.
      {"C3 grid: rows on, within 72 KB", OMNI, 32, 16, 32, 80, 0, true, false, 1, 50, 1, 64816, 70000},
      // A <= 72 KB < A + H, the plan's own tile: 4608 omni samples x 127 steps.  36 rows fit 74 KB, ceil(4608 / 128) = 36
      // reaches that, and of 36 .. 27 rows 32 fill best (4096 of 4096).  A = 32 * 128 * 16 + 16 = 65552, H = 2 * 128 * 32
      // = 8192, together 73744 > 73728: no rows, the rollout's LDS alone.
      {"rows would cost the second workgroup per CU: off", OMNI, 24, 12, 16, 127, 0, true, false, 1, 32, 0, 65552, 65552},
      // ... and the fewest steps that reach that branch at all: 128 rows per workgroup (DDDMR_RT=128, the most), omni,
      // 34 steps.  A = 128 * 35 * 16 + 16 = 71696, H = 2 * 35 * 32 = 2240, together 73936 > 73728.
      {"the same at DDDMR_RT=128, 34 steps: off", OMNI, 16, 8, 2, 34, 128, true, false, 1, 128, 0, 71696, 71696},
      // one step fewer stays inside: A = 128 * 34 * 16 + 16 = 69648, H = 2 * 34 * 32 = 2176, together 71824 <= 73728.
      {"DDDMR_RT=128, 33 steps: on", OMNI, 16, 8, 2, 33, 128, true, false, 1, 128, 1, 69648, 71824},
      // A alone beyond 72 KB, the fewest steps: 128 rows x 35 steps.  A = 128 * 36 * 16 + 16 = 73744 > 73728: one
      // workgroup per CU either way, so the rows come along.  H = 2 * 36 * 16 = 1152, together 74896 <= 153600.
      {"rollout alone beyond 72 KB (DDDMR_RT=128, 35 steps): on", DD, 128, 1, 2, 35, 128, true, false, 1, 128, 1, 73744, 74896},
      // ... and with the plan's own tile: 16 samples x 1151 steps; floor((74 * 1024 - 16) / (1152 * 16)) = 4 rows fit 74 KB
      // and max(ceil(16 / 128), 4) = 4.  A = 4 * 1152 * 16 + 16 = 73744, H = 2 * 1152 * 16 = 36864, together 110608.
      {"rollout alone beyond 72 KB (own tile, 1151 steps): on", DD, 8, 1, 2, 1151, 0, true, false, 1, 4, 1, 73744, 110608},
      // Beyond kScoreLdsMax with the rows, the fewest steps: omni x 355 steps at DDDMR_RT=128, which the 128 KB cap of the
      // rollout's own LDS brings down to 23 rows (24 * 356 * 16 + 16 = 136720 > 131072).  A = 23 * 356 * 16 + 16 = 131024,
      // H = 2 * 356 * 32 = 22784, together 153808 > 153600: off.
      {"rows would pass 150 KB (DDDMR_RT=128, 355 steps): off", OMNI, 8, 4, 1, 355, 128, true, false, 1, 23, 0, 131024, 131024},
      // one step fewer fits: A = 23 * 355 * 16 + 16 = 130656, H = 2 * 355 * 32 = 22720, together 153376 <= 153600.
      {"DDDMR_RT=128, 354 steps: on", OMNI, 8, 4, 1, 354, 128, true, false, 1, 23, 1, 130656, 153376},
      // where the rows are never shared: the C1 grid again
      {"DDDMR_HEADING_ROWS=0: off", DD, 8, 1, 8, 20, 0, false, false, 1, 4, 0, 1360, 1360},
      {"list mode: off", DD, 8, 1, 8, 20, 0, true, true, 1, 4, 0, 1360, 1360},
      // rank 0 of 4 owns [0, 2 * 1 / 4) = nothing of two samples: no rollout workgroup, no LDS
      {"empty shard: off", DD, 1, 1, 2, 20, 0, true, false, 4, 0, 0, 0, 0},
  };
  for (const RowsCase& c : cases) check_rows_case(c);
  return (int)(sizeof(cases) / sizeof(cases[0]));
}

}  // namespace

int main() {
  long shapes = 0, windows = 0;
  const int plan_cases = check_rows_plan();
  const int nths[] = {1, 2, 8, 32};
  for (int nth : nths) {
    const int phases[] = {0, 1, nth - 1};
    for (int ph : phases) {
      if (ph < 0 || ph >= nth) continue;
      for (int lap : {0, 3}) {                        // begin beyond the first lap of the axis too
        const int begin = ph + lap * nth;
        std::vector<int> sizes = {nth, 4 * nth, 50 * nth, 4 * nth + 1, 7 * nth + nth / 2, 5 * nth + nth - 1, 1, 513, 4099};
        for (int m = 1; m < nth; m += (nth > 8 ? 5 : 1)) sizes.push_back(m);       // smaller than nth
        if (nth > 1) sizes.push_back(nth - 1);
        for (int n_local : sizes) {
          if (n_local <= 0) continue;
          windows += check_shape(begin, n_local, nth);
          ++shapes;
        }
      }
    }
  }
  // the BASELINE shards (whole grids on one rank) and their rollout tiles
  const int base[4][3] = {{64, 8, 4}, {4096, 16, 32}, {16384, 32, 50}, {65536, 64, 80}};
  for (const auto& b : base) {
    CHECK(heading_rows_shared(grid_tick(0, b[0], b[1], b[2], 20)), "BASELINE shape %d / %d, rt %d", b[0], b[1], b[2]);
    windows += check_shape(0, b[0], b[1]);
    ++shapes;
  }
  // where the rows are not shared
  DevTick k = grid_tick(0, 64, 8, 4, 20);
  CHECK(heading_rows_shared(k), "the C1 grid");
  k.list_mode = 1;
  CHECK(!heading_rows_shared(k), "list mode");
  k = grid_tick(0, 64, 8, 4, 0);
  CHECK(!heading_rows_shared(k), "the reference's step rule");
  k = grid_tick(0, 64, 8, 9, 20);
  CHECK(!heading_rows_shared(k), "thin shard: 8 members per class, 9 positions per workgroup");
  k = grid_tick(3, 5, 8, 1, 20);
  CHECK(!heading_rows_shared(k), "thin shard: fewer trajectories than classes");
  k = grid_tick(0, 0, 8, 4, 20);
  CHECK(!heading_rows_shared(k), "empty shard");
  if (failures) {
    std::printf("heading rows: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("heading rows OK: %ld shapes, %ld windows, %d plan cases\n", shapes, windows, plan_cases);
  return 0;
}
