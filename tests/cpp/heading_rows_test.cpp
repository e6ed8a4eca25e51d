// The class-major deal of the rollout (csrc/rollout_kernels.hip.h): class_major_position() and heading_rows_shared()
// on the CPU.  For every shard shape below the position -> li function must be a permutation of [0, n_local), classes
// must ascend along it (members in ascending li), and where the predicate holds no window of rt positions may span more
// than two classes.  The program makes no HIP call.
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

}  // namespace

int main() {
  long shapes = 0, windows = 0;
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
  std::printf("heading rows OK: %ld shapes, %ld windows\n", shapes, windows);
  return 0;
}
