// The deal of the load-feedback assignment (deal_slot() of csrc/rollout_kernels.hip.h) and plan_tick()'s choice of it
// (TickPlan::deal, csrc/tick_plan.hip.h), on the CPU.
//  * every mode is a bijection from the ranks of an assignment group onto the slots k_score's workgroups read for it
//    (tile_slot() < n_local, congruent to the group), over a sweep of shard sizes, tiles and group counts;
//  * mode 0 is the formula the deal had before it had modes, restated below, rank for rank, the tail-round layouts included;
//  * in mode 1 the ranks of workgroup b all precede those of workgroup b + G, and with q = ng / tl, rem = ng % tl the
//    group's first rem workgroups hold q + 1 members and the others q (tile and tile - 1 on a shard that fills its tiles);
//  * in mode 2 the head workgroups hold the group's heaviest ranks and the tail workgroups its lightest;
//  * plan_tick picks the deal as specified, on named ticks.
// The program makes no HIP call.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tick_plan.hip.h"

namespace {

int failures = 0;
long checks = 0;
#define CHECK(cond, ...)                                             \
  do {                                                               \
    ++checks;                                                        \
    if (!(cond)) {                                                   \
      if (++failures <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                \
  } while (0)

// assign_block's group_slot lambda as it was before deal_slot() replaced it
int old_group_slot(const DevTick& k, int grp, int r) {
  const int G = k.assign_groups;
  const int n = k.n_local, tl = k.n_tiles / G, tlb = k.nb_tiles / G;
  const int ng = (n - grp + G - 1) / G;
  const int early = k.r0 * tlb;
  int start, width, round;
  if (r < early) { round = r / tlb; start = round * tlb; width = tlb; }
  else { round = k.r0 + (r - early) / tl; start = early + (round - k.r0) * tl; width = tl; }
  const int pos = r - start;
  const int bl = ((round & 1) && start + width <= ng) ? width - 1 - pos : pos;
  return grp + G * (start + bl);
}

// slot -> workgroup that reads it (k_score: slot tile_slot(k, b, j) for j < tile, when b takes part in round j), -1: nobody
void slot_owners(const DevTick& k, std::vector<int>* owner) {
  owner->assign((size_t)k.n_local, -1);
  for (int b = 0; b < k.n_tiles; ++b)
    for (int j = 0; j < k.tile; ++j) {
      if (!(b < k.nb_tiles || j + k.r0 < k.tile)) continue;
      const int s = tile_slot(k, b, j);
      if (s < 0 || s >= k.n_local) continue;
      CHECK((*owner)[(size_t)s] == -1, "slot %d read by two workgroups", s);
      (*owner)[(size_t)s] = b;
    }
}

// one layout, every mode: bijection, mode 0 against the restatement, the order and sizes of mode 1, the split of mode 2
void check_layout(const DevTick& k, const char* what) {
  const int G = k.assign_groups, n = k.n_local;
  std::vector<int> owner;
  slot_owners(k, &owner);
  for (int s = 0; s < n; ++s) CHECK(owner[(size_t)s] >= 0, "%s: slot %d of n %d tile %d G %d has no reader", what, s, n, k.tile, G);
  const int tl = k.n_tiles / G;
  std::vector<int> seen((size_t)n), first((size_t)k.n_tiles), last((size_t)k.n_tiles), members((size_t)k.n_tiles);
  const int heads[] = {0, 1, tl / 2, tl - 1, tl, tl + 3, -2};
  for (int mode = 0; mode <= 2; ++mode)
    for (int hi = 0; hi < (mode == 2 ? 7 : 1); ++hi) {
      const int head = heads[hi];
      std::fill(seen.begin(), seen.end(), 0);
      std::fill(first.begin(), first.end(), -1);
      std::fill(last.begin(), last.end(), -1);
      std::fill(members.begin(), members.end(), 0);
      for (int grp = 0; grp < G; ++grp) {
        const int ng = (n - grp + G - 1) / G;
        for (int r = 0; r < ng; ++r) {
          const int s = deal_slot(k, grp, r, mode, head);
          CHECK(s >= 0 && s < n && s % G == grp, "%s mode %d: rank %d of group %d -> slot %d (n %d tile %d G %d)", what, mode, r, grp, s, n, k.tile, G);
          if (s < 0 || s >= n) continue;
          CHECK(seen[(size_t)s] == 0, "%s mode %d: slot %d dealt twice (n %d tile %d G %d)", what, mode, s, n, k.tile, G);
          seen[(size_t)s] = 1;
          if (mode == 0 || k.r0 > 0)
            CHECK(s == old_group_slot(k, grp, r), "%s mode %d: rank %d of group %d -> %d, the old formula %d", what, mode, r, grp, s, old_group_slot(k, grp, r));
          const int b = owner[(size_t)s];
          if (b < 0) continue;
          CHECK(b % G == grp, "%s: slot %d of group %d belongs to workgroup %d", what, s, grp, b);
          if (first[(size_t)b] < 0) first[(size_t)b] = r;
          last[(size_t)b] = std::max(last[(size_t)b], r);
          ++members[(size_t)b];
        }
      }
      for (int s = 0; s < n; ++s) CHECK(seen[(size_t)s] == 1, "%s mode %d: slot %d not dealt (n %d tile %d G %d)", what, mode, s, n, k.tile, G);
      if (k.r0 > 0) continue;
      for (int grp = 0; grp < G; ++grp) {
        const int ng = (n - grp + G - 1) / G, q = ng / tl, rem = ng % tl;
        if (mode == 1) {
          for (int bl = 0; bl < tl; ++bl) {
            const int b = grp + G * bl, want = q + (bl < rem ? 1 : 0);
            CHECK(members[(size_t)b] == want, "%s sorted: workgroup %d holds %d, expected %d (n %d tile %d G %d)", what, b, members[(size_t)b], want, n, k.tile, G);
            if (ng > (k.tile - 1) * tl)     // the shard fills its tiles: `tile` members in the first ng - (tile - 1) * tl, tile - 1 behind
              CHECK(want == (bl < ng - (k.tile - 1) * tl ? k.tile : k.tile - 1), "%s sorted: size rule at workgroup %d", what, b);
            if (bl + 1 < tl && members[(size_t)b] > 0 && members[(size_t)(b + G)] > 0)
              CHECK(last[(size_t)b] < first[(size_t)(b + G)], "%s sorted: workgroup %d ends at rank %d, workgroup %d starts at %d", what, b,
                    last[(size_t)b], b + G, first[(size_t)(b + G)]);
            if (members[(size_t)b] > 0)
              CHECK(last[(size_t)b] - first[(size_t)b] + 1 == members[(size_t)b], "%s sorted: workgroup %d's ranks are not consecutive", what, b);
          }
        } else if (mode == 2) {
          const int hd = std::min(std::max(head, 0), tl);
          int head_max = -1, tail_min = ng;
          for (int bl = 0; bl < tl; ++bl) {
            const int b = grp + G * bl;
            CHECK(members[(size_t)b] == q + (bl < rem ? 1 : 0), "%s light tail: workgroup %d holds %d", what, b, members[(size_t)b]);
            if (members[(size_t)b] == 0) continue;
            if (bl < hd) head_max = std::max(head_max, last[(size_t)b]);
            else tail_min = std::min(tail_min, first[(size_t)b]);
          }
          CHECK(head_max < tail_min, "%s light tail (head %d): a head workgroup holds rank %d, a tail workgroup rank %d", what, hd, head_max, tail_min);
        }
      }
    }
}

long check_sweep() {
  long layouts = 0;
  for (int G = 1; G <= 4; ++G)
    for (int tile = 2; tile <= 16; ++tile) {
      std::vector<int> ns;
      for (int n = 1; n <= 260; ++n) ns.push_back(n);
      const int mults[] = {tile * 37, tile * 171, G * tile * 19, G * tile * 64, 2731, 4096, 4100};
      for (int m : mults)
        for (int d = -1; d <= 1; ++d)
          if (m + d > 260 && m + d <= 4200) ns.push_back(m + d);
      for (int n : ns) {
        DevTick k{};
        k.n_local = n;
        k.tile = tile;
        k.assign_groups = G;
        k.n_tiles = ((n + tile - 1) / tile + G - 1) / G * G;     // plan_tick: a multiple of the groups
        k.nb_tiles = k.n_tiles;
        k.r0 = 0;
        k.use_assign = 1;
        check_layout(k, "sweep");
        ++layouts;
      }
    }
  return layouts;
}

struct Shape { int nx, ny, nth, steps; };
const Shape kC2 = {16, 8, 32, 50}, kC3 = {32, 16, 32, 80};

// an omni grid tick with fixed steps, as tests/cpp/fused_walk_test.cpp builds it
int plan_of(const Shape& c, const TickKnobs& kn, bool have_feedback, int feedback_nlocal, TickPlan* p) {
  dddmr_theory_config th;
  std::memset(&th, 0, sizeof(th));
  std::snprintf(th.name, sizeof(th.name), "deal");
  th.kind = DDDMR_THEORY_OMNI_SIMPLE;
  th.sim_time = 2.0;
  th.sim_granularity = 0.025;
  th.angular_sim_granularity = 0.1;
  th.controller_frequency = 10.0;
  th.bench_fixed_steps = c.steps;
  const float lo = -0.05f, hi = 0.05f;
  const float cube[8][3] = {{lo, lo, lo}, {lo, hi, lo}, {lo, lo, hi}, {hi, lo, lo}, {lo, hi, hi}, {hi, hi, hi}, {hi, lo, hi}, {hi, hi, lo}};
  std::memcpy(th.cuboid, cube, sizeof(cube));
  th.critics[0].kind = DDDMR_CRITIC_COLLISION;
  th.critics[0].weight = 1.0;
  th.critics[1].kind = DDDMR_CRITIC_STICK_PATH;
  th.critics[1].weight = 1.0;
  th.n_critics = 2;
  Window w;
  for (int i = 0; i < c.nx; ++i) w.ax.push_back(0.1f + 0.4f * (float)i / (float)std::max(c.nx - 1, 1));
  for (int i = 0; i < c.ny; ++i) w.ay.push_back(c.ny > 1 ? -0.1f + 0.2f * (float)i / (float)(c.ny - 1) : 0.f);
  for (int i = 0; i < c.nth; ++i) w.ath.push_back(c.nth > 1 ? -0.5f + 1.0f * (float)i / (float)(c.nth - 1) : 0.f);
  dddmr_rollout_config cfg{};
  cfg.abi_version = DDDMR_ROLLOUT_ABI_VERSION;
  cfg.max_points = 1u << 20;
  cfg.max_trajectories = 1u << 20;
  cfg.max_steps = 4096;
  cfg.max_plan_poses = 1024;
  cfg.rank = 0;
  cfg.world_size = 1;
  dddmr_tick_input in{};
  in.robot_pose[6] = 1.0;
  const double plan_last[7] = {0, 0, 0, 0, 0, 0, 1};
  TickFeedback fb;
  if (have_feedback) {
    fb.load_theory = 0;
    fb.load_nlocal = feedback_nlocal;
    fb.collided_share = 0.25f;
  }
  std::string err;
  const int rc = plan_tick(kn, fb, cfg, th, 0, in, w, 500000, 80, plan_last, false, p, &err);
  CHECK(rc == DDDMR_OK, "plan_tick returned %d (%s)", rc, err.c_str());
  return rc;
}

int check_decisions() {
  int n = 0;
  struct Case { const char* name; Shape s; int deal_knob; bool tail_round; bool no_assign; int tile_override; bool feedback; int fb_delta;
                int want_assign, want_deal, want_tile; };
  const Case cases[] = {
      // C2: 4096 trajectories on 512 workgroups of 8: one round of resident workgroups, the snake
      {"C2 tick with feedback: one round, snake", kC2, -1, false, false, 0, true, 0, 1, kDealSnake, 8},
      // C3: 16384 trajectories in 2731 workgroups of 6 on 512 slots: several rounds, sorted
      {"C3 tick with feedback: sorted", kC3, -1, false, false, 0, true, 0, 1, kDealSorted, 6},
      {"C3 first tick of a context: no assignment, snake", kC3, -1, false, false, 0, false, 0, 0, kDealSnake, 6},
      {"C3 after a tick of another shard size: strided, snake", kC3, -1, false, false, 0, true, -1, 0, kDealSnake, 6},
      {"C3 DDDMR_DEAL=0", kC3, 0, false, false, 0, true, 0, 1, kDealSnake, 6},
      {"C3 DDDMR_DEAL=1", kC3, 1, false, false, 0, true, 0, 1, kDealSorted, 6},
      {"C3 DDDMR_DEAL=2", kC3, 2, false, false, 0, true, 0, 1, kDealLightTail, 6},
      {"C2 DDDMR_DEAL=1: sorted wherever there is an assignment", kC2, 1, false, false, 0, true, 0, 1, kDealSorted, 8},
      {"C2 DDDMR_DEAL=2", kC2, 2, false, false, 0, true, 0, 1, kDealLightTail, 8},
      {"C2 DDDMR_DEAL=1 without feedback: no assignment, snake", kC2, 1, false, false, 0, false, 0, 0, kDealSnake, 8},
      {"C3 DDDMR_NO_ASSIGN", kC3, -1, false, true, 0, true, 0, 0, kDealSnake, 6},
      {"C3 DDDMR_DEAL=1 with DDDMR_NO_ASSIGN", kC3, 1, false, true, 0, true, 0, 0, kDealSnake, 6},
      {"C3 DDDMR_TAIL_ROUND=1: the tail-round layout keeps the snake", kC3, -1, true, false, 0, true, 0, 1, kDealSnake, 6},
      {"C3 DDDMR_TAIL_ROUND=1 with DDDMR_DEAL=1", kC3, 1, true, false, 0, true, 0, 1, kDealSnake, 6},
      {"C3 with one trajectory a workgroup: nothing to sort into", kC3, -1, false, false, 1, true, 0, 1, kDealSnake, 1},
  };
  for (const Case& c : cases) {
    TickKnobs kn;
    kn.deal_mode = c.deal_knob;
    kn.tail_round = c.tail_round;
    kn.no_assign = c.no_assign;
    kn.tile_override = c.tile_override;
    if (c.tile_override) kn.threads_override = 512;
    TickPlan p;
    const int nl = c.s.nx * c.s.ny * c.s.nth;
    if (plan_of(c.s, kn, c.feedback, nl + c.fb_delta, &p) != DDDMR_OK) continue;
    ++n;
    CHECK(p.k.tile == c.want_tile, "%s: tile %d, expected %d", c.name, p.k.tile, c.want_tile);
    CHECK(p.k.use_assign == c.want_assign, "%s: use_assign %d, expected %d", c.name, p.k.use_assign, c.want_assign);
    CHECK(p.deal == c.want_deal, "%s: deal %d, expected %d", c.name, p.deal, c.want_deal);
    if (c.tail_round) CHECK(p.k.r0 > 0, "%s: the case must reach the tail-round layout, r0 %d", c.name, p.k.r0);
    if (p.deal == kDealLightTail) {
      // the whole rounds of 512 resident workgroups, per assignment group
      const int want_head = (p.k.n_tiles / 512) * 512 / p.k.assign_groups;
      CHECK(p.deal_head == want_head, "%s: deal_head %d, expected %d", c.name, p.deal_head, want_head);
    }
    if (p.k.use_assign) check_layout(p.k, c.name);     // the planned layouts themselves: C3's 2732 workgroups in 4 groups, the tail round
  }
  return n;
}

}  // namespace

int main() {
  const long layouts = check_sweep();
  const int decisions = check_decisions();
  if (failures) {
    std::printf("deal FAILED: %d checks of %ld\n", failures, checks);
    return 1;
  }
  std::printf("deal OK: %ld layouts, %d decisions, %ld checks\n", layouts, decisions, checks);
  return 0;
}
