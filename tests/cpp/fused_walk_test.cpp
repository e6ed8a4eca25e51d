// plan_tick()'s decision whether k_score walks the prune plan inside the collision walk (TickPlan::fused_walk,
// csrc/tick_plan.hip.h): named ticks, one per branch of the rule, against values worked out by hand.  The rule: the knob
// is on, the launch is lean, the collision critic is wanted, the cloud has at least 5 points, the plan at least one
// pose, a workgroup's pairs = tile x steps are more than 256 and at most the lane count, and the previous tick's
// collided share is at most 1 - 256 / pairs.  The program makes no HIP call.
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

struct FuseCase {
  const char* name;
  int nx, ny, nth, steps;        // an omni grid tick of nx * ny * nth samples with bench_fixed_steps = steps
  int tile_override, threads;    // DDDMR_TILE, DDDMR_THREADS (0: the plan's own shape)
  bool knob;                     // DDDMR_FUSE_WALK
  int critics;                   // bit 0 collision, bit 1 min-max, bit 2 stick path
  float half;                    // half edge of the cuboid: 0.05 keeps it inside the 1 m search ball (lean), 0.6 does not
  unsigned n_points, plan_m;
  float share;                   // TickFeedback::collided_share; < 0: a context's first tick (the struct's default)
  int world;
  int want_tile, want_thr, want_lean, want_fused;
};

void check_case(const FuseCase& c) {
  dddmr_theory_config th;
  std::memset(&th, 0, sizeof(th));
  std::snprintf(th.name, sizeof(th.name), "fuse");
  th.kind = DDDMR_THEORY_OMNI_SIMPLE;
  th.sim_time = 2.0;
  th.sim_granularity = 0.025;
  th.angular_sim_granularity = 0.1;
  th.controller_frequency = 10.0;
  th.bench_fixed_steps = c.steps;
  const float lo = -c.half, hi = c.half;   // the reference's push order: blb brb blt flb brt frt flt frb
  const float cube[8][3] = {{lo, lo, lo}, {lo, hi, lo}, {lo, lo, hi}, {hi, lo, lo}, {lo, hi, hi}, {hi, hi, hi}, {hi, lo, hi}, {hi, hi, lo}};
  std::memcpy(th.cuboid, cube, sizeof(cube));
  const int kinds[3] = {DDDMR_CRITIC_COLLISION, DDDMR_CRITIC_COLLISION_MIN_MAX, DDDMR_CRITIC_STICK_PATH};
  for (int b = 0; b < 3; ++b)
    if (c.critics & (1 << b)) {
      th.critics[th.n_critics].kind = kinds[b];
      th.critics[th.n_critics].weight = 1.0;
      ++th.n_critics;
    }
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
  cfg.world_size = c.world;
  dddmr_tick_input in{};
  in.robot_pose[6] = 1.0;
  const double plan_last[7] = {0, 0, 0, 0, 0, 0, 1};
  TickKnobs kn;
  kn.tile_override = c.tile_override;
  kn.threads_override = c.threads;
  kn.fuse_walk = c.knob;
  TickFeedback fb;
  CHECK(fb.collided_share == 1.0f, "a context's first tick must see every trajectory as collided, share %g", (double)fb.collided_share);
  if (c.share >= 0.f) {
    fb.load_theory = 0;
    fb.load_nlocal = c.nx * c.ny * c.nth / c.world;
    fb.collided_share = c.share;
  }
  TickPlan p;
  std::string err;
  const int rc = plan_tick(kn, fb, cfg, th, 0, in, w, c.n_points, c.plan_m, plan_last, false, &p, &err);
  CHECK(rc == DDDMR_OK, "%s: plan_tick returned %d (%s)", c.name, rc, err.c_str());
  if (rc != DDDMR_OK) return;
  CHECK(p.s_tick == c.steps, "%s: horizon %d", c.name, p.s_tick);
  CHECK(p.k.tile == c.want_tile, "%s: tile %d, expected %d", c.name, p.k.tile, c.want_tile);
  CHECK(p.thr == c.want_thr, "%s: lanes %d, expected %d", c.name, p.thr, c.want_thr);
  CHECK((int)p.lean == c.want_lean, "%s: lean %d, expected %d", c.name, (int)p.lean, c.want_lean);
  CHECK(p.fused_walk == c.want_fused, "%s: fused_walk %d, expected %d", c.name, p.fused_walk, c.want_fused);
}

int check_cases() {
  const int COLL = 1, MM = 2, STICK = 4;
  // C3's shape: 32 x 16 x 32 = 16384 samples x 80 steps; the shard does not fit one round of 512 workgroups of <= 16
  // trajectories, so the tile is the largest with tile * 80 <= 512: 6, 480 pairs, share bound 1 - 256 / 480 = 0.46667.
  // C2's shape: 16 x 8 x 32 = 4096 samples x 50 steps spread over 512 workgroups: tile 8, 400 pairs, bound 0.36.
  const FuseCase cases[] = {
      {"C3 shape, the measured 0.25: fused", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 500000, 80, 0.25f, 1, 6, 512, 1, 1},
      {"C3 shape just under its bound 0.46667", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 500000, 80, 0.4666f, 1, 6, 512, 1, 1},
      {"C3 shape just over its bound", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 500000, 80, 0.4668f, 1, 6, 512, 1, 0},
      {"C3 shape, nothing collided", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 500000, 80, 0.0f, 1, 6, 512, 1, 1},
      {"C3 shape, first tick of a context (share 1.0)", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 500000, 80, -1.f, 1, 6, 512, 1, 0},
      {"C3 shape, an r01 scene's 0.86", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 500000, 80, 0.86f, 1, 6, 512, 1, 0},
      {"C2 shape just under its bound 0.36", 16, 8, 32, 50, 0, 0, true, COLL | STICK, 0.05f, 500000, 50, 0.359f, 1, 8, 512, 1, 1},
      {"C2 shape just over its bound", 16, 8, 32, 50, 0, 0, true, COLL | STICK, 0.05f, 500000, 50, 0.361f, 1, 8, 512, 1, 0},
      {"DDDMR_FUSE_WALK=0", 32, 16, 32, 80, 0, 0, false, COLL | STICK, 0.05f, 500000, 80, 0.25f, 1, 6, 512, 1, 0},
      {"min-max critic: not lean", 32, 16, 32, 80, 0, 0, true, COLL | MM | STICK, 0.05f, 500000, 80, 0.25f, 1, 6, 512, 0, 0},
      // (a forced 4-trajectory tile: the pose words and the cuboid's eight cell rows make a pair's LDS larger)
      {"cuboid beyond the search ball: not lean", 32, 16, 32, 80, 4, 512, true, COLL | STICK, 0.6f, 500000, 80, 0.25f, 1, 4, 512, 0, 0},
      {"no collision critic", 32, 16, 32, 80, 0, 0, true, STICK, 0.05f, 500000, 80, 0.25f, 1, 6, 512, 1, 0},
      {"4-point cloud", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 4, 80, 0.25f, 1, 6, 512, 1, 0},
      {"5-point cloud", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 5, 80, 0.25f, 1, 6, 512, 1, 1},
      {"no plan", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 500000, 0, 0.25f, 1, 6, 512, 1, 0},
      {"one-pose plan", 32, 16, 32, 80, 0, 0, true, COLL | STICK, 0.05f, 500000, 1, 0.25f, 1, 6, 512, 1, 1},
      // forced shapes: DDDMR_TILE alone runs the 256-lane kernel
      {"7 x 80 = 560 pairs > 512 lanes", 32, 16, 32, 80, 7, 512, true, COLL | STICK, 0.05f, 500000, 80, 0.0f, 1, 7, 512, 1, 0},
      {"4 x 80 = 320 pairs > 256 lanes", 32, 16, 32, 80, 4, 0, true, COLL | STICK, 0.05f, 500000, 80, 0.0f, 1, 4, 256, 1, 0},
      {"3 x 80 = 240 pairs: phase P would split", 32, 16, 32, 80, 3, 512, true, COLL | STICK, 0.05f, 500000, 80, 0.0f, 1, 3, 512, 1, 0},
      {"4 x 64 = 256 pairs: phase P would split", 32, 16, 32, 64, 4, 512, true, COLL | STICK, 0.05f, 500000, 80, 0.0f, 1, 4, 512, 1, 0},
      {"8 x 64 = 512 pairs fill the lanes, bound 0.5", 32, 16, 32, 64, 8, 512, true, COLL | STICK, 0.05f, 500000, 80, 0.5f, 1, 8, 512, 1, 1},
      {"8 x 64 = 512 pairs just over 0.5", 32, 16, 32, 64, 8, 512, true, COLL | STICK, 0.05f, 500000, 80, 0.501f, 1, 8, 512, 1, 0},
      {"1 x 257 pairs, bound 0.0039: nothing collided", 8, 1, 8, 257, 1, 512, true, COLL | STICK, 0.05f, 500000, 80, 0.0f, 1, 1, 512, 1, 1},
      {"1 x 257 pairs, one in a hundred collided", 8, 1, 8, 257, 1, 512, true, COLL | STICK, 0.05f, 500000, 80, 0.01f, 1, 1, 512, 1, 0},
      // rank 0 of 4 owns nothing of two samples
      {"empty shard", 1, 1, 2, 300, 0, 0, true, COLL | STICK, 0.05f, 500000, 80, 0.0f, 4, 1, 512, 1, 0},
  };
  for (const FuseCase& c : cases) check_case(c);
  return (int)(sizeof(cases) / sizeof(cases[0]));
}

}  // namespace

int main() {
  // the bound itself, from its derivation: pairs x (1 - c) > 256 survivors while c < 1 - 256 / pairs
  CHECK(fused_walk_share_max(480) > 0.4666f && fused_walk_share_max(480) < 0.4667f, "C3 bound %g", (double)fused_walk_share_max(480));
  CHECK(fused_walk_share_max(400) > 0.3599f && fused_walk_share_max(400) < 0.3601f, "C2 bound %g", (double)fused_walk_share_max(400));
  CHECK(fused_walk_share_max(512) == 0.5f, "bound at 512 pairs %g", (double)fused_walk_share_max(512));
  const int n = check_cases();
  if (failures) {
    std::printf("fused walk plan FAILED: %d checks\n", failures);
    return 1;
  }
  std::printf("fused walk plan OK: %d cases\n", n);
  return 0;
}
