// Runs score_stack(), traj_load_of() and the slot-word helpers (csrc/rollout_kernels.hip.h) on the CPU for
// tests/test_score_tail_cpu.py: the one scoring function k_score's single-round tail and k_finalize share, against
// stacks worked out by hand.  usage: score_tail_test      (prints "score tail OK: <n> checks", exit status 0)
// The program makes no HIP call.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rollout_kernels.hip.h"

using namespace dddmr;

static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                                     \
  do {                                                                                  \
    ++n_checks;                                                                         \
    if (!(cond)) { ++n_failed; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } \
  } while (0)

struct Slot { int kind; double w, tw, ow; };

// a tick with a healthy cloud (>= 5 points) and an 80-pose plan unless told otherwise
static DevTick make_tick(const Slot* slots, int n, int n_points = 1000, int m = 80, double heading_dev = 0.5) {
  DevTick k;
  std::memset(&k, 0, sizeof(k));
  k.n_points = n_points;
  k.m = m;
  k.heading_dev = heading_dev;
  k.n_critics = n;
  for (int i = 0; i < n; ++i) {
    k.ckind[i] = slots[i].kind;
    k.cw[i] = slots[i].w;
    k.ctw[i] = slots[i].tw;
    k.cow[i] = slots[i].ow;
    if (slots[i].kind == DDDMR_CRITIC_COLLISION) k.want_collision = 1;
    if (slots[i].kind == DDDMR_CRITIC_COLLISION_MIN_MAX) k.want_minmax = 1;
  }
  return k;
}

struct Traj {
  float w = 0.25f;
  int steps = 40;
  bool hit_box = false, hit_mm = false;
  double stick_sum = 16.0, pp_dist = 2.0, pp_yaw = 0.5;
  float dist_last = 0.75f;
};

static double score(const DevTick& k, const Traj& t, int64_t* bits) {
  StackArgs sa;
  stack_args_load(k, sa);
  return score_stack(k, sa, t.w, t.steps, t.hit_box, t.hit_mm, t.stick_sum, t.pp_dist, t.pp_yaw, t.dist_last, bits);
}

static int64_t bits_of(double d) {
  int64_t i;
  std::memcpy(&i, &d, sizeof(i));
  return i;
}

int main() {
  int64_t b = 0;
  const Traj free_t;
  Traj boxed = free_t; boxed.hit_box = true; boxed.stick_sum = 0.0; boxed.dist_last = 0.f;
  Traj mmed = free_t; mmed.hit_mm = true; mmed.stick_sum = 0.0; mmed.dist_last = 0.f;

  // ---- the weights travel through the register tuples unchanged ----
  {
    const Slot s[8] = {{6, 1.5, -2.25, 1e-300}, {5, 3.0, 4.0, 5.0}, {2, 0, 0, 0}, {3, 0, 0.1, 0.2}, {4, 7, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0},
                       {6, 9.999999e6, 1e300, -0.0}};
    const DevTick k = make_tick(s, 8);
    StackArgs sa;
    stack_args_load(k, sa);
    for (int i = 0; i < 8; ++i) {
      CHECK(sa.kind[i] == s[i].kind);
      CHECK(bits_of(StackArgs::weight(sa.w, i)) == bits_of(s[i].w));
      CHECK(bits_of(StackArgs::weight(sa.tw, i)) == bits_of(s[i].tw));
      CHECK(bits_of(StackArgs::weight(sa.ow, i)) == bits_of(s[i].ow));
    }
  }
  // ---- every critic kind on its own ----
  {
    const Slot s[] = {{DDDMR_CRITIC_COLLISION, 1, 0, 0}};
    const DevTick k = make_tick(s, 1);
    CHECK(score(k, free_t, &b) == 0.0 && b == 0);
    CHECK(score(k, boxed, &b) == -1.0 && b == kKeyNone);
    CHECK(score(k, mmed, &b) == 0.0 && b == 0);                       // the other critic's verdict is not this one's
    const DevTick sparse = make_tick(s, 1, /*n_points=*/4);           // "< 5 points": the collision critics return 0
    CHECK(score(sparse, boxed, &b) == 0.0 && b == 0);
  }
  {
    const Slot s[] = {{DDDMR_CRITIC_COLLISION_MIN_MAX, 1, 0, 0}};
    const DevTick k = make_tick(s, 1);
    CHECK(score(k, free_t, &b) == 0.0);
    CHECK(score(k, mmed, &b) == -1.0 && b == kKeyNone);
    CHECK(score(k, boxed, &b) == 0.0);
  }
  {
    const Slot s[] = {{DDDMR_CRITIC_STICK_PATH, 1, 0, 0}};
    CHECK(score(make_tick(s, 1), free_t, &b) == 16.0 / 80.0 && b == bits_of(0.2));
    CHECK(score(make_tick(s, 1, 1000, 3), free_t, &b) == 16.0 / 3.0);
    CHECK(score(make_tick(s, 1, 1000, 2), free_t, &b) == 10.0);      // m < 3
    CHECK(score(make_tick(s, 1, 1000, 0), free_t, &b) == 10.0);
  }
  {
    const Slot s[] = {{DDDMR_CRITIC_PURE_PURSUIT, 0, 1.0, 0.01}};
    CHECK(score(make_tick(s, 1), free_t, &b) == 1.0 * 2.0 + 0.01 * 0.5);
    Traj one = free_t; one.steps = 1;
    CHECK(score(make_tick(s, 1), one, &b) == -4.0 && b == kKeyNone);  // steps < 2
    Traj two = free_t; two.steps = 2;
    CHECK(score(make_tick(s, 1), two, &b) == 1.0 * 2.0 + 0.01 * 0.5);
    CHECK(score(make_tick(s, 1, 1000, 0), free_t, &b) == -4.0);       // no plan
  }
  {
    const Slot s[] = {{DDDMR_CRITIC_TOWARD_GLOBAL_PLAN, 3.0, 0, 0}};
    CHECK(score(make_tick(s, 1), free_t, &b) == 0.75 * 3.0);
    CHECK(score(make_tick(s, 1, 1000, 2), free_t, &b) == 10.0);      // m < 3
  }
  {
    const Slot s[] = {{DDDMR_CRITIC_SHORTEST_ANGLE, 1.5, 0, 0}};
    Traj neg = free_t; neg.w = -0.25f;
    Traj zero = free_t; zero.w = 0.f;
    CHECK(score(make_tick(s, 1, 1000, 80, 0.5), free_t, &b) == 1.5);
    CHECK(score(make_tick(s, 1, 1000, 80, 0.5), neg, &b) == 3.0);
    CHECK(score(make_tick(s, 1, 1000, 80, 0.0), zero, &b) == 1.5);   // both comparisons are >=
    CHECK(score(make_tick(s, 1, 1000, 80, -0.5), free_t, &b) == 3.0);
    CHECK(score(make_tick(s, 1, 1000, 80, -0.5), neg, &b) == 1.5);
  }
  {
    const Slot s[] = {{DDDMR_CRITIC_TWIRLING, 4.0, 0, 0}};
    Traj neg = free_t; neg.w = -0.5f;
    CHECK(score(make_tick(s, 1), free_t, &b) == 1.0 && b == bits_of(1.0));
    CHECK(score(make_tick(s, 1), neg, &b) == 2.0);
  }
  // ---- the sum of a full stack, in stack order ----
  {
    const Slot s[] = {{DDDMR_CRITIC_COLLISION, 1, 0, 0}, {DDDMR_CRITIC_STICK_PATH, 1, 0, 0}, {DDDMR_CRITIC_PURE_PURSUIT, 0, 1.0, 0.01},
                      {DDDMR_CRITIC_TOWARD_GLOBAL_PLAN, 3.0, 0, 0}, {DDDMR_CRITIC_SHORTEST_ANGLE, 1.5, 0, 0}, {DDDMR_CRITIC_TWIRLING, 4.0, 0, 0}};
    const double want = ((((0.0 + 0.0) + 16.0 / 80.0) + (1.0 * 2.0 + 0.01 * 0.5)) + 0.75 * 3.0 + 1.5) + 1.0;
    CHECK(score(make_tick(s, 6), free_t, &b) == want && b == bits_of(want));
    CHECK(score(make_tick(s, 6), boxed, &b) == -1.0);
    // n_critics cuts the stack: slots behind it are not read
    DevTick cut = make_tick(s, 6);
    cut.n_critics = 2;
    CHECK(score(cut, free_t, &b) == 0.2);
  }
  // ---- a path critic AHEAD of a collision critic, collided trajectory: exactly -1, whatever its record holds ----
  {
    const Slot s[] = {{DDDMR_CRITIC_STICK_PATH, 1, 0, 0}, {DDDMR_CRITIC_TOWARD_GLOBAL_PLAN, 3.0, 0, 0}, {DDDMR_CRITIC_PURE_PURSUIT, 0, 1.0, 0.01},
                      {DDDMR_CRITIC_COLLISION, 1, 0, 0}, {DDDMR_CRITIC_TWIRLING, 4.0, 0, 0}};
    Traj garbage = boxed;
    garbage.stick_sum = std::nan(""); garbage.dist_last = std::nanf("");     // a dead trajectory's distances are never read
    CHECK(score(make_tick(s, 5), boxed, &b) == -1.0 && b == kKeyNone);
    CHECK(score(make_tick(s, 5), garbage, &b) == -1.0 && b == kKeyNone);
    const Slot s2[] = {{DDDMR_CRITIC_STICK_PATH, 1, 0, 0}, {DDDMR_CRITIC_COLLISION, 1, 0, 0}, {DDDMR_CRITIC_COLLISION_MIN_MAX, 1, 0, 0}};
    Traj gm = mmed; gm.stick_sum = std::nan("");
    CHECK(score(make_tick(s2, 3), gm, &b) == -1.0);
    // the first negative return wins: pure pursuit's guard ahead of the collision critic
    Traj one = boxed; one.steps = 1;
    CHECK(score(make_tick(s, 5), one, &b) == -4.0);
    // a sparse cloud: nobody is dead, the path critics count
    CHECK(score(make_tick(s2, 3, /*n_points=*/4), Traj{0.25f, 40, true, true, 16.0, 2.0, 0.5, 0.75f}, &b) == 0.2);
  }
  // ---- not generated ----
  {
    const Slot s[] = {{DDDMR_CRITIC_TWIRLING, 4.0, 0, 0}};
    Traj none = free_t; none.steps = 0;
    CHECK(score(make_tick(s, 1), none, &b) == DDDMR_COST_NOT_GENERATED && b == kKeyNone);
    CHECK(DDDMR_COST_NOT_GENERATED == -100.0);
  }
  // ---- the planner's cap (local_planner.cpp:452,460): 9999999 itself is accepted, anything above is not ----
  {
    Traj half = free_t; half.w = 0.5f;
    const Slot cap[] = {{DDDMR_CRITIC_TWIRLING, 2 * 9999999.0, 0, 0}};
    CHECK(score(make_tick(cap, 1), half, &b) == 9999999.0 && b == bits_of(9999999.0));
    const Slot over[] = {{DDDMR_CRITIC_TWIRLING, 4e7, 0, 0}};
    CHECK(score(make_tick(over, 1), half, &b) == 2e7 && b == kKeyNone);
    const Slot just[] = {{DDDMR_CRITIC_TWIRLING, 2 * 9999999.000000002, 0, 0}};
    CHECK(score(make_tick(just, 1), half, &b) > 9999999.0 && b == kKeyNone);
    CHECK(cost_bits(0.0) == 0 && cost_bits(-1.0) == kKeyNone && cost_bits(std::nan("")) == kKeyNone);
  }
  // ---- load feedback ----
  CHECK(traj_load_of(80, 7, 40, false) == 7u + 40u * (2u + 5u));
  CHECK(traj_load_of(80, 7, 40, true) == 7u + 40u * 2u);
  CHECK(traj_load_of(0, 0, 0, false) == 0u);
  CHECK(traj_load_of(81, 0, 1, false) == 2u + 6u);
  // ---- the record's flag word ----
  for (int walked : {0, 1, 12345, (1 << 29)})
    for (int hb = 0; hb < 2; ++hb)
      for (int hm = 0; hm < 2; ++hm) {
        const uint32_t f = partial_flags(walked, hb != 0, hm != 0);
        CHECK((int)(f >> 2) == walked && (int)(f & 1u) == hb && (int)((f >> 1) & 1u) == hm);
      }
  CHECK(sizeof(TrajPartial) == 32);
  // ---- slot word 3: w bits, collided and generated counts of a workgroup (up to 256 trajectories and beyond) ----
  {
    const uint32_t counts[] = {0, 1, 255, 256, 257, 1024};
    const uint32_t ws[] = {0u, 0x3f000000u, 0xbf800000u, 0xffffffffu};
    for (uint32_t c : counts)
      for (uint32_t g : counts)
        for (uint32_t w : ws) {
          const unsigned long long w3 = pack_slot_word3(w, c, g);
          CHECK(slot_w_bits(w3) == w && slot_collided(w3) == c && slot_generated(w3) == g);
        }
  }
  if (n_failed) { std::fprintf(stderr, "%d of %d checks failed\n", n_failed, n_checks); return 1; }
  std::printf("score tail OK: %d checks\n", n_checks);
  return 0;
}
