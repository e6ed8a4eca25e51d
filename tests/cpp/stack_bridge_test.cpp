// PerceptionStackBridge (adapters/ros2/dddmr_rollout_adapter/include/dddmr_rollout_adapter/perception_bridge.h) WITHOUT ROS,
// PCL or a GPU, against a fake C ABI of its own: the fake keeps the stacked arrays, changes a random set of nodes in every
// pass and serves the change list in random order, or DDDMR_ERR_CAPACITY with the true count when the set is larger than
// max_changes.  After every pass the bridge's mirror must equal the fake's full arrays, bit for bit.  Built with
// -fsanitize=address,undefined and run as a program (tests/test_stack_cpu.py).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "dddmr_rollout_adapter/perception_bridge.h"

struct V3 { double x = 0, y = 0, z = 0; };
struct Q4 { double x = 0, y = 0, z = 0, w = 1; };
struct TransformStamped { struct { V3 translation; Q4 rotation; } transform; };
struct alignas(16) PointXYZ { float x = 0, y = 0, z = 0, pad = 1; };
template <class P> struct Cloud { typedef P PointType; std::vector<P> points; void push_back(const P& p) { points.push_back(p); } };

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// ---- fake C ABI ----
struct dddmr_rollout_ctx { int dummy; };
static struct Fake {
  bool created = false;
  dddmr_stack_config cfg{};
  std::vector<double> value;
  std::vector<uint8_t> mask;
  std::vector<uint32_t> changed;          // of the last pass, in the order the list is served
  std::vector<double> host;               // the last host layer handed over
  std::mt19937_64 rng{12345};
  size_t next_changes = 0;                // how many nodes the next pass changes
  int rc_update = DDDMR_OK;
  int n_full_dgraph = 0, n_full_mask = 0, n_update = 0, n_reset = 0;
} F;

static double random_value() {
  switch (F.rng() % 8) {
    case 0: return 99999.9;
    case 1: return -0.0;
    case 2: return 0.0;
    default: return (double)(F.rng() % 1000000) / 100.0;
  }
}

extern "C" {
int dddmr_rollout_stack_create(dddmr_rollout_ctx*, const dddmr_stack_config* cfg) {
  F.created = true; F.cfg = *cfg;
  F.value.assign((size_t)cfg->n_ground + 1, 99999.9); F.mask.assign((size_t)cfg->n_ground + 1, 0); F.changed.clear();
  for (size_t i = 0; i < F.value.size(); i += 3) { F.value[i] = random_value(); F.mask[i] = (uint8_t)(F.rng() % 4); }   // layers that hold state already
  return DDDMR_OK; }
int dddmr_rollout_stack_set_host_layer(dddmr_rollout_ctx*, int32_t slot, const double* v) {
  if (slot < 0 || slot >= F.cfg.n_host_layers) return DDDMR_ERR_BAD_ARG;
  F.host.assign(v, v + F.value.size()); return DDDMR_OK; }
int dddmr_rollout_stack_update(dddmr_rollout_ctx*, const double b2s[7], const double g2b[7], dddmr_stack_stats* st) {
  CHECK(F.created && b2s[6] == 1.0 && g2b[0] == 2.0 && st);
  ++F.n_update;
  std::memset(st, 0, sizeof(*st));
  // a random set of distinct nodes, each really changed (value bits or mask)
  std::vector<uint32_t> all(F.value.size());
  for (size_t i = 0; i < all.size(); ++i) all[i] = (uint32_t)i;
  std::shuffle(all.begin(), all.end(), F.rng);
  all.resize(F.next_changes);
  for (uint32_t i : all) {
    if (F.rng() % 4 == 0) { F.mask[i] = (uint8_t)((F.mask[i] + 1u + F.rng() % 7u) & 7u); continue; }
    double v; uint64_t a, b;
    do { v = random_value(); std::memcpy(&a, &v, 8); std::memcpy(&b, &F.value[i], 8); } while (a == b);
    F.value[i] = v;
  }
  F.changed = all;
  st->n_changed = (uint32_t)all.size();
  st->lidar_rc = F.rc_update;
  return F.rc_update; }
int dddmr_rollout_stack_get_changes(dddmr_rollout_ctx*, uint32_t* node, double* value, uint8_t* mask, size_t capacity, size_t* n) {
  *n = F.changed.size();
  if (F.changed.size() > F.cfg.max_changes || F.changed.size() > capacity) return DDDMR_ERR_CAPACITY;
  for (size_t i = 0; i < F.changed.size(); ++i) { node[i] = F.changed[i]; value[i] = F.value[F.changed[i]]; mask[i] = F.mask[F.changed[i]]; }
  return DDDMR_OK; }
int dddmr_rollout_stack_get_min_dgraph(dddmr_rollout_ctx*, double* out, size_t capacity) {
  if (capacity < F.value.size()) return DDDMR_ERR_CAPACITY;
  ++F.n_full_dgraph; std::memcpy(out, F.value.data(), F.value.size() * sizeof(double)); return DDDMR_OK; }
int dddmr_rollout_stack_get_lethal_mask(dddmr_rollout_ctx*, uint8_t* out, size_t capacity) {
  if (capacity < F.mask.size()) return DDDMR_ERR_CAPACITY;
  ++F.n_full_mask; std::memcpy(out, F.mask.data(), F.mask.size()); return DDDMR_OK; }
int dddmr_rollout_stack_reset(dddmr_rollout_ctx*) {
  ++F.n_reset; F.value.assign(F.value.size(), 9999.0); F.mask.assign(F.mask.size(), 0); F.changed.clear(); return DDDMR_OK; }
}

using dddmr_rollout_adapter::PerceptionStackBridge;

static void check_mirror(const PerceptionStackBridge& b, const char* what) {
  CHECK(b.minDGraph().size() == F.value.size() && b.lethalMasks().size() == F.mask.size());
  if (std::memcmp(b.minDGraph().data(), F.value.data(), F.value.size() * sizeof(double)) != 0 ||
      std::memcmp(b.lethalMasks().data(), F.mask.data(), F.mask.size()) != 0) {
    std::fprintf(stderr, "mirror differs from the full arrays: %s\n", what);
    std::exit(1);
  }
  for (unsigned i = 0; i < F.value.size(); i += 7) {
    uint64_t a, c; const double v = b.minDGraphValue(i);
    std::memcpy(&a, &v, 8); std::memcpy(&c, &F.value[i], 8);
    CHECK(a == c && b.lethalMask(i) == F.mask[i]);
  }
  CHECK(b.minDGraphValue((unsigned)F.value.size()) == 99999.9 && b.minDGraphValue(0xFFFFFFFFu) == 99999.9);
  CHECK(b.lethalMask((unsigned)F.mask.size()) == 0);
}

int main() {
  dddmr_rollout_ctx ctx{0};
  TransformStamped b2s, g2b;
  g2b.transform.translation.x = 2.0;
  int passes = 0, overflows = 0, lethal_listed = 0;
  const uint32_t grounds[] = {0, 1, 63, 500, 4225};
  for (uint32_t n_ground : grounds) {
    for (uint32_t max_changes : {0u, 1u, 16u, n_ground + 1}) {
      dddmr_stack_config cfg;
      std::memset(&cfg, 0, sizeof(cfg));
      cfg.n_ground = n_ground; cfg.use_lidar_layer = 1; cfg.use_depth_layer = 1; cfg.n_host_layers = 1; cfg.n_order = 3;
      cfg.layer_order[0] = DDDMR_STACK_HOST0; cfg.layer_order[1] = DDDMR_STACK_LIDAR; cfg.layer_order[2] = DDDMR_STACK_DEPTH;
      cfg.max_changes = max_changes;
      PerceptionStackBridge b;
      CHECK(!b.ready() && b.clearThenMark(b2s, g2b) == DDDMR_ERR_STATE);
      CHECK(b.create(nullptr, cfg) == DDDMR_ERR_BAD_ARG && !b.ready());
      CHECK(b.create(&ctx, cfg) == DDDMR_OK && b.ready());
      check_mirror(b, "after create over layers that hold state");
      CHECK(b.setHostLayer(0, std::vector<double>(n_ground + 1, 1.5)) == DDDMR_OK && F.host.size() == n_ground + 1);
      CHECK(b.setHostLayer(0, std::vector<double>(n_ground, 1.5)) == DDDMR_ERR_BAD_ARG);
      CHECK(b.setHostLayer(1, std::vector<double>(n_ground + 1, 1.5)) == DDDMR_ERR_BAD_ARG);
      for (int pass = 0; pass < 40; ++pass) {
        // sizes around the capacity, every node, none; an overflow is followed by passes that fit again
        const size_t nodes = (size_t)n_ground + 1;
        const size_t pick[] = {0, 1, max_changes, (size_t)max_changes + 1, nodes, (size_t)(F.rng() % (nodes + 1)), (size_t)(F.rng() % (max_changes + 1))};
        F.next_changes = std::min(nodes, pick[F.rng() % 7]);
        const int full_before = F.n_full_dgraph;
        dddmr_stack_stats st;
        bool resynced = false;
        F.rc_update = pass % 11 == 10 ? DDDMR_ERR_CAPACITY : DDDMR_OK;      // a layer failed: the code comes back, the mirror follows all the same
        CHECK(b.clearThenMark(b2s, g2b, &st, &resynced) == F.rc_update && b.ready());
        CHECK(st.n_changed == F.next_changes);
        const bool over = F.next_changes > max_changes;
        CHECK(resynced == over && (F.n_full_dgraph - full_before) == (over ? 1 : 0));
        overflows += over;
        ++passes;
        check_mirror(b, "after a pass");
      }
      // aggregateLethal: plugin order, ascending inside a layer, a node lethal in both layers twice, the last node never,
      // the host layer's bit (position 0) never
      Cloud<PointXYZ> ground, lethal;
      for (uint32_t i = 0; i < n_ground; ++i) { PointXYZ p; p.x = (float)i; ground.points.push_back(p); }
      b.aggregateLethal(ground, lethal);
      std::vector<float> want;
      for (int bit : {1, 2})
        for (uint32_t i = 0; i < n_ground; ++i)
          if ((F.mask[i] >> bit) & 1) want.push_back((float)i);
      CHECK(lethal.points.size() == want.size());
      for (size_t i = 0; i < want.size(); ++i) CHECK(lethal.points[i].x == want[i]);
      lethal_listed += (int)want.size();
      CHECK(b.reset() == DDDMR_OK && b.ready());
      check_mirror(b, "after reset");
      CHECK(b.minDGraphValue(0) == 9999.0);
    }
  }
  CHECK(overflows > 20 && passes - overflows > 20 && lethal_listed > 1000);
  std::printf("%d passes, %d overflows resynchronised, all mirrors equal\n", passes, overflows);
  return 0;
}
