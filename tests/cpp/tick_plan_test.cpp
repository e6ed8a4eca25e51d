// Replays tests/golden/tick_plan_cases.bin through plan_tick() (csrc/tick_plan.hip.h) on the CPU.  Every record holds
// the inputs of one tick's planning stage and what the engine decided for it when the record was taken (by the commit
// before plan_tick existed, on an MI355X: 256 compute units): the return code and, for a tick that was launched, its
// DevTick with seq zeroed, the k_score lanes / LDS / variant, the sample upload, the launch grids and the result's head.
// The program makes no HIP call.
//
// Record: u32 magic "TPLN", u32 input bytes, u32 output bytes, then
//   inputs : dddmr_theory_config, dddmr_tick_input, f32 cell_size, 12 x i32 (cell_forced gnz_one tile_override
//            threads_override rt_override tail_round final_mode probe_mode no_assign no_boxfast no_tab n_cu),
//            i32 load_theory, i32 load_nlocal, f32 collided_share, i32 theory_id, u32 max_points max_trajectories
//            max_steps max_plan_poses, i32 rank world_size, u32 n_points plan_m, f64 plan_last[7], i32 exchange,
//            i32 list_mode, u32 n_ax n_ay n_ath n_list, the floats of ax, ay, ath, list (4 per sample)
//   outputs: i32 rc, then for an error u32 length + message, else DevTick, i32 s_tick thr lean upload cnt_blocks
//            bin_blocks roll_blocks, u64 score_lds roll_lds, u32 n_samples local_begin n_local
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tick_plan.hip.h"

static_assert(sizeof(DevTick) == 1568, "DevTick's layout changed: the recorded ticks no longer describe it");

namespace {

struct Reader {
  const unsigned char* p;
  const unsigned char* end;
  bool ok = true;
  void get(void* out, size_t n) {
    if (n == 0) return;
    if ((size_t)(end - p) < n) { ok = false; std::memset(out, 0, n); return; }
    std::memcpy(out, p, n);
    p += n;
  }
  template <typename T> T val() { T v; get(&v, sizeof(v)); return v; }
};

int failures = 0;
#define EXPECT_EQ(rec, what, got, want)                                                                       \
  do { const long long g_ = (long long)(got), w_ = (long long)(want);   /* each evaluated once: `want` reads on */ \
    if (g_ != w_) { ++failures; std::fprintf(stderr, "record %d: %s is %lld, recorded %lld\n", rec, what, g_, w_); } } while (0)

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s tick_plan_cases.bin\n", argv[0]); return 2; }
  std::vector<unsigned char> buf;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    unsigned char chunk[65536];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    std::fclose(f);
  }
  Reader file{buf.data(), buf.data() + buf.size()};
  int n_rec = 0, n_ok = 0, n_err = 0;
  while (file.p < file.end) {
    const uint32_t magic = file.val<uint32_t>(), n_in = file.val<uint32_t>(), n_out = file.val<uint32_t>();
    if (!file.ok || magic != 0x4E4C5054u || (size_t)(file.end - file.p) < (size_t)n_in + n_out) {
      std::fprintf(stderr, "record %d: malformed header\n", n_rec);
      return 1;
    }
    Reader in{file.p, file.p + n_in}, out{file.p + n_in, file.p + n_in + n_out};
    file.p += (size_t)n_in + n_out;

    dddmr_theory_config th;
    dddmr_tick_input tick;
    in.get(&th, sizeof(th));
    in.get(&tick, sizeof(tick));
    TickKnobs kn;
    kn.cell_size = in.val<float>();
    kn.cell_forced = in.val<int32_t>() != 0;
    kn.gnz_one = in.val<int32_t>() != 0;
    kn.tile_override = in.val<int32_t>();
    kn.threads_override = in.val<int32_t>();
    kn.rt_override = in.val<int32_t>();
    kn.tail_round = in.val<int32_t>() != 0;
    kn.final_mode = in.val<int32_t>();
    kn.probe_mode = in.val<int32_t>();
    kn.no_assign = in.val<int32_t>() != 0;
    kn.no_boxfast = in.val<int32_t>() != 0;
    kn.no_tab = in.val<int32_t>() != 0;
    kn.n_cu = in.val<int32_t>();
    TickFeedback fb;
    fb.load_theory = in.val<int32_t>();
    fb.load_nlocal = in.val<int32_t>();
    fb.collided_share = in.val<float>();
    const int theory_id = in.val<int32_t>();
    dddmr_rollout_config cfg{};
    cfg.abi_version = DDDMR_ROLLOUT_ABI_VERSION;
    cfg.max_points = in.val<uint32_t>();
    cfg.max_trajectories = in.val<uint32_t>();
    cfg.max_steps = in.val<uint32_t>();
    cfg.max_plan_poses = in.val<uint32_t>();
    cfg.rank = in.val<int32_t>();
    cfg.world_size = in.val<int32_t>();
    const uint32_t n_points = in.val<uint32_t>(), plan_m = in.val<uint32_t>();
    double plan_last[7];
    in.get(plan_last, sizeof(plan_last));
    const bool exchange = in.val<int32_t>() != 0;
    Window w;
    w.list_mode = in.val<int32_t>() != 0;
    const uint32_t n_ax = in.val<uint32_t>(), n_ay = in.val<uint32_t>(), n_ath = in.val<uint32_t>(), n_list = in.val<uint32_t>();
    if (!in.ok || (size_t)(in.end - in.p) != ((size_t)n_ax + n_ay + n_ath + (size_t)4 * n_list) * sizeof(float)) {
      std::fprintf(stderr, "record %d: malformed inputs\n", n_rec);
      return 1;
    }
    w.ax.resize(n_ax); w.ay.resize(n_ay); w.ath.resize(n_ath); w.list.resize(n_list);
    in.get(w.ax.data(), n_ax * sizeof(float));
    in.get(w.ay.data(), n_ay * sizeof(float));
    in.get(w.ath.data(), n_ath * sizeof(float));
    in.get(w.list.data(), n_list * sizeof(float4));

    // the recorded window is the one make_window gives for the recorded theory and tick input
    {
      Window again;
      make_window(th, tick, again);
      const bool same = again.list_mode == w.list_mode && again.ax == w.ax && again.ay == w.ay && again.ath == w.ath &&
                        again.list.size() == w.list.size() &&
                        (w.list.empty() || std::memcmp(again.list.data(), w.list.data(), w.list.size() * sizeof(float4)) == 0);
      EXPECT_EQ(n_rec, "make_window == recorded window", (int)same, 1);
    }

    TickPlan plan;
    std::string err;
    const int rc = plan_tick(kn, fb, cfg, th, theory_id, tick, w, n_points, plan_m, plan_last, exchange, &plan, &err);
    const int want_rc = out.val<int32_t>();
    EXPECT_EQ(n_rec, "return code", rc, want_rc);
    if (want_rc != DDDMR_OK) {
      const uint32_t len = out.val<uint32_t>();
      std::string msg(len, '\0');
      out.get(&msg[0], len);
      if (err != msg) {
        ++failures;
        std::fprintf(stderr, "record %d: message '%s', recorded '%s'\n", n_rec, err.c_str(), msg.c_str());
      }
      ++n_err;
    } else if (rc == DDDMR_OK) {
      DevTick want;
      out.get(&want, sizeof(want));
      DevTick got = plan.k;
      got.seq = 0;
      if (std::memcmp(&got, &want, sizeof(DevTick)) != 0) {
        ++failures;
        const unsigned char *a = (const unsigned char*)&got, *b = (const unsigned char*)&want;
        size_t at = 0;
        while (a[at] == b[at]) ++at;
        std::fprintf(stderr, "record %d (%s): DevTick differs from the recorded one, first at byte %zu\n", n_rec, th.name, at);
      }
      EXPECT_EQ(n_rec, "s_tick", plan.s_tick, out.val<int32_t>());
      EXPECT_EQ(n_rec, "thr", plan.thr, out.val<int32_t>());
      EXPECT_EQ(n_rec, "lean", (int)plan.lean, out.val<int32_t>());
      EXPECT_EQ(n_rec, "upload", (int)plan.upload, out.val<int32_t>());
      EXPECT_EQ(n_rec, "cnt_blocks", plan.cnt_blocks, out.val<int32_t>());
      EXPECT_EQ(n_rec, "bin_blocks", plan.bin_blocks, out.val<int32_t>());
      EXPECT_EQ(n_rec, "roll_blocks", plan.roll_blocks, out.val<int32_t>());
      EXPECT_EQ(n_rec, "score_lds", plan.score_lds, out.val<uint64_t>());
      EXPECT_EQ(n_rec, "roll_lds", plan.roll_lds, out.val<uint64_t>());
      EXPECT_EQ(n_rec, "n_samples", plan.n_samples, out.val<uint32_t>());
      EXPECT_EQ(n_rec, "local_begin", plan.local_begin, out.val<uint32_t>());
      EXPECT_EQ(n_rec, "n_local", plan.n_local, out.val<uint32_t>());
      ++n_ok;
    }
    if (!out.ok || out.p != out.end) {
      std::fprintf(stderr, "record %d: malformed outputs\n", n_rec);
      return 1;
    }
    ++n_rec;
  }
  if (failures) {
    std::fprintf(stderr, "%d mismatches in %d records\n", failures, n_rec);
    return 1;
  }
  std::printf("tick plan OK: %d records (%d launched, %d refused)\n", n_rec, n_ok, n_err);
  return 0;
}
