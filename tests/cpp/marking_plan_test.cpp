// Replays tests/golden/marking_plan_cases.bin through make_update_frame() and plan_fused_update()
// (csrc/marking_plan.hip.h) on the CPU.  Every record holds the inputs of one marking update and what the engine
// launched for it when the record was taken (by the commit before marking_plan.hip.h existed, on an MI355X, over one run
// of tests/test_marking_gpu.py with default knobs).  Integers compare exactly, floats and doubles bit for bit.  Then the
// n_part estimate by hand, and the plan's invariants over the recorded inputs with every non-default knob.  The program
// makes no HIP call.
//
// Record: u32 magic "MKPL", u32 input bytes, u32 output bytes, then
//   inputs : dddmr_marking_config, f64 T_base_sensor[7], f64 T_gbl_base[7], ground grid (f32 ox oy oz inv_xy inv_z,
//            i32 nx ny nz), u32 max_row n_ground obs_cap_cells n_obs n_prev n_alive seq table pool_cap, f32 pad,
//            u32 grid_parts unmark_with_groups grid_in_lds splat_parts unmark_parts fuse_cells, u32 fused (the route taken)
//   outputs: MarkParams, then on the fused route u32 mark big, observation grid (as the ground grid, + u32 n; only
//            meaningful when mark), SplatRange (i32 cx0 cx1 cy0 cy1, u32 rows segs, i32 delta, u32 bands), u32 n_part
//            seg_groups, u32 count launch blocks (0: none), grid launch: u32 blocks nb_grid slot blocks, clear launch:
//            u32 blocks (0: skipped) nb_clear nb_cc, seed launch: u32 blocks (0: skipped) nb_roots nb_un nb_walk n_part_un,
//            partition launch: u32 launched blocks nb_un_groups nb_band_groups, commit launch: u32 blocks nb_commit nb_b
//            walk blocks; on either route last u32 launches_last_update
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "marking_plan.hip.h"

static_assert(sizeof(dddmr_marking_config) == 136, "dddmr_marking_config's layout changed: the recorded updates no longer describe it");
static_assert(sizeof(MarkParams) == 320, "MarkParams' layout changed: the recorded updates no longer describe it");

namespace {

struct Reader {
  const unsigned char* p;
  const unsigned char* end;
  bool ok = true;
  void get(void* out, size_t n) {
    if ((size_t)(end - p) < n) { ok = false; std::memset(out, 0, n); return; }
    std::memcpy(out, p, n);
    p += n;
  }
  template <typename T> T val() { T v; get(&v, sizeof(v)); return v; }
};

int failures = 0;
int rec = 0;   // the record being replayed
#define EXPECT_EQ(what, got, want)                                                                             \
  do { const long long g_ = (long long)(got), w_ = (long long)(want);   /* each evaluated once: `want` reads on */ \
    if (g_ != w_) { ++failures; std::fprintf(stderr, "record %d: %s is %lld, expected %lld\n", rec, what, g_, w_); } } while (0)
// floats and doubles: the same bits
#define EXPECT_BITS(what, got, want)                                                                           \
  do { const auto g_ = (got); const decltype(g_) w_ = (want);                                                  \
    if (std::memcmp(&g_, &w_, sizeof(g_)) != 0) { ++failures; std::fprintf(stderr, "record %d: %s is %.17g, expected %.17g\n", rec, what, (double)g_, (double)w_); } } while (0)

void read_geometry(Reader& r, PointGrid& g) {
  g.ox = r.val<float>(); g.oy = r.val<float>(); g.oz = r.val<float>(); g.inv_xy = r.val<float>(); g.inv_z = r.val<float>();
  g.nx = r.val<int32_t>(); g.ny = r.val<int32_t>(); g.nz = r.val<int32_t>();
}

void expect_params(const MarkParams& a, const MarkParams& b) {
#define F(x) EXPECT_BITS("MarkParams." #x, a.x, b.x)
#define I(x) EXPECT_EQ("MarkParams." #x, a.x, b.x)
  F(res); F(hres); F(marking_height); F(window); F(fov_top); F(fov_bottom); F(ps); F(pe); F(ns); F(ne);
  F(ignore_ratio); F(inscribed); F(inflation); F(tol); F(tol2); I(min_cluster); F(sd);
  for (int i = 0; i < 3; ++i) { F(sn[i]); F(st[i]); }
  for (int i = 0; i < 9; ++i) F(Rs[i]);
  for (int i = 0; i < 4; ++i) F(mc[i]);
  I(wx0); I(wx1); I(wy0); I(wy1); I(wz0); I(wz1);
  I(n_obs); I(n_prev); I(table_mask); I(pool_cap); I(n_ground); I(seq); I(n_alive_prev); F(pad);
#undef F
#undef I
}

struct Inputs {
  dddmr_marking_config cfg;
  double T_bs[7], T_gb[7];
  PointGrid ground;
  uint32_t max_row, n_ground, obs_cap, n_obs, n_prev, n_alive, seq, table, pool_cap;
  float pad;
  MarkKnobs kn;
};

FusedPlan plan_of(const Inputs& in, const MarkKnobs& kn, const UpdateFrame& f) {
  return plan_fused_update(kn, in.cfg, f, in.ground, in.max_row, in.n_ground, in.obs_cap, in.n_obs, in.n_alive, in.table);
}

// what holds for every plan, whatever the knobs
void expect_invariants(const Inputs& in, const MarkKnobs& kn, const FusedPlan& p, const char* knob) {
  char what[96];
#define EXPECT_INV(name, cond) do { std::snprintf(what, sizeof(what), "[%s] %s", knob, name); EXPECT_EQ(what, (int)(cond), 1); } while (0)
  EXPECT_INV("mark == n_obs > 5", p.mark == (in.n_obs > 5));
  if (!p.mark) {
    EXPECT_INV("nothing marked: no grid, union-find, seed, commit or band blocks",
               p.nb_grid == 0 && p.nb_cc == 0 && p.nb_roots == 0 && p.nb_commit == 0 && p.nb_b == 0 && p.count_blocks == 0);
    EXPECT_INV("nothing marked: no partition launch", p.part_launch() == 0 && p.nb_un_groups == 0 && p.nb_band_groups == 0);
    EXPECT_INV("nothing marked: a single walk block in the commit launch", p.nb_commit_walk == 1 && p.commit_launch() == 1);
  }
  if (p.rg.bands == 0) EXPECT_INV("no bands: no band blocks", p.nb_b == 0 && p.nb_un == 0 && p.nb_band_groups == 0);
  // removePCPtr's blocks: in exactly one of the seed and the partition launch, and only with markings alive
  const uint32_t un_seed = p.nb_un + p.nb_walk, un_part = p.nb_un_groups;
  EXPECT_INV("unmark blocks in one launch only", un_seed == 0 || un_part == 0);
  EXPECT_INV("unmark blocks iff markings alive", (un_seed + un_part > 0) == (in.n_alive > 0));
  EXPECT_INV("unmark blocks ride in the partition launch iff there is one and the knob says so",
             (un_part > 0) == (in.n_alive > 0 && p.mark && kn.unmark_with_groups));
  EXPECT_INV("band blocks of the partition launch are among its unmark blocks", p.nb_band_groups <= p.nb_un_groups);
  // every launch's grid is the sum of its parts
  EXPECT_INV("grid launch", p.grid_launch() == p.nb_grid + p.nb_slots && p.nb_slots == (in.table + 1023) / 1024 && p.grid_launch() > 0);
  EXPECT_INV("clear launch", p.clear_launch() == p.nb_clear + p.nb_cc);
  EXPECT_INV("seed launch", p.seed_launch() == p.nb_roots + p.nb_un + p.nb_walk);
  EXPECT_INV("partition launch", p.part_launch() == (p.mark ? (uint32_t)kFuseParts + p.nb_un_groups : 0u));
  EXPECT_INV("commit launch", p.commit_launch() == p.nb_commit + p.nb_b + p.nb_commit_walk && p.commit_launch() > 0);
  EXPECT_INV("the observation grid fits its storage", !p.mark || (uint64_t)p.obs.nx * p.obs.ny * p.obs.nz <= std::min(in.obs_cap, kn.fuse_cells));
  EXPECT_INV("the window's cells lie in the ground grid", p.rg.cx0 >= 0 && p.rg.cx0 <= p.rg.cx1 && p.rg.cx1 < in.ground.nx &&
                                                          p.rg.cy0 >= 0 && p.rg.cy0 <= p.rg.cy1 && p.rg.cy1 < in.ground.ny);
#undef EXPECT_INV
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s marking_plan_cases.bin\n", argv[0]); return 2; }
  std::vector<unsigned char> buf;
  {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    unsigned char chunk[65536];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    std::fclose(f);
  }

  // ---- the n_part estimate by hand: clamp(chunks + chunks / 3, 8, 48), chunks = (2 delta + 1) * ceil(max(1, n_obs / 2 / max(1, bands)) / 256) ----
  rec = -1;
  {
    MarkKnobs kn;
    EXPECT_EQ("n_part(6000 points, 27 bands, delta 4)", plan_n_part(kn, 6000, 27, 4), 12);     // 111 per band: 9 x 1 chunks, + 3
    EXPECT_EQ("n_part(32768 points, 10 bands, delta 4)", plan_n_part(kn, 32768, 10, 4), 48);   // 1638 per band: 9 x 7 chunks, + 21 = 84 -> 48
    EXPECT_EQ("n_part(6 points, no bands, delta 1)", plan_n_part(kn, 6, 0, 1), 8);             // 3 x 1 chunks, + 1 = 4 -> 8
    kn.splat_parts = 20;
    EXPECT_EQ("n_part forced (6000, 27, 4)", plan_n_part(kn, 6000, 27, 4), 20);
    EXPECT_EQ("n_part forced (32768, 10, 4)", plan_n_part(kn, 32768, 10, 4), 20);
    EXPECT_EQ("n_part forced (6, 0, 1)", plan_n_part(kn, 6, 0, 1), 20);
  }

  Reader file{buf.data(), buf.data() + buf.size()};
  int n_rec = 0, n_fused = 0, n_variants = 0;
  int kinds[6] = {0, 0, 0, 0, 0, 0};   // nothing marked, first update, alive markings, big, no bands, far from the origin
  while (file.p < file.end) {
    rec = n_rec;
    const uint32_t magic = file.val<uint32_t>(), n_in = file.val<uint32_t>(), n_out = file.val<uint32_t>();
    if (!file.ok || magic != 0x4C504B4Du || (size_t)(file.end - file.p) < (size_t)n_in + n_out) {
      std::fprintf(stderr, "record %d: malformed header\n", n_rec);
      return 1;
    }
    Reader in{file.p, file.p + n_in}, out{file.p + n_in, file.p + n_in + n_out};
    file.p += (size_t)n_in + n_out;

    Inputs I;
    in.get(&I.cfg, sizeof(I.cfg));
    in.get(I.T_bs, sizeof(I.T_bs));
    in.get(I.T_gb, sizeof(I.T_gb));
    read_geometry(in, I.ground);
    I.max_row = in.val<uint32_t>(); I.n_ground = in.val<uint32_t>(); I.obs_cap = in.val<uint32_t>(); I.n_obs = in.val<uint32_t>();
    I.n_prev = in.val<uint32_t>(); I.n_alive = in.val<uint32_t>(); I.seq = in.val<uint32_t>(); I.table = in.val<uint32_t>();
    I.pool_cap = in.val<uint32_t>();
    I.pad = in.val<float>();
    I.kn.grid_parts = in.val<uint32_t>();
    I.kn.unmark_with_groups = in.val<uint32_t>() != 0;
    I.kn.grid_in_lds = in.val<uint32_t>() != 0;
    I.kn.splat_parts = in.val<uint32_t>();
    I.kn.unmark_parts = in.val<uint32_t>();
    I.kn.fuse_cells = in.val<uint32_t>();
    const bool fused = in.val<uint32_t>() != 0;
    if (!in.ok || in.p != in.end) {
      std::fprintf(stderr, "record %d: malformed inputs\n", n_rec);
      return 1;
    }

    const UpdateFrame f = make_update_frame(I.cfg, I.T_bs, I.T_gb, I.n_obs, I.n_prev, I.table, I.pool_cap, I.n_ground, I.n_alive, I.seq, I.pad);
    MarkParams want;
    out.get(&want, sizeof(want));
    expect_params(f.k, want);

    if (fused) {
      const FusedPlan p = plan_of(I, I.kn, f);
      EXPECT_EQ("mark", p.mark, out.val<uint32_t>());
      EXPECT_EQ("big", p.big, out.val<uint32_t>());
      PointGrid og;
      read_geometry(out, og);
      og.n = out.val<uint32_t>();
      if (p.mark) {     // (an update that marks nothing leaves the grid of an older observation in place)
        EXPECT_BITS("obs.ox", p.obs.ox, og.ox); EXPECT_BITS("obs.oy", p.obs.oy, og.oy); EXPECT_BITS("obs.oz", p.obs.oz, og.oz);
        EXPECT_BITS("obs.inv_xy", p.obs.inv_xy, og.inv_xy); EXPECT_BITS("obs.inv_z", p.obs.inv_z, og.inv_z);
        EXPECT_EQ("obs.nx", p.obs.nx, og.nx); EXPECT_EQ("obs.ny", p.obs.ny, og.ny); EXPECT_EQ("obs.nz", p.obs.nz, og.nz);
        EXPECT_EQ("obs.n", p.obs.n, og.n);
      }
      EXPECT_EQ("rg.cx0", p.rg.cx0, out.val<int32_t>()); EXPECT_EQ("rg.cx1", p.rg.cx1, out.val<int32_t>());
      EXPECT_EQ("rg.cy0", p.rg.cy0, out.val<int32_t>()); EXPECT_EQ("rg.cy1", p.rg.cy1, out.val<int32_t>());
      EXPECT_EQ("rg.rows", p.rg.rows, out.val<uint32_t>()); EXPECT_EQ("rg.segs", p.rg.segs, out.val<uint32_t>());
      EXPECT_EQ("rg.delta", p.rg.delta, out.val<int32_t>()); EXPECT_EQ("rg.bands", p.rg.bands, out.val<uint32_t>());
      EXPECT_EQ("n_part", p.n_part, out.val<uint32_t>());
      EXPECT_EQ("seg_groups", p.seg_groups, out.val<uint32_t>());
      EXPECT_EQ("count launch", p.count_blocks, out.val<uint32_t>());
      EXPECT_EQ("grid launch", p.grid_launch(), out.val<uint32_t>());
      EXPECT_EQ("nb_grid", p.nb_grid, out.val<uint32_t>());
      EXPECT_EQ("nb_slots", p.nb_slots, out.val<uint32_t>());
      EXPECT_EQ("clear launch", p.clear_launch(), out.val<uint32_t>());
      EXPECT_EQ("nb_clear", p.nb_clear, out.val<uint32_t>());
      EXPECT_EQ("nb_cc", p.nb_cc, out.val<uint32_t>());
      EXPECT_EQ("seed launch", p.seed_launch(), out.val<uint32_t>());
      EXPECT_EQ("nb_roots", p.nb_roots, out.val<uint32_t>());
      EXPECT_EQ("nb_un", p.nb_un, out.val<uint32_t>());
      EXPECT_EQ("nb_walk", p.nb_walk, out.val<uint32_t>());
      EXPECT_EQ("n_part_un", p.n_part_un, out.val<uint32_t>());
      EXPECT_EQ("partition launch issued", p.part_launch() > 0, out.val<uint32_t>());
      EXPECT_EQ("partition launch", p.part_launch(), out.val<uint32_t>());
      EXPECT_EQ("nb_un_groups", p.nb_un_groups, out.val<uint32_t>());
      EXPECT_EQ("nb_band_groups", p.nb_band_groups, out.val<uint32_t>());
      EXPECT_EQ("commit launch", p.commit_launch(), out.val<uint32_t>());
      EXPECT_EQ("nb_commit", p.nb_commit, out.val<uint32_t>());
      EXPECT_EQ("nb_b", p.nb_b, out.val<uint32_t>());
      EXPECT_EQ("nb_commit_walk", p.nb_commit_walk, out.val<uint32_t>());
      // what the update launched, as far as the plan decides it (the store's housekeeping and a fallback to the general
      // route launch more)
      const uint32_t launched = out.val<uint32_t>();
      const uint32_t planned = (p.count_blocks > 0) + 1u + (p.clear_launch() > 0) + (p.seed_launch() > 0) + (p.part_launch() > 0) + 1u;
      EXPECT_EQ("launches_last_update >= the plan's launches", (int)(launched >= planned), 1);
      expect_invariants(I, I.kn, p, "recorded knobs");
      ++n_fused;
      kinds[0] += I.n_obs <= 5;
      kinds[1] += I.n_alive == 0;
      kinds[2] += I.n_alive > 0;
      kinds[3] += p.big;
      kinds[4] += p.rg.bands == 0;
      kinds[5] += std::fabs(I.T_gb[0]) > 1000.0;

      // ---- the recorded inputs again with every non-default knob ----
      struct Variant { const char* name; MarkKnobs kn; } variants[4];
      for (Variant& v : variants) v.kn = MarkKnobs();
      variants[0].name = "unmark_with_groups off"; variants[0].kn.unmark_with_groups = false;
      variants[1].name = "grid_in_lds off"; variants[1].kn.grid_in_lds = false;
      variants[2].name = "grid_parts 1"; variants[2].kn.grid_parts = 1;
      variants[3].name = "grid_parts 8"; variants[3].kn.grid_parts = 8;
      for (const Variant& v : variants) {
        const FusedPlan q = plan_of(I, v.kn, f);
        expect_invariants(I, v.kn, q, v.name);
        char what[96];
        std::snprintf(what, sizeof(what), "[%s] grid blocks", v.name);
        EXPECT_EQ(what, q.nb_grid, !q.mark ? 0u : ((v.kn.grid_in_lds || q.big) ? v.kn.grid_parts : 1u));
        std::snprintf(what, sizeof(what), "[%s] count launch only without the LDS grid, and never for a big observation", v.name);
        EXPECT_EQ(what, (int)(q.count_blocks > 0), (int)(q.mark && !v.kn.grid_in_lds && !q.big));
        ++n_variants;
      }
    } else {
      (void)out.val<uint32_t>();   // launches_last_update of the general route
    }
    if (!out.ok || out.p != out.end) {
      std::fprintf(stderr, "record %d: malformed outputs\n", n_rec);
      return 1;
    }
    ++n_rec;
  }
  rec = -1;
  // the kinds of update the recorded set has to hold
  const char* kind_names[6] = {"n_obs <= 5 (nothing marked)", "the first update (n_alive == 0)", "an update with alive markings",
                               "n_obs > 16384 (big)", "bands == 0", "an offset far from the origin"};
  for (int i = 0; i < 6; ++i)
    if (kinds[i] == 0) { ++failures; std::fprintf(stderr, "no fused record of the kind: %s\n", kind_names[i]); }
  if (failures) {
    std::fprintf(stderr, "%d mismatches in %d records\n", failures, n_rec);
    return 1;
  }
  std::printf("marking plan OK: %d records (%d fused, %d knob variants); kinds %d %d %d %d %d %d\n", n_rec, n_fused, n_variants, kinds[0], kinds[1],
              kinds[2], kinds[3], kinds[4], kinds[5]);
  return 0;
}
