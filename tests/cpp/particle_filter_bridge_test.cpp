// particle_filter_bridge.h without ROS, against a fake C-ABI (tests/test_particle_filter_cpu.py):
//   particle_filter_bridge_test SEED N N_DUPLICATES
// prints the canonical draw, the N noise rows the bridge hands the library (hex bit patterns), and the engine's next
// value after resample() has restored it, for comparison with the reference's recorded draws (tests/golden/REF_MCL_PF_*.npz).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "dddmr_rollout_adapter/particle_filter_bridge.h"

static uint32_t g_dup;
static std::vector<float> g_rows;
static double g_u;
static size_t g_n;

extern "C" {
int dddmr_rollout_mcl_filter_create(dddmr_rollout_ctx*, const dddmr_mcl_filter_config* cfg) { return cfg->max_particles ? DDDMR_OK : DDDMR_ERR_BAD_ARG; }
int dddmr_rollout_mcl_filter_set_particles(dddmr_rollout_ctx*, const float*, const float*, const float*, size_t n) { g_n = n; return DDDMR_OK; }
int dddmr_rollout_mcl_filter_resample(dddmr_rollout_ctx*, double u, const float* noise, size_t rows, dddmr_mcl_filter_resample_stats* stats) {
  g_u = u;
  g_rows.assign(noise, noise + 10 * rows);
  stats->n_duplicates = g_dup;
  return rows >= g_dup ? DDDMR_OK : DDDMR_ERR_CAPACITY;
}
}

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const unsigned seed = (unsigned)std::atol(argv[1]);
  const size_t n = (size_t)std::atol(argv[2]);
  g_dup = (uint32_t)std::atol(argv[3]);
  dddmr_rollout_adapter::ParticleFilterBridge b;
  dddmr_mcl_filter_resample_stats st;
  std::default_random_engine engine(seed);
  const float mean[6] = {0, 0, 0, 0, 0, 0}, sigma[6] = {0.2f, 0.2f, 0.2f, 0.2f, 0.2f, 0.1f};
  if (b.resample(engine, mean, sigma, &st) != DDDMR_ERR_STATE) return 3;              // before create
  int fake;
  dddmr_rollout_ctx* ctx = reinterpret_cast<dddmr_rollout_ctx*>(&fake);
  if (b.create(ctx, 0, 5.0, 10.0, 2.0, 1.57) != DDDMR_ERR_BAD_ARG || b.created()) return 4;
  if (b.create(ctx, 1 << 14, 5.0, 10.0, 2.0, 1.57) != DDDMR_OK || !b.created()) return 5;
  std::vector<float> states(13 * n, 0.0f);
  if (b.setParticles(states.data(), nullptr, nullptr, n) != DDDMR_OK || b.size() != n || g_n != n) return 6;
  if (b.resample(engine, mean, sigma, &st) != DDDMR_OK || st.n_duplicates != g_dup || g_rows.size() != 10 * n) return 7;
  std::printf("%08x\n", bits((float)g_u));
  for (size_t i = 0; i < g_rows.size(); ++i) std::printf("%08x%s", bits(g_rows[i]), (i % 10 == 9) ? "\n" : " ");
  std::printf("%u\n", (unsigned)engine());
  return 0;
}
