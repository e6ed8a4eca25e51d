// Runs plan_pack_pairs() (csrc/rollout_kernels.hip.h) on the CPU for tests/test_plan_pairs_cpu.py.
// usage: plan_pairs_test in.bin out.bin
//   in : per case u32 m, then m float4 poses (x y z w)
//   out: u32 kPlanChunk, u32 kPlanTrip, u32 kPlanPoseWords, then per case u64 plan_padded_poses(m) and that many
//        poses as pair records (kPlanPoseWords floats each)
// The output buffer of every case has guard words behind it; a write past plan_padded_poses(m) poses fails the run.
// The program makes no HIP call.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rollout_kernels.hip.h"

using namespace dddmr;

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) { std::perror("open"); return 2; }
  const uint32_t head[3] = {(uint32_t)kPlanChunk, (uint32_t)kPlanTrip, (uint32_t)kPlanPoseWords};
  std::fwrite(head, sizeof(head), 1, out);
  constexpr size_t kGuard = 64;
  constexpr uint32_t kGuardBits = 0x7fc0dead;     // a NaN no repack produces
  int n_cases = 0;
  uint32_t m;
  while (std::fread(&m, sizeof(m), 1, in) == 1) {
    std::vector<float4> xyz(m);
    if (m && std::fread(xyz.data(), sizeof(float4), m, in) != m) { std::fprintf(stderr, "case %d: short input\n", n_cases); return 2; }
    const uint64_t n = plan_padded_poses(m);
    std::vector<float> rec(n * kPlanPoseWords + kGuard);
    for (auto& f : rec) std::memcpy(&f, &kGuardBits, 4);
    plan_pack_pairs(m ? xyz.data() : nullptr, m, rec.data());
    for (size_t g = 0; g < kGuard; ++g) {
      uint32_t bits;
      std::memcpy(&bits, &rec[n * kPlanPoseWords + g], 4);
      if (bits != kGuardBits) { std::fprintf(stderr, "case %d (m = %u): wrote past the padded size\n", n_cases, m); return 1; }
    }
    std::fwrite(&n, sizeof(n), 1, out);
    std::fwrite(rec.data(), sizeof(float), n * kPlanPoseWords, out);
    ++n_cases;
  }
  std::fclose(in);
  if (std::fclose(out) != 0) { std::perror("close"); return 2; }
  std::printf("plan pairs OK: %d cases\n", n_cases);
  return 0;
}
