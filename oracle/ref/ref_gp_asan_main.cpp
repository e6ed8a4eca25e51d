/*
 * ref_gp_asan_main.cpp -- a stand-alone program that runs a file of planner cases through ref_gp_driver.cpp's own
 * entry points, built by `make -C oracle ref` with -fsanitize=address,undefined into oracle/_ref/ref_gp_asan (a program
 * with its own main: it needs no preload).  tests/test_global_plan_pin_cpu.py writes every case it sends to the
 * reference into such a file and requires exit status 0: the proof, independent of the restatement, that no pinned case
 * reaches the read of an emptied set's begin() (a_star_on_pre_graph.cpp:89).
 *
 * TEST INFRASTRUCTURE ONLY.  Our code.  The driver leaves every StaticGraph and planner allocated on purpose (see its
 * head), so the leak check is switched off below; every other check stays on and ends the program.
 *
 * File (little endian): u64 magic, u64 n_cases; per case u64 n, n_edges, n_dgraph, u32 start, goal, f64 radius,
 * inscribed_radius, descending_rate, max_obstacle_distance, turning_weight, then f32 xyzi[4n], u32 row_start[n + 1],
 * u32 neighbour[n_edges], f32 weight[n_edges], u32 order[n_edges], f64 dgraph[n_dgraph]; then u64 n_theta and
 * f32 xy[6 n_theta].  Prints one line per case and a checksum of the thetas.
 */
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int ref_gp_plan(const float* xyzi, std::size_t n, const uint32_t* row_start, const uint32_t* neighbour,
                           const float* weight, const uint32_t* order, std::size_t n_edges, const double* dgraph,
                           std::size_t n_dgraph, double radius, double inscribed_radius, double descending_rate,
                           double max_obstacle_distance, double turning_weight, uint32_t start, uint32_t goal,
                           uint32_t* path, std::size_t path_cap, std::size_t* path_len, float* g, float* f,
                           uint32_t* parent, uint8_t* opened, uint8_t* closed, std::size_t* set_size);
extern "C" void ref_gp_theta(const float* xy, std::size_t n, double* theta);
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {
const uint64_t MAGIC = 0x3153435047464552ull;   // "REFGPCS1"
const uint64_t LIMIT = 1u << 24;

template <class T> bool get(std::FILE* fp, std::vector<T>& v, std::size_t count) {
  v.resize(count);
  return count == 0 || std::fread(v.data(), sizeof(T), count, fp) == count;
}
template <class T> bool get(std::FILE* fp, T& v) { return std::fread(&v, sizeof(T), 1, fp) == 1; }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s CASES\n", argv[0]);
    return 2;
  }
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) {
    std::perror(argv[1]);
    return 2;
  }
  uint64_t magic = 0, n_cases = 0;
  if (!get(fp, magic) || !get(fp, n_cases) || magic != MAGIC) {
    std::fprintf(stderr, "%s: not a case file\n", argv[1]);
    return 2;
  }
  for (uint64_t c = 0; c < n_cases; ++c) {
    uint64_t n = 0, n_edges = 0, n_dgraph = 0;
    uint32_t ends[2];
    double par[5];
    if (!get(fp, n) || !get(fp, n_edges) || !get(fp, n_dgraph) || !get(fp, ends) || !get(fp, par) || n > LIMIT ||
        n_edges > LIMIT || n_dgraph > LIMIT) {
      std::fprintf(stderr, "case %llu: short or oversized header\n", (unsigned long long)c);
      return 2;
    }
    std::vector<float> xyzi, weight;
    std::vector<uint32_t> row_start, neighbour, order;
    std::vector<double> dgraph;
    if (!get(fp, xyzi, 4 * n) || !get(fp, row_start, n + 1) || !get(fp, neighbour, n_edges) || !get(fp, weight, n_edges) ||
        !get(fp, order, n_edges) || !get(fp, dgraph, n_dgraph)) {
      std::fprintf(stderr, "case %llu: short arrays\n", (unsigned long long)c);
      return 2;
    }
    std::vector<uint32_t> path(n + 1), parent(n);
    std::vector<float> g(n), f(n);
    std::vector<uint8_t> opened(n), closed(n);
    std::size_t path_len = 0, set_size = 0;
    const int rc = ref_gp_plan(xyzi.data(), n, row_start.data(), neighbour.data(), weight.data(), order.data(), n_edges,
                               dgraph.data(), n_dgraph, par[0], par[1], par[2], par[3], par[4], ends[0], ends[1],
                               path.data(), path.size(), &path_len, g.data(), f.data(), parent.data(), opened.data(),
                               closed.data(), &set_size);
    if (rc != 0) {
      std::fprintf(stderr, "case %llu: refused (%d)\n", (unsigned long long)c, rc);
      return 3;
    }
    std::printf("%llu %zu %zu\n", (unsigned long long)c, path_len, set_size);
  }
  uint64_t n_theta = 0;
  if (get(fp, n_theta)) {
    std::vector<float> xy;
    if (n_theta > LIMIT || !get(fp, xy, 6 * n_theta)) {
      std::fprintf(stderr, "short theta block\n");
      return 2;
    }
    std::vector<double> theta(n_theta);
    ref_gp_theta(xy.data(), n_theta, theta.data());
    uint64_t sum = 0;
    for (double t : theta) {
      uint64_t bits;
      std::memcpy(&bits, &t, sizeof bits);
      sum = sum * 1099511628211ull + bits;
    }
    std::printf("theta %llu %016llx\n", (unsigned long long)n_theta, (unsigned long long)sum);
  }
  std::fclose(fp);
  return 0;
}
