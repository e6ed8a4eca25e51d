// A host A* over downloaded arrays, for tools/global_plan_bench.py: a RESTATEMENT of A_Star_on_PreGraph::getPath with the
// reference's containers (std::set<std::pair<float, unsigned>> as the frontier, std::unordered_map<unsigned, Node> as the
// list, Initial() clearing every node before each plan) -- this tool's own code, NOT the reference, which cannot be built
// here.  Arithmetic: csrc/global_plan_plan.hip.h.  It reads one binary file
//   uint32 n, uint64 n_edges, uint32 n_queries, double turning_weight, radius, inscribed, rate,
//   uint32 row_start[n + 1], uint32 neighbour[n_edges], float weight[n_edges], float xyz[n][3], double dgraph[n + 1],
//   uint32 start[n_queries], uint32 goal[n_queries]
// runs every query `reps` times and prints per query: path length, expansions, and the median time in microseconds.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

#include "global_plan_plan.hip.h"

struct Node { unsigned self_index; float g, h, f; unsigned parent_index; bool is_closed, is_opened; };

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int reps = std::atoi(argv[2]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0, nq = 0;
  uint64_t ne = 0;
  double par[4];
  if (!rd(f, &n, 1) || !rd(f, &ne, 1) || !rd(f, &nq, 1) || !rd(f, par, 4)) return 2;
  std::vector<uint32_t> row_start(n + 1), neighbour(ne), start(nq), goal(nq);
  std::vector<float> weight(ne), xyz(3 * (size_t)n);
  std::vector<double> dgraph(n + 1);
  if (!rd(f, row_start.data(), n + 1) || !rd(f, neighbour.data(), ne) || !rd(f, weight.data(), ne) || !rd(f, xyz.data(), 3 * (size_t)n) ||
      !rd(f, dgraph.data(), n + 1) || !rd(f, start.data(), nq) || !rd(f, goal.data(), nq))
    return 2;
  std::fclose(f);
  const double tw = par[0], radius = par[1], inscribed = par[2], rate = par[3];
  std::unordered_map<unsigned, Node> list;
  std::set<std::pair<float, unsigned>> frontier;
  for (uint32_t q = 0; q < nq; ++q) {
    std::vector<double> us;
    size_t path_len = 0, expanded = 0;
    for (int r = 0; r < reps; ++r) {
      const auto t0 = std::chrono::steady_clock::now();
      const unsigned s = start[q], g = goal[q];
      const float* pg = &xyz[3 * (size_t)g];
      // Initial(): every node of the graph gets a cleared record
      list.clear();
      for (uint32_t i = 0; i < n; ++i) list[i] = Node{0, 0, 0, 0, 0, false, false};
      frontier.clear();
      const float f0 = dddmr::gp_dist(xyz[3 * (size_t)s], xyz[3 * (size_t)s + 1], xyz[3 * (size_t)s + 2], pg[0], pg[1], pg[2]);
      list[s] = Node{s, 0, 0, f0, s, false, true};
      frontier.insert({f0, s});
      std::vector<unsigned> path;
      expanded = 0;
      while (!frontier.empty()) {
        auto it = frontier.begin();
        Node cur = list[it->second];
        if (!cur.is_closed) {
          frontier.erase(it);
        } else {
          while (cur.is_closed && !frontier.empty()) {
            frontier.erase(it);
            if (frontier.empty()) break;                     // (the reference reads begin() of the empty set here)
            it = frontier.begin();
            cur = list[it->second];
          }
          if (cur.is_closed) break;
        }
        const float* pc = &xyz[3 * (size_t)cur.self_index];
        const float* pp = &xyz[3 * (size_t)cur.parent_index];
        for (uint32_t e = row_start[cur.self_index]; e < row_start[cur.self_index + 1]; ++e) {
          const unsigned nb = neighbour[e];
          const double d = dgraph[nb];
          if (dddmr::gp_edge_skipped(weight[e], radius, d, inscribed)) continue;
          const float* pe = &xyz[3 * (size_t)nb];
          const double factor = dddmr::gp_factor(rate, d, inscribed);
          const double theta = dddmr::gp_theta(pp[0], pp[1], pc[0], pc[1], pe[0], pe[1]);
          const float new_g = dddmr::gp_new_g(cur.g, weight[e], factor, theta, tw, 0.f);
          const float new_h = dddmr::gp_dist(pe[0], pe[1], pe[2], pg[0], pg[1], pg[2]);
          const float new_f = new_g + new_h;
          Node& rec = list[nb];
          if (rec.is_closed) continue;
          if (rec.is_opened && !(rec.g > new_g)) continue;
          rec = Node{nb, new_g, new_h, new_f, cur.self_index, false, true};
          frontier.insert({new_f, nb});
        }
        list[cur.self_index].is_closed = true;
        ++expanded;
        if (list[g].is_closed) {
          Node t = list[g];
          while (t.self_index != t.parent_index) { path.push_back(t.self_index); t = list[t.parent_index]; }
          path.push_back(t.self_index);
          std::reverse(path.begin(), path.end());
          break;
        }
      }
      const auto t1 = std::chrono::steady_clock::now();
      us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
      path_len = path.size();
    }
    std::sort(us.begin(), us.end());
    std::printf("Q %u %zu %zu %.3f %.3f %.3f\n", q, path_len, expanded, us[us.size() / 10], us[us.size() / 2], us[(9 * us.size()) / 10]);
  }
  return 0;
}
