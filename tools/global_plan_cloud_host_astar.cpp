// A host A* on the ground cloud over downloaded arrays, for tools/global_plan_bench.py --cloud: a RESTATEMENT of
// A_Star_on_Graph::getPath (a_star_on_pc.cpp:200-329) with isLineOfSightClear (:168-198) -- this tool's own code, NOT the
// reference: its searches are uniform grids instead of nanoflann's kd-trees, its containers the reference's
// (std::set<std::pair<float, unsigned>> as the frontier, std::unordered_map<unsigned, Node> as the list, Initial() clearing
// every node before each plan).  The lethal grid is built once, outside the timed plan (the reference builds its lethal
// kd-tree inside getPath).  Arithmetic: csrc/global_plan_cloud_plan.hip.h.  It reads one binary file
//   uint32 n, uint32 n_lethal, uint32 n_queries, double turning_weight, radius, inscribed, rate,
//   float xyz[n][3], double dgraph[n + 1], float lethal[n_lethal][3], uint32 start[n_queries], uint32 goal[n_queries]
// runs every query `reps` times and prints per query: path length, expansions, marched edges, p10 / median / p90 in us.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

#include "global_plan_cloud_plan.hip.h"

struct Node { unsigned self_index; float g, h, f; unsigned parent_index; bool is_closed, is_opened; };

static float l2(const float* a, const float* b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

struct Grid {                                 // dense uniform grid, cell-sorted ids
  float lo[3] = {0, 0, 0}, inv = 1;
  int n[3] = {1, 1, 1};
  std::vector<uint32_t> start, ids;
  const float* xyz = nullptr;
  int cell(float v, int a) const { return std::min(std::max((int)std::floor((v - lo[a]) * inv), 0), n[a] - 1); }
  void build(const float* pts, uint32_t count, float size) {
    xyz = pts;
    inv = 1.0f / size;
    float hi[3] = {0, 0, 0};
    for (uint32_t i = 0; i < count; ++i)
      for (int a = 0; a < 3; ++a) {
        lo[a] = i ? std::min(lo[a], pts[3 * (size_t)i + a]) : pts[a];
        hi[a] = i ? std::max(hi[a], pts[3 * (size_t)i + a]) : pts[a];
      }
    for (int a = 0; a < 3; ++a) n[a] = std::max(1, (int)std::ceil((hi[a] - lo[a]) * inv) + 1);
    start.assign((size_t)n[0] * n[1] * n[2] + 1, 0);
    std::vector<uint32_t> at(count);
    for (uint32_t i = 0; i < count; ++i) {
      at[i] = (uint32_t)((cell(pts[3 * (size_t)i + 2], 2) * n[1] + cell(pts[3 * (size_t)i + 1], 1)) * n[0] + cell(pts[3 * (size_t)i], 0));
      ++start[at[i] + 1];
    }
    for (size_t c = 1; c < start.size(); ++c) start[c] += start[c - 1];
    ids.resize(count);
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (uint32_t i = 0; i < count; ++i) ids[fill[at[i]]++] = i;
  }
  template <class F>
  void for_each(const float* q, float r, F&& f) const {   // every point of the cells the box touches; f returns true to stop
    const int x0 = cell(q[0] - r, 0), x1 = cell(q[0] + r, 0), y0 = cell(q[1] - r, 1), y1 = cell(q[1] + r, 1), z0 = cell(q[2] - r, 2), z1 = cell(q[2] + r, 2);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const size_t row = ((size_t)z * n[1] + y) * n[0];
        for (uint32_t k = start[row + x0]; k < start[row + x1 + 1]; ++k)
          if (f(ids[k])) return;
      }
  }
  bool covers(const float* q, float r) const {
    for (int a = 0; a < 3; ++a)
      if (cell(q[a] - r, a) != 0 || cell(q[a] + r, a) != n[a] - 1) return false;
    return true;
  }
};

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int reps = std::atoi(argv[2]);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0, nl = 0, nq = 0;
  double par[4];
  if (!rd(f, &n, 1) || !rd(f, &nl, 1) || !rd(f, &nq, 1) || !rd(f, par, 4)) return 2;
  std::vector<float> xyz(3 * (size_t)n), lethal(3 * (size_t)nl);
  std::vector<double> dgraph(n + 1);
  std::vector<uint32_t> start(nq), goal(nq);
  if (!rd(f, xyz.data(), xyz.size()) || !rd(f, dgraph.data(), n + 1) || !rd(f, lethal.data(), lethal.size()) || !rd(f, start.data(), nq) || !rd(f, goal.data(), nq))
    return 2;
  std::fclose(f);
  const double tw = par[0], radius = par[1], inscribed = par[2], rate = par[3];
  if (n < 8 || !(inscribed > 0)) return 2;
  const float r2 = dddmr::gp_cloud_radius2(radius), rf = (float)radius + 1e-3f;
  const float los_r2 = dddmr::gp_cloud_radius2(2.0 * inscribed), los_rf = (float)(2.0 * inscribed) + 1e-3f;
  Grid ground, leth;
  ground.build(xyz.data(), n, std::max(0.25f, 0.5f * rf));
  if (nl) leth.build(lethal.data(), nl, std::max(0.25f, los_rf));
  std::unordered_map<unsigned, Node> list;
  std::set<std::pair<float, unsigned>> frontier;
  std::vector<std::pair<float, unsigned>> succ;
  for (uint32_t q = 0; q < nq; ++q) {
    std::vector<double> us;
    size_t path_len = 0, expanded = 0, marched = 0;
    for (int r = 0; r < reps; ++r) {
      const auto t0 = std::chrono::steady_clock::now();
      const unsigned s = start[q], g = goal[q];
      const float* pg = &xyz[3 * (size_t)g];
      list.clear();
      for (uint32_t i = 0; i < n; ++i) list[i] = Node{0, 0, 0, 0, 0, false, false};   // Initial()
      frontier.clear();
      const float f0 = std::sqrt(l2(&xyz[3 * (size_t)s], pg));
      list[s] = Node{s, 0, 0, f0, s, false, true};
      frontier.insert({f0, s});
      std::vector<unsigned> path;
      expanded = marched = 0;
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
        succ.clear();
        ground.for_each(pc, rf, [&](uint32_t id) {
          const float d2 = l2(&xyz[3 * (size_t)id], pc);
          if (d2 < r2) succ.push_back({d2, id});
          return false;
        });
        if (succ.size() < dddmr::kGpCloudKnn) {              // the 8 nearest: boxes of doubling half width
          for (float h = 2.0f * rf;; h *= 2.0f) {
            const bool all = ground.covers(pc, h);
            const float d2_max = dddmr::gp_cloud_shell_d2(h);
            succ.clear();
            size_t inside = 0;
            ground.for_each(pc, h, [&](uint32_t id) {
              const float d2 = l2(&xyz[3 * (size_t)id], pc);
              succ.push_back({d2, id});
              inside += d2 <= d2_max;
              return false;
            });
            if (all || inside >= dddmr::kGpCloudKnn) break;
          }
          std::partial_sort(succ.begin(), succ.begin() + dddmr::kGpCloudKnn, succ.end());
          succ.resize(dddmr::kGpCloudKnn);
        } else {
          std::sort(succ.begin(), succ.end());
        }
        for (const auto& e : succ) {
          const unsigned nb = e.second;
          const double d = dgraph[nb];
          if (d < inscribed) continue;
          const float* pe = &xyz[3 * (size_t)nb];
          if (dddmr::gp_cloud_los_needed(e.first, inscribed)) {
            ++marched;
            const float dX = pe[0] - pc[0], dY = pe[1] - pc[1], dZ = pe[2] - pc[2];
            const float dt = dddmr::gp_cloud_los_dt(dX, dY, dZ, inscribed);
            bool clear = true;
            uint32_t k = 0;
            for (float t = 0.f; clear && dddmr::gp_cloud_los_goes_on(t, dt); t += dt) {
              if (++k > dddmr::kGpLosMaxSamples) { clear = false; break; }
              const float rr = dddmr::gp_cloud_los_r(t);
              const float sp[3] = {dddmr::gp_cloud_los_coord(pc[0], dX, rr), dddmr::gp_cloud_los_coord(pc[1], dY, rr), dddmr::gp_cloud_los_coord(pc[2], dZ, rr)};
              int cnt = 0;
              if (nl) leth.for_each(sp, los_rf, [&](uint32_t id) { cnt += l2(&lethal[3 * (size_t)id], sp) < los_r2; return cnt > 1; });
              if (cnt > 1) clear = false;
            }
            if (!clear) continue;
          }
          const double factor = dddmr::gp_factor(rate, d, inscribed);
          const double theta = dddmr::gp_theta(pp[0], pp[1], pc[0], pc[1], pe[0], pe[1]);
          const float new_g = dddmr::gp_cloud_new_g(cur.g, std::sqrt(e.first), factor, 0.f, theta, tw, 0.f);
          const float new_h = std::sqrt(l2(pe, pg));
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
    std::printf("Q %u %zu %zu %zu %.3f %.3f %.3f\n", q, path_len, expanded, marched, us[us.size() / 10], us[us.size() / 2], us[(9 * us.size()) / 10]);
  }
  return 0;
}
