// Training-label matching on the host (pemp_label_assign) — restates, on the sparse candidate list of
// pemp_label_candidates, the sequential half of
//   ConstructGraph.py:627-694   _construct_edge_labels_4
//   ConstructGraph.py:769-942   _construct_edge_labels_6 (its hard-coded method == 2, "semi agnostic")
// The reference solves two dense [G, N] assignments with scipy (linear_sum_assignment, maximize) and keeps the
// pairs of nonzero weight. Those pairs are a maximum-weight matching of the sparse bipartite graph of the nonzero
// entries, which falls into small connected components: each component is solved exactly as a dense rectangular
// assignment (shortest augmenting paths with potentials), zero standing for "no edge".
//
// Plain C++ without HIP: labels.hip includes it for the library, tools/label_assign_main.cpp for a sanitizer build.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <limits>
#include <numeric>
#include <vector>

#include "../../include/pemp.h"

namespace pemp {
namespace labels {

// Maximum-weight assignment of a dense r x c matrix w (row-major, entries >= 0), r <= c: col_of[i] for every row.
// Minimises -w by shortest augmenting paths (the classical O(r^2 c) Hungarian method with potentials).
inline void lsap_max_rows(const std::vector<double>& w, int r, int c, std::vector<int>& col_of) {
  const double INF = std::numeric_limits<double>::infinity();
  std::vector<double> u(r + 1, 0.0), v(c + 1, 0.0), minv(c + 1);
  std::vector<int> p(c + 1, 0), way(c + 1, 0);
  std::vector<char> used(c + 1);
  for (int i = 1; i <= r; ++i) {
    p[0] = i;
    int j0 = 0;
    std::fill(minv.begin(), minv.end(), INF);
    std::fill(used.begin(), used.end(), 0);
    do {
      used[j0] = 1;
      const int i0 = p[j0];
      double delta = INF;
      int j1 = 0;
      for (int j = 1; j <= c; ++j) {
        if (used[j]) continue;
        const double cur = -w[(size_t)(i0 - 1) * c + (j - 1)] - u[i0] - v[j];
        if (cur < minv[j]) {
          minv[j] = cur;
          way[j] = j0;
        }
        if (minv[j] < delta) {
          delta = minv[j];
          j1 = j;
        }
      }
      for (int j = 0; j <= c; ++j) {
        if (used[j]) {
          u[p[j]] += delta;
          v[j] -= delta;
        } else {
          minv[j] -= delta;
        }
      }
      j0 = j1;
    } while (p[j0] != 0);
    do {
      const int j1 = way[j0];
      p[j0] = p[j1];
      j0 = j1;
    } while (j0);
  }
  col_of.assign(r, -1);
  for (int j = 1; j <= c; ++j)
    if (p[j]) col_of[p[j] - 1] = j - 1;
}

struct Edge {
  int g, n;
  double w;
};

// Maximum-weight matching of the sparse bipartite graph `edges` (w > 0) between G rows and N columns:
// match[g] = column or -1. Connected components by union-find, each solved densely.
inline void sparse_match(const std::vector<Edge>& edges, int G, int N, std::vector<int>& match) {
  match.assign(G, -1);
  if (edges.empty()) return;
  std::vector<int> parent(G + N);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  };
  for (const Edge& e : edges) {
    const int a = find(e.g), b = find(G + e.n);
    if (a != b) parent[std::max(a, b)] = std::min(a, b);
  }
  // edges grouped by component (stable: the (g, n) order inside a component is kept)
  std::vector<int> order(edges.size());
  std::iota(order.begin(), order.end(), 0);
  std::vector<int> comp(edges.size());
  for (size_t i = 0; i < edges.size(); ++i) comp[i] = find(edges[i].g);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return comp[a] < comp[b]; });
  std::vector<int> rloc(G, -1), cloc(N, -1), rows, cols, col_of;
  std::vector<double> w;
  for (size_t s = 0; s < order.size();) {
    size_t t = s;
    while (t < order.size() && comp[order[t]] == comp[order[s]]) ++t;
    rows.clear();
    cols.clear();
    for (size_t i = s; i < t; ++i) {
      const Edge& e = edges[order[i]];
      if (rloc[e.g] < 0) {
        rloc[e.g] = (int)rows.size();
        rows.push_back(e.g);
      }
      if (cloc[e.n] < 0) {
        cloc[e.n] = (int)cols.size();
        cols.push_back(e.n);
      }
    }
    const int r = (int)rows.size(), c = (int)cols.size();
    if (t - s == 1) {
      match[rows[0]] = cols[0];
    } else if (r <= c) {
      w.assign((size_t)r * c, 0.0);
      for (size_t i = s; i < t; ++i) {
        const Edge& e = edges[order[i]];
        w[(size_t)rloc[e.g] * c + cloc[e.n]] = e.w;
      }
      lsap_max_rows(w, r, c, col_of);
      for (int i = 0; i < r; ++i)
        if (w[(size_t)i * c + col_of[i]] != 0.0) match[rows[i]] = cols[col_of[i]];
    } else {   // more rows than columns: the transposed problem
      w.assign((size_t)r * c, 0.0);
      for (size_t i = s; i < t; ++i) {
        const Edge& e = edges[order[i]];
        w[(size_t)cloc[e.n] * r + rloc[e.g]] = e.w;
      }
      lsap_max_rows(w, c, r, col_of);
      for (int j = 0; j < c; ++j)
        if (w[(size_t)j * r + col_of[j]] != 0.0) match[rows[col_of[j]]] = cols[j];
    }
    for (int g : rows) rloc[g] = -1;
    for (int n : cols) cloc[n] = -1;
    s = t;
  }
}

struct Params {
  int method;             // 4 or 6 (EDGE_LABEL_METHOD)
  int use_neighbours;     // USE_NEIGHBOURS
  int with_background;    // WITH_BACKGROUND (method 6)
  double matching_radius, inclusion_radius;
  int J;                  // joint types; the background class is J
};

// One image. cand[0, n_cand) in (g, n) order with image-local n in [0, N); gt_tab[g] = person * J + joint.
// Outputs are this image's [N] slices; node_classes / class_mask may be NULL (method 4). Returns false when a
// record is out of range.
inline bool assign_image(const pemp_label_cand* cand, int64_t n_cand, const int32_t* gt_tab, int G, int N,
                         const Params& p, float* node_labels, int64_t* node_persons, int64_t* node_classes,
                         float* label_mask_node, float* class_mask, uint8_t* ambiguous) {
  for (int n = 0; n < N; ++n) {
    node_labels[n] = 0.f;
    node_persons[n] = -1;
    if (node_classes) node_classes[n] = 0;
    label_mask_node[n] = 1.f;
    ambiguous[n] = 0;
  }
  std::vector<Edge> same, diff;
  for (int64_t i = 0; i < n_cand; ++i) {
    const int g = cand[i].g, n = (int)(cand[i].n & 0x7fffffffu);
    if (g < 0 || g >= G || n >= N) return false;
    if (!(cand[i].sim >= p.matching_radius) || cand[i].sim == 0.0) continue;
    ((cand[i].n >> 31) ? same : diff).push_back({g, n, cand[i].sim});
  }
  std::vector<int> col(G, -1), alt;
  sparse_match(same, G, N, col);
  if (p.method == 6) {
    sparse_match(diff, G, N, alt);
    for (int g = 0; g < G; ++g)
      if (col[g] < 0) col[g] = alt[g];   // the row rule (ConstructGraph.py:820-829)
  }
  std::vector<int> row_1(G, -1);   // matched rows renumbered in row order
  int M = 0;
  for (int g = 0; g < G; ++g)
    if (col[g] >= 0) row_1[g] = M++;
  auto write = [&](int g, int n) {   // in the reference's order: the last write of a column wins
    node_labels[n] = 1.f;
    node_persons[n] = gt_tab[g] / p.J;
    if (node_classes) node_classes[n] = gt_tab[g] % p.J;
  };
  for (int g = 0; g < G; ++g)
    if (col[g] >= 0) write(g, col[g]);
  if (p.use_neighbours) {
    std::vector<char> taken(N, 0);
    for (int g = 0; g < G; ++g)
      if (col[g] >= 0) taken[col[g]] = 1;
    auto second = [&](const pemp_label_cand& c) {
      if (!(c.sim >= p.inclusion_radius) || c.sim == 0.0) return false;
      if (p.method == 4 && (!(c.n >> 31) || !(c.sim >= p.matching_radius))) return false;
      return !taken[c.n & 0x7fffffffu];
    };
    std::vector<int> cnt(N, 0);
    for (int64_t i = 0; i < n_cand; ++i)
      if (second(cand[i])) ++cnt[cand[i].n & 0x7fffffffu];
    for (int n = 0; n < N; ++n) ambiguous[n] = cnt[n] > 1;
    for (int64_t i = 0; i < n_cand; ++i) {
      const int n = (int)(cand[i].n & 0x7fffffffu);
      if (second(cand[i]) && !ambiguous[n] && row_1[cand[i].g] >= 0) write(cand[i].g, n);
    }
    if (p.method == 6)
      for (int n = 0; n < N; ++n)
        if (ambiguous[n]) label_mask_node[n] = 0.f;
  }
  if (p.method == 6) {
    for (int n = 0; n < N; ++n) {
      if (class_mask) class_mask[n] = p.with_background ? 1.f : node_labels[n] * label_mask_node[n];
      if (p.with_background && node_classes && node_labels[n] != 1.f) node_classes[n] = p.J;
    }
  }
  return true;
}

}  // namespace labels
}  // namespace pemp
