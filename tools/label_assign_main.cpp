// Stand-alone driver of pemp_label_assign for sanitizer builds (no Python, no GPU work in the process).
//   label_assign_main DIR K
// reads, for k in [0, K): DIR/k.dims (int64 G, N), DIR/k.cost (f64 [G, N]), DIR/k.rows, DIR/k.cols (int64 [M], the
// expected nonzero assignment), as tools/label_assign_san.py writes them from tests/golden/labels_lsap_*.npz. Each
// matrix goes through the entry three times: as a same-type problem (method 4), as a same-type problem with the
// neighbour rule, and as a different-type problem (method 6), plus its transpose (rows above columns). Exit 0 when
// every returned assignment is the expected one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../include/pemp.h"

template <typename T>
static std::vector<T> slurp(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path.c_str());
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v(n / sizeof(T));
  if (n && fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}

// the assignment as (row of column n, or -1) from one call; diff: records carry another type (method 6's second solve)
static std::vector<int64_t> solve(const std::vector<double>& w, int G, int N, bool transpose, int method, int nb,
                                  bool diff) {
  const int R = transpose ? N : G, C = transpose ? G : N;
  std::vector<pemp_label_cand> recs;
  for (int g = 0; g < R; ++g)
    for (int n = 0; n < C; ++n) {
      const double v = transpose ? w[(size_t)n * N + g] : w[(size_t)g * N + n];
      if (v > 0) recs.push_back({g, (uint32_t)n | (diff ? 0u : 0x80000000u), v});
    }
  std::vector<int32_t> hdr = {(int32_t)recs.size(), R, 0}, tab(R);
  for (int g = 0; g < R; ++g) tab[g] = g;   // P = R people of J = 1 joint: person g
  const int64_t off[2] = {0, C};
  std::vector<float> labels(C), mask_node(C), class_mask(C);
  std::vector<int64_t> persons(C), classes(C);
  std::vector<uint8_t> amb(C);
  const int rc = pemp_label_assign(1, R, 1, hdr.data(), tab.data(), recs.data(), (int64_t)recs.size(), off, method, nb,
                                   0, 1e-9, 2.0, labels.data(), persons.data(), classes.data(), mask_node.data(),
                                   class_mask.data(), amb.data());
  if (rc != 0) {
    fprintf(stderr, "pemp_label_assign: %d %s\n", rc, pemp_last_error());
    exit(3);
  }
  return persons;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::string dir = argv[1];
  int bad = 0;
  for (int k = 0; k < atoi(argv[2]); ++k) {
    const std::string base = dir + "/" + std::to_string(k);
    const auto dims = slurp<int64_t>(base + ".dims");
    const auto w = slurp<double>(base + ".cost");
    const auto rows = slurp<int64_t>(base + ".rows"), cols = slurp<int64_t>(base + ".cols");
    const int G = (int)dims[0], N = (int)dims[1];
    if ((size_t)G * N != w.size() || rows.size() != cols.size()) return 2;
    std::vector<int64_t> want(N, -1), want_t(G, -1);
    for (size_t i = 0; i < rows.size(); ++i) want[cols[i]] = rows[i], want_t[rows[i]] = cols[i];
    const bool ok = solve(w, G, N, false, 4, 0, false) == want && solve(w, G, N, false, 4, 1, false) == want &&
                    solve(w, G, N, false, 6, 0, true) == want && solve(w, G, N, true, 4, 0, false) == want_t &&
                    solve(w, G, N, true, 6, 1, true) == want_t;
    printf("matrix %d: %d x %d, %zu pairs: %s\n", k, G, N, rows.size(), ok ? "ok" : "MISMATCH");
    bad += !ok;
  }
  return bad ? 1 : 0;
}
