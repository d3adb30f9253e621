// The layout allocnet_amd/csrc/workspace.h adds for the shortest route through a corridor (sfc_path_ws), carved in host memory as
// tests/cpp/test_sfc_workspace_layout.cpp carves its siblings: build with the host compiler and -fsanitize=address,undefined, run
// as an ordinary program (tests/test_sfc_path_cpu.py does both).
// stdin: one shape per line, "sfc_path N K ld m npf expected" -- expected: what the library's anet_sfc_shortest_path_workspace()
// returned for the shape.  For each: allocate exactly the measured bytes, carve, fill every region with its own index over its
// full typed extent, verify that every region still holds it, is aligned for its type and ends inside the total; the optimiser's
// rows must be those of lbfgs_layout for (N-1) K variables at the head of the workspace (the x rows first, the gradient rows next).
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../allocnet_amd/csrc/workspace.h"

using namespace anet;

static int g_failures = 0;
static long g_checked = 0;
static void failure(const std::string &what, const std::string &why) {
  if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what.c_str(), why.c_str());
}

struct Region { std::string name; char *p; size_t bytes, align; };
struct Regions {
  std::vector<Region> v;
  template <class T>
  void add(const char *name, T *p, int64_t count) {
    if (count > 0) v.push_back({name, (char *)p, sizeof(T) * (size_t)count, alignof(T)});
  }
  void add(const LbfgsLayout &L) {
    const int64_t n = (int64_t)L.n * L.ld;
    add("x", L.x, n); add("g", L.g, n); add("xp", L.xp, n); add("gp", L.gp, n); add("d", L.d, n);
    add("lm_s", L.lm_s, L.m * n); add("lm_y", L.lm_y, L.m * n); add("lm_ys", L.lm_ys, L.m * L.ld);
    add("lm_alpha", L.lm_alpha, L.m * L.ld); add("pf", L.pf, L.npf * L.ld); add("ds", L.ds, DS_COUNT_ * L.ld);
    add("feval", L.feval, L.ld); add("is", L.is, IS_COUNT_ * L.ld);
  }
};

int main() {
  char lb[1 << 10];
  while (fgets(lb, sizeof lb, stdin)) {
    std::istringstream in(lb);
    std::string kind;
    std::vector<int64_t> a;
    in >> kind;
    for (int64_t x; in >> x;) a.push_back(x);
    if (kind.empty()) continue;
    const std::string what = std::string(lb).substr(0, std::string(lb).find('\n'));
    if (kind != "sfc_path" || a.size() != 6) { failure(what, "unknown layout or wrong argument count"); continue; }
    ++g_checked;
    const int N = (int)a[0], K = (int)a[1], m = (int)a[3], npf = a[4] > 1 ? (int)a[4] : 1;
    const int64_t ld = a[2], total = sfc_path_ws(nullptr, N, K, ld, m, npf).doubles;
    if (total != a[5]) { failure(what, "measures " + std::to_string(total) + " doubles, the library says " + std::to_string(a[5])); continue; }
    char *buf = (char *)malloc(total > 0 ? (size_t)total * 8 : 1);
    const SfcPathWs W = sfc_path_ws((double *)buf, N, K, ld, m, npf);
    if (W.doubles != total) failure(what, "carving and measuring disagree");
    const int64_t n = (int64_t)(N - 1) * K;
    if (W.opt.n != n || W.opt.m != m || W.opt.npf != npf || W.opt.ld != ld) failure(what, "not the route's optimiser shape");
    if ((char *)W.opt.x != buf || W.opt.g != W.opt.x + n * ld) failure(what, "x and g are not the first rows of the workspace");
    Regions r;
    r.add(W.opt);
    r.add("norm", W.norm, (int64_t)3 * (N - 1) * ld);
    bool inside = true;
    for (const Region &q : r.v) {
      if ((uintptr_t)q.p % q.align) failure(what, q.name + " is misaligned");
      if (q.p < buf || q.p + q.bytes > buf + total * 8) { failure(what, q.name + " leaves the workspace"); inside = false; }
    }
    if (inside) {
      for (size_t i = 0; i < r.v.size(); ++i)
        for (size_t k = 0; k < r.v[i].bytes; ++k) r.v[i].p[k] = (char)(i + 1);
      for (size_t i = 0; i < r.v.size(); ++i)
        for (size_t k = 0; k < r.v[i].bytes; ++k)
          if (r.v[i].p[k] != (char)(i + 1)) { failure(what, r.v[i].name + " was overwritten by another region"); break; }
    }
    free(buf);
  }
  printf("%ld layouts carved, %d failures\n", g_checked, g_failures);
  return g_failures || g_checked == 0 ? 1 : 0;
}
