// The three layouts allocnet_amd/csrc/workspace.h adds for the corridor-constrained MINCO L-BFGS (sfc_ws, sfc_overlap_ws,
// sfc_backward_p_ws), carved in host memory as tests/cpp/test_workspace_layout.cpp carves the others: build with the host compiler
// and -fsanitize=address,undefined, run as an ordinary program (tests/test_sfc_opt_cpu.py does both).
// stdin: one shape per line, "sfc s N K ld m npf expected", "sfc_overlap N B M K expected", "sfc_backward_p N K ld expected" --
// expected: what the library's anet_sfc_*workspace() returned for the shape.  For each: allocate exactly the measured bytes, carve,
// fill every region with its own index over its full typed extent, verify that every region still holds it, is aligned for its type
// and ends inside the total; for sfc also with the run of xi only (durations fixed), which must leave everything behind the
// optimiser's state in place.
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

template <class F>
static void check(const std::string &what, F &&carve, int64_t expected) {
  ++g_checked;
  const int64_t total = carve(nullptr, nullptr);
  if (total != expected) return failure(what, "measures " + std::to_string(total) + " doubles, the library says " + std::to_string(expected));
  char *buf = (char *)malloc(total > 0 ? (size_t)total * 8 : 1);
  Regions r;
  if (carve((double *)buf, &r) != total) failure(what, "carving and measuring disagree");
  bool inside = true;
  for (size_t i = 0; i < r.v.size(); ++i) {
    const Region &q = r.v[i];
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
    if (kind == "sfc" && a.size() == 7) {
      const int s = (int)a[0], N = (int)a[1], K = (int)a[2], m = (int)a[4], npf = a[5] > 1 ? (int)a[5] : 1;
      const int64_t ld = a[3];
      ptrdiff_t behind[2] = {0, 0};
      const int runs[2] = {(N - 1) * K + N, (N - 1) * K};
      for (int k = 0; k < 2; ++k)
        check(what + " run of " + std::to_string(runs[k]), [&](double *w, Regions *r) {
          const SfcWs W = sfc_ws(w, s, N, K, ld, m, npf, runs[k]);
          if (r) {
            const int64_t nco = (int64_t)N * 3 * 2 * s;
            r->add(W.opt);
            r->add("co", W.cg.co, nco * ld); r->add("gdC", W.cg.gdC, nco * ld); r->add("gdT", W.cg.gdT, N * ld);
            r->add("pc", W.cg.pc, N * ld); r->add("en", W.cg.en, ld);
            r->add("wps", W.wps, (int64_t)3 * (N - 1) * ld); r->add("gP", W.gP, (int64_t)3 * (N - 1) * ld);
            r->add("gT", W.gT, (int64_t)N * ld); r->add("norm", W.norm, (int64_t)3 * (N - 1) * ld);
            behind[k] = (char *)W.cg.co - (char *)w;
          }
          return W.doubles;
        }, a[6]);
      if (behind[0] != behind[1]) failure(what, "the regions behind the state move with opt_flags");
    } else if (kind == "sfc_overlap" && a.size() == 5) {
      const int N = (int)a[0], M = (int)a[2], K = (int)a[3];
      const int64_t B = a[1], P = (int64_t)(N - 1) * B;
      check(what, [&](double *w, Regions *r) {
        const SfcOverlapWs W = sfc_overlap_ws(w, N, B, M, K);
        if (r) { r->add("stacked", W.stacked, P * 2 * M * 4); r->add("verts", W.verts, P * K * 3); r->add("count", W.count, P); r->add("status", W.status, P); }
        return W.doubles;
      }, a[4]);
    } else if (kind == "sfc_backward_p" && a.size() == 4) {
      const int N = (int)a[0], K = (int)a[1];
      const int64_t ld = a[2];
      check(what, [&](double *w, Regions *r) {
        const LbfgsLayout L = sfc_backward_p_ws(w, N, K, ld);
        if (r) r->add(L);
        if (L.n != K || L.ld != (int64_t)(N - 1) * ld || L.m != kSfcTinyMem || L.npf != kSfcTinyPast) failure(what, "not the tiny problem's shape");
        return L.doubles;
      }, a[3]);
    } else {
      failure(what, "unknown layout or wrong argument count");
    }
  }
  printf("%ld layouts carved, %d failures\n", g_checked, g_failures);
  return g_failures || g_checked == 0 ? 1 : 0;
}
