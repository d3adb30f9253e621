// Every layout of allocnet_amd/csrc/workspace.h, carved in host memory: build with the host compiler and
// -fsanitize=address,undefined, run as an ordinary program (tests/test_workspace_layout_cpu.py does both).
// stdin: one shape per line, "<layout> <arguments...> <expected doubles>" -- the list and the recorded sizes of
// tests/golden/workspace_sizes.json, so the sizes are checked here without the library as well.  For each shape: allocate exactly
// the measured bytes (the sanitizer sees a write one byte past them), carve, fill every region with its own index over its full
// typed extent, then verify that every region still holds its index (no overlap), that every pointer is aligned for its type and
// that no region ends behind the total.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
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

struct Regions {
  struct R {
    std::string name;
    char *p;
    size_t bytes, align;
    std::function<void(int)> fill;
    std::function<bool(int)> holds;
  };
  std::vector<R> v;
  template <class T>
  void add(const char *name, T *p, int64_t count) {
    if (count == 0) return;
    v.push_back({name, (char *)p, sizeof(T) * (size_t)count, alignof(T),
                 [p, count](int k) { for (int64_t i = 0; i < count; ++i) p[i] = (T)k; },
                 [p, count](int k) { for (int64_t i = 0; i < count; ++i) if (p[i] != (T)k) return false; return true; }});
  }
  void add(const LbfgsLayout &L) {
    const int64_t v_ = (int64_t)L.n * L.ld;
    add("x", L.x, v_); add("g", L.g, v_); add("xp", L.xp, v_); add("gp", L.gp, v_); add("d", L.d, v_);
    add("lm_s", L.lm_s, L.m * v_); add("lm_y", L.lm_y, L.m * v_); add("lm_ys", L.lm_ys, L.m * L.ld);
    add("lm_alpha", L.lm_alpha, L.m * L.ld); add("pf", L.pf, L.npf * L.ld); add("ds", L.ds, DS_COUNT_ * L.ld);
    add("feval", L.feval, L.ld); add("is", L.is, IS_COUNT_ * L.ld);
  }
  void add(const ResumeTail &t, int64_t per, int64_t ld) {
    add("cont", t.cont, per * ld); add("score", t.score, ld); add("order", t.order, ld); add("bins", t.bins, kOrderBuckets);
  }
  void add(const CostGradWs &W, int s, int N, int64_t ld) {
    const int64_t nco = (int64_t)N * 3 * 2 * s;
    add("co", W.co, nco * ld); add("gdC", W.gdC, nco * ld); add("gdT", W.gdT, N * ld); add("pc", W.pc, N * ld); add("en", W.en, ld);
  }
};

// carve(base, regions) -> doubles; base == nullptr measures
template <class F>
static void check(const std::string &what, F &&carve, int64_t expected = -1) {
  ++g_checked;
  const int64_t total = carve(nullptr, nullptr);
  if (expected >= 0 && total != expected)
    return failure(what, "measures " + std::to_string(total) + " doubles, recorded " + std::to_string(expected));
  char *buf = (char *)malloc(total > 0 ? (size_t)total * 8 : 1);
  Regions r;
  if (carve((double *)buf, &r) != total) failure(what, "carving and measuring disagree");
  for (size_t i = 0; i < r.v.size(); ++i) {
    const Regions::R &q = r.v[i];
    if ((uintptr_t)q.p % q.align) failure(what, q.name + " is misaligned");
    if (q.p < buf || q.p + q.bytes > buf + total * 8) failure(what, q.name + " leaves the workspace");
    else q.fill((int)i + 1);
  }
  for (size_t i = 0; i < r.v.size(); ++i)
    if (!r.v[i].holds((int)i + 1)) failure(what, r.v[i].name + " was overwritten by another region");
  free(buf);
}

int main() {
  // the cursor itself, as the staging buffers of the host entry points use it: every region rounded up to whole doubles
  check("cursor: mixed element types", [&](double *w, Regions *r) {
    Cursor c(w);
    float *f = c.take<float>(3);
    uint64_t *u = c.take<uint64_t>(2);
    int32_t *i = c.take<int32_t>(5);
    char *b = c.take<char>(1);
    double *d = c.take<double>(1), *sp = c.spare(4);  // 4 + 4 + 7 bytes of rounding so far: two of the four doubles
    if (r) { r->add("float", f, 3); r->add("uint64", u, 2); r->add("int32", i, 5); r->add("char", b, 1); r->add("double", d, 1); r->add("spare", sp, 2); }
    return c.doubles();
  }, 2 + 2 + 3 + 1 + 1 + 2);
  std::string line;
  char lb[1 << 12];
  while (fgets(lb, sizeof lb, stdin)) {
    line = lb;
    std::istringstream in(line);
    std::string kind;
    std::vector<int64_t> a;
    in >> kind;
    for (int64_t x; in >> x;) a.push_back(x);
    if (kind.empty()) continue;
    const std::string what = line.substr(0, line.find('\n'));
    if (kind == "cost_grad" && a.size() == 4) {
      const int s = (int)a[0], N = (int)a[1];
      const int64_t ld = a[2];
      check(what, [&](double *w, Regions *r) { const CostGradWs W = cost_grad_ws(w, s, N, ld); if (r) r->add(W, s, N, ld); return W.doubles; }, a[3]);
    } else if (kind == "lbfgs" && a.size() == 5) {
      const int n = (int)a[0], m = (int)a[2], npf = a[3] > 1 ? (int)a[3] : 1;
      const int64_t ld = a[1];
      check(what, [&](double *w, Regions *r) { const LbfgsLayout L = lbfgs_layout(w, n, m, npf, ld); if (r) r->add(L); return L.doubles; }, a[4]);
      check(what + " (result rows)", [&](double *w, Regions *r) {
        const LbfgsResultRows R = lbfgs_result_rows(w, ld);
        if (r) { r->add("status", R.status, ld); r->add("iters", R.iters, ld); r->add("evals", R.evals, ld); }
        return R.doubles;
      });
    } else if (kind == "lbfgs_minco" && a.size() == 6) {
      const int s = (int)a[0], N = (int)a[1], m = (int)a[3], npf = a[4] > 1 ? (int)a[4] : 1, nw = 3 * (N - 1), nt = N;
      const int64_t ld = a[2];
      // the sizes were recorded with the default switches: the two-launch tail from 36 variables on (tuning.h)
      const bool with_tail = nw + nt >= 36;
      ptrdiff_t tail_at[3];
      const int runs[3] = {nw + nt, nw, nt};  // waypoints + durations, waypoints only, durations only
      for (int k = 0; k < 3; ++k) {
        if (runs[k] == 0) { tail_at[k] = tail_at[0]; continue; }  // (one piece has no waypoints)
        check(what + " run of " + std::to_string(runs[k]), [&](double *w, Regions *r) {
          const LbfgsMincoWs W = lbfgs_minco_ws(w, s, N, ld, m, npf, runs[k], with_tail);
          if (r) {
            r->add(W.opt); r->add(W.cg, s, N, ld); r->add("gP", W.gP, (int64_t)nw * ld); r->add("gT", W.gT, (int64_t)nt * ld);
            if (with_tail) r->add(W.tail, kPersistContDoubles, ld);
            tail_at[k] = with_tail ? (char *)W.tail.cont - (char *)w : 0;
            if (with_tail != (W.tail.cont != nullptr)) failure(what, "tail present / absent against with_tail");
          }
          return W.doubles;
        }, a[5]);
      }
      if (tail_at[1] != tail_at[0] || tail_at[2] != tail_at[0]) failure(what, "the tail moves with opt_flags");
    } else if (kind == "qp" && a.size() == 6) {
      const int s = (int)a[0], N = (int)a[1], res = (int)a[3], M = (int)a[4];
      const int64_t batch = a[2];
      check(what, [&](double *w, Regions *r) {
        const QpSolveWs W = qp_solve_ws(w, s, N, batch, res, M);
        if (r) {
          r->add("front", W.front, 2 * W.m * batch); r->add("residuals", W.residuals, 2 * batch);
          r->add(W.tail, qp_cont_doubles(s, N), batch);
          const QpSolveWs::View ad = W.admm(), ip = W.ipm();
          if (ad.z != W.front || ad.y != ad.z + W.m * batch || ad.y + W.m * batch != W.front + 2 * W.m * batch || ad.residuals != W.residuals)
            failure(what, "ADMM view does not tile the front");
          if (ip.z != W.front || ip.y != ip.z + W.mi * batch || ip.residuals != ip.y + W.mi * batch ||
              ip.residuals + 2 * batch > W.front + 2 * W.m * batch)
            failure(what, "interior-point view leaves the front");
        }
        return W.doubles;
      }, a[5]);
    } else if (kind == "firi" && a.size() == 5) {  // batch, max_points, max_rows, row stride, expected
      const int64_t batch = a[0], ld = a[3];
      const int Np = a[1] > 0 ? (int)a[1] : 1, H = (int)a[2];
      auto add_ws = [&](Regions *r, const FiriWs &W) {
        r->add("ell", W.ell, batch * kFiriEll); r->add("fpc", W.fpc, batch * Np * 4); r->add("A", W.A, (int64_t)3 * H * ld);
        r->add(W.opt); r->add("flag", W.flag, batch * Np); r->add("mok", W.mok, batch); r->add("np0", W.np0, batch);
      };
      check(what, [&](double *w, Regions *r) { const FiriWs W = firi_ws(w, batch, ld, Np, H); if (r) add_ws(r, W); return W.doubles; }, a[4]);
    } else {
      failure(what, "unknown layout or wrong argument count");
    }
  }
  printf("%ld layouts carved, %d failures\n", g_checked, g_failures);
  return g_failures || g_checked == 0 ? 1 : 0;
}
