// The staging statements of the trajectory-major host entry points (allocnet_amd/csrc/staging.h), replayed in host memory: build
// with the host compiler and -fsanitize=address,undefined, run as an ordinary program (tests/test_staging_layout_cpu.py does
// both).  The transport is memcpy with a host transpose, and the "scratch" is a malloc of exactly the measured bytes, so the
// sanitizer sees a write one byte past them.  For every batch (with the library's row stride for it) and every distinct field
// sequence of every entry point over the shape list below:
//   * every region, the staging area included, lies inside the buffer, is aligned for its type and overlaps no other;
//   * every in() comes back through download() bit for bit, every shared() array lies on the "device" bit for bit;
//   * a single trajectory's inputs go out with one copy;
//   * a download() wider than the measured width is refused;
//   * the measured size is at most what the entry point's hand-written sums asked for before the statements replaced them (written
//     down here as plain arithmetic), and at least the bytes touched.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "../../allocnet_amd/csrc/staging.h"

using namespace anet;

static int g_failures = 0;
static long g_checked = 0;
static void failure(const std::string &what, const std::string &why) {
  if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s\n", what.c_str(), why.c_str());
}

struct MemTransport {
  char *buf = nullptr;
  int64_t buf_bytes = 0, touched = 0;  // touched: the furthest byte written or read in the buffer
  std::vector<double> pinned;
  int puts = 0, refused = 0;
  ~MemTransport() { free(buf); }
  void touch(const void *p, int64_t n_doubles) {
    const int64_t end = ((const char *)p - buf) + 8 * n_doubles;
    touched = std::max(touched, end);
  }
  int scratch(int64_t bytes, void **base) {
    free(buf);
    buf = (char *)malloc(bytes > 0 ? (size_t)bytes : 1);
    buf_bytes = bytes;
    *base = buf;
    return buf ? 0 : -2;
  }
  int pack(int64_t off, const double *host, int64_t nf) {
    if ((int64_t)pinned.size() < off + nf) pinned.resize((size_t)(off + nf));
    memcpy(pinned.data() + off, host, sizeof(double) * nf);
    return 0;
  }
  const double *packed() const { return pinned.data(); }
  int put(double *dev, const double *host, int64_t n) {
    ++puts;
    touch(dev, n);
    memcpy(dev, host, sizeof(double) * n);
    return 0;
  }
  int scatter(const double *host, int64_t batch, int64_t nf, int64_t ld, double *area, double *dev) {
    touch(area, batch * nf);
    touch(dev, (nf - 1) * ld + batch);
    memcpy(area, host, sizeof(double) * batch * nf);
    for (int64_t b = 0; b < batch; ++b)
      for (int64_t f = 0; f < nf; ++f) dev[f * ld + b] = area[b * nf + f];
    return 0;
  }
  int gather(const double *dev, int64_t batch, int64_t nf, int64_t ld, double *area, double *host) {
    touch(area, batch * nf);
    touch(dev, (nf - 1) * ld + batch);
    for (int64_t b = 0; b < batch; ++b)
      for (int64_t f = 0; f < nf; ++f) area[b * nf + f] = dev[f * ld + b];
    memcpy(host, area, sizeof(double) * batch * nf);
    return 0;
  }
  int fetch(const double *dev, int64_t n, double *host) {
    touch(dev, n);
    memcpy(host, dev, sizeof(double) * n);
    return 0;
  }
  int refuse(const char *) { ++refused; return -1; }
};
using Stage = Staging<MemTransport>;

// what a statement took, in order
struct Field {
  char kind;  // i in, o out, r rows, w workspace in doubles, s shared
  int64_t n;  // fields, rows or doubles
  char *p;
  int64_t bytes, align;
  std::vector<double> host;  // the input of an in / shared
};

// the takers of Stage::Pass, recorded; inputs are made up on the live pass (the measuring pass must not read them)
struct Rec {
  Stage::Pass &p;
  std::vector<Field> &log;
  std::string &key;
  int64_t batch, ld;
  std::vector<double> &make(int64_t n) {
    static uint64_t seed = 0x9e3779b97f4a7c15ull;
    log.emplace_back();
    std::vector<double> &h = log.back().host;
    h.resize((size_t)n);
    for (double &x : h) {
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      x = (double)(int64_t)(seed >> 11) * 0x1p-40;  // distinct finite bit patterns
    }
    return h;
  }
  void note(char kind, int64_t n, void *dev, int64_t bytes, int64_t align, bool made = false) {
    key += kind + std::to_string(n) + " ";
    if (!p.c.base) return;
    if (!made) log.emplace_back();
    Field &f = log.back();
    f.kind = kind; f.n = n; f.p = (char *)dev; f.bytes = bytes; f.align = align;
  }
  void in(int64_t nf, double **dev) {
    if (!p.c.base) p.in(nullptr, nf, dev);
    else p.in(make(batch * nf).data(), nf, dev);
    note('i', nf, *dev, 8 * nf * ld, 8, true);
  }
  void out(int64_t nf, double **dev) { p.out(nf, dev); note('o', nf, *dev, 8 * nf * ld, 8); }
  template <class T>
  void rows(int64_t n, T **dev) { p.rows(n, dev); note(sizeof(T) == 4 ? 'j' : 'r', n, *dev, (int64_t)sizeof(T) * n * ld, alignof(T)); }
  void doubles(int64_t w, double **dev) { p.doubles(w, dev); note('w', w, *dev, 8 * w, 8); }
  void shared(int64_t n, double **dev) {
    if (!p.c.base) p.shared(nullptr, n, dev);
    else p.shared(make(n).data(), n, dev);
    note('s', n, *dev, 8 * n, 8, true);
  }
  void result_rows() {
    const LbfgsResultRows R = lbfgs_result_rows(p.c, ld);
    note('j', 1, R.status, 4 * ld, 4); note('j', 1, R.iters, 4 * ld, 4); note('j', 1, R.evals, 4 * ld, 4);
  }
  void layout(const LbfgsLayout &L) { note('w', L.doubles, L.x, 8 * L.doubles, 8); }
};

struct Shape {
  int s, c, N, M, nq, K;
  unsigned opt;  // bit k: the k-th optional input of the entry point is present
  int64_t nco() const { return (int64_t)N * 3 * 2 * s; }
  int64_t nhp() const { return (int64_t)N * M * 4; }
  bool has(int k) const { return opt >> k & 1; }
};
constexpr int kMem = 8, kPast = 1;  // L-BFGS history and past costs of the replayed workspaces
static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int64_t result_rows_of(int64_t ld) { return ceil_div(lbfgs_result_rows(nullptr, ld).doubles, ld); }
static int64_t max3(int64_t a, int64_t b, int64_t c) { return std::max(a, std::max(b, c)); }
static int64_t sfc_wmax(const Shape &h, int64_t batch, int64_t ld) {
  return max3(sfc_ws(nullptr, h.s, h.N, h.K, ld, kMem, kPast, (h.N - 1) * h.K + h.N).doubles,
              sfc_overlap_ws(nullptr, h.N, batch, h.M, h.K).doubles, sfc_backward_p_ws(nullptr, h.N, h.K, ld).doubles);
}
static int64_t lbfgs_minco_w(const Shape &h, int64_t ld) {
  return lbfgs_minco_ws(nullptr, h.s, h.N, ld, kMem, kPast, 3 * (h.N - 1) + h.N, true).doubles;
}

// One entry point: its statement, the scratch its hand-written sums asked for (doubles: batch * max_field + total_fields * ld),
// the number of optional inputs, and whether the shape applies.
struct Site {
  const char *name;
  void (*statement)(Rec &, const Shape &);
  int64_t (*parent)(const Shape &, int64_t batch, int64_t ld);
  int optionals;
  bool (*applies)(const Shape &);
};
static bool always(const Shape &) { return true; }
static void boundary(Rec &p, const Shape &h) {  // head, tail, waypoints, durations
  double *d;
  p.in(3 * h.c, &d); p.in(3 * h.c, &d); p.in(3 * (int64_t)(h.N - 1), &d); p.in(h.N, &d);
}
static void coeffs_T(Rec &p, const Shape &h) {
  double *d;
  p.in(h.nco(), &d); p.in(h.N, &d);
}

static const Site kSites[] = {
    {"anet_minco_solve",
     [](Rec &p, const Shape &h) { double *d; boundary(p, h); p.out(h.nco(), &d); p.rows(1, &d); },
     [](const Shape &h, int64_t batch, int64_t ld) {
       const int64_t n_in = 6 * h.c + 3 * (h.N - 1) + h.N, n_co = h.nco();
       return batch * std::max(n_in, n_co) + (n_in + n_co + 1) * ld;
     }, 0, always},
    {"anet_minco_sample_costs",
     [](Rec &p, const Shape &h) {
       double *d;
       p.in(h.N, &d); p.rows(1, &d); p.shared(3 * h.c, &d); p.shared(3 * h.c, &d); p.shared(3 * (int64_t)(h.N - 1), &d);
     },
     [](const Shape &h, int64_t batch, int64_t ld) {
       const int64_t npb = 6 * h.c + 3 * (h.N - 1);
       return batch * h.N + (h.N + 1 + ceil_div(npb, batch) + 1) * ld;
     }, 0, always},
    {"anet_traj_eval",
     [](Rec &p, const Shape &h) { double *d; coeffs_T(p, h); p.in(h.nq, &d); p.out(3 * (int64_t)h.nq, &d); },
     [](const Shape &h, int64_t batch, int64_t ld) {
       return batch * std::max(h.nco(), (int64_t)3 * h.nq) + (h.nco() + h.N + h.nq + 3 * h.nq) * ld;
     }, 0, always},
    {"anet_traj_cost",
     [](Rec &p, const Shape &h) { double *d; coeffs_T(p, h); p.rows(1, &d); },
     [](const Shape &h, int64_t batch, int64_t ld) { return batch * h.nco() + (h.nco() + h.N + 1) * ld; }, 0, always},
    {"anet_traj_cost_grad_T",
     [](Rec &p, const Shape &h) { double *d; coeffs_T(p, h); p.out(h.N, &d); },
     [](const Shape &h, int64_t batch, int64_t ld) { return batch * h.nco() + (h.nco() + 2 * h.N) * ld; }, 0, always},
    {"anet_traj_max_rate",
     [](Rec &p, const Shape &h) { double *d; coeffs_T(p, h); p.out(h.N, &d); },
     [](const Shape &h, int64_t batch, int64_t ld) { return batch * h.nco() + (h.nco() + 2 * h.N) * ld; }, 0, always},
    {"anet_minco_cost_grad",  // optional: hpolys
     [](Rec &p, const Shape &h) {
       double *d;
       boundary(p, h);
       if (h.has(0) && h.nhp()) p.in(h.nhp(), &d);
       p.rows(1, &d); p.out(3 * (int64_t)(h.N - 1), &d); p.out(h.N, &d); p.out(h.nco(), &d);
       p.doubles(cost_grad_ws(nullptr, h.s, h.N, p.ld).doubles, &d);
     },
     [](const Shape &h, int64_t batch, int64_t ld) {
       const int64_t nhp = h.has(0) ? h.nhp() : 0, n_in = 6 * h.c + 3 * (h.N - 1) + h.N + nhp, n_out = 1 + 3 * (h.N - 1) + h.N + h.nco();
       return batch * max3(h.nco(), nhp, 3 * h.c) + (n_in + n_out + cost_grad_ws(nullptr, h.s, h.N, 1).doubles) * ld;
     }, 1, always},
    {"anet_lbfgs_mvie",
     [](Rec &p, const Shape &h) {
       double *d;
       p.in(3 * (int64_t)h.M, &d); p.in(9, &d);
       p.layout(lbfgs_layout(p.p.c, 9, kMem, kPast, p.ld));
       p.result_rows();
     },
     [](const Shape &h, int64_t batch, int64_t ld) {
       return batch * std::max((int64_t)3 * h.M, (int64_t)9) +
              (3 * h.M + 9 + lbfgs_layout(nullptr, 9, kMem, kPast, 1).doubles + result_rows_of(ld)) * ld;
     }, 0, [](const Shape &h) { return h.M >= 1; }},
    {"anet_lbfgs_minco",  // optional: hpolys
     [](Rec &p, const Shape &h) {
       double *d;
       boundary(p, h);
       if (h.has(0) && h.nhp()) p.in(h.nhp(), &d);
       p.out(h.nco(), &d); p.doubles(lbfgs_minco_w(h, p.ld), &d); p.rows(1, &d);
       p.result_rows();
     },
     [](const Shape &h, int64_t batch, int64_t ld) {
       const int64_t nhp = h.has(0) ? h.nhp() : 0;
       return batch * max3(h.nco(), nhp, 3 * h.c) +
              (6 * h.c + 3 * (h.N - 1) + h.N + nhp + h.nco() + ceil_div(lbfgs_minco_w(h, ld), ld) + 1 + result_rows_of(ld)) * ld;
     }, 1, always},
    {"anet_flat_forward",  // optional: psi, dpsi
     [](Rec &p, const Shape &h) {
       double *d;
       p.in(3, &d); p.in(3, &d); p.in(3, &d);
       if (h.has(0)) p.in(1, &d);
       if (h.has(1)) p.in(1, &d);
       p.out(1, &d); p.out(4, &d); p.out(3, &d);
     },
     [](const Shape &, int64_t batch, int64_t ld) { return batch * 4 + (11 + 8) * ld; }, 2, always},
    {"anet_flat_backward",  // optional: psi, dpsi, pos_grad, vel_grad
     [](Rec &p, const Shape &h) {
       double *d;
       p.in(3, &d); p.in(3, &d); p.in(3, &d);
       if (h.has(0)) p.in(1, &d);
       if (h.has(1)) p.in(1, &d);
       if (h.has(2)) p.in(3, &d);
       if (h.has(3)) p.in(3, &d);
       p.in(1, &d); p.in(4, &d); p.in(3, &d);
       p.out(3, &d); p.out(3, &d); p.out(3, &d); p.out(3, &d); p.out(1, &d); p.out(1, &d);
     },
     [](const Shape &, int64_t batch, int64_t ld) { return batch * 4 + (11 + 14 + 14) * ld; }, 4, always},
    {"anet_traj_flat_states",
     [](Rec &p, const Shape &h) { double *d; coeffs_T(p, h); p.in(h.nq, &d); p.out((int64_t)h.nq * 11, &d); },
     [](const Shape &h, int64_t batch, int64_t ld) {
       const int64_t nout = (int64_t)h.nq * 11;
       return batch * std::max(h.nco(), nout) + (h.nco() + h.N + h.nq + nout) * ld;
     }, 0, always},
    {"anet_traj_flat_extrema",
     [](Rec &p, const Shape &h) { double *d; coeffs_T(p, h); p.out(4, &d); },
     [](const Shape &h, int64_t batch, int64_t ld) { return batch * h.nco() + (h.nco() + h.N + 4) * ld; }, 0, always},
    {"anet_lbfgs_minco_sfc",  // optional: wps_start
     [](Rec &p, const Shape &h) {
       double *d;
       int32_t *i;
       const int64_t nwp = 3 * (int64_t)(h.N - 1), nxi = (int64_t)(h.N - 1) * h.K;
       p.in(3 * h.c, &d); p.in(3 * h.c, &d);
       if (h.has(0)) p.in(nwp, &d);
       p.in(h.N, &d); p.in(h.nhp(), &d);
       p.out(nxi, &d); p.rows(3 * nxi, &d);
       p.rows(h.N - 1, &i); p.rows(h.N - 1, &i); p.out(h.N - 1, &d);
       p.out(nwp, &d); p.out(h.nco(), &d); p.rows(1, &d); p.doubles(sfc_wmax(h, p.batch, p.ld), &d);
       p.result_rows();
       p.p.at_least(h.N - 1);
     },
     [](const Shape &h, int64_t batch, int64_t ld) {
       const int64_t nwp = 3 * (int64_t)(h.N - 1), nxi = (int64_t)(h.N - 1) * h.K;
       const int64_t mx = std::max(max3(h.nco(), h.nhp(), nxi), (int64_t)3 * h.c);
       return batch * mx + (6 * h.c + nwp + h.N + h.nhp() + nxi + 3 * nxi + 3 * (h.N - 1) + nwp + h.nco() + 1 +
                            ceil_div(sfc_wmax(h, batch, ld), ld) + result_rows_of(ld)) * ld;
     }, 1, [](const Shape &h) { return h.N >= 2 && h.M >= 1; }},
};

static void replay(const Site &site, const Shape &h, int64_t batch, int64_t ld, std::set<std::string> &seen) {
  Stage st{{}, batch, ld};
  std::vector<Field> log;
  log.reserve(64);  // (the statement keeps references into it)
  std::string key, live_key;
  const int rc = st.stage([&](Stage::Pass &p) {
    Rec r{p, log, p.c.base ? live_key : key, batch, ld};
    site.statement(r, h);
  });
  if (!seen.insert(key).second) return;  // the same sequence under another shape
  ++g_checked;
  const std::string what = std::string(site.name) + " batch " + std::to_string(batch) + ": " + key;
  if (rc) return failure(what, "stage() failed");
  if (key != live_key) failure(what, "the two passes took different fields");
  MemTransport &tr = st.tr;
  if (st.bytes != tr.buf_bytes) failure(what, "the scratch is not the measured size");
  const int64_t parent = 8 * site.parent(h, batch, ld);
  if (st.bytes > parent) failure(what, "asks for " + std::to_string(st.bytes) + " bytes, the hand-written sum for " + std::to_string(parent));
  // every input is where it belongs
  int64_t widest = 0, ins = 0, shareds = 0;
  for (const Field &f : log) {
    if (f.kind == 'i' || f.kind == 'o') widest = std::max(widest, f.n);
    if (f.kind == 'i' && f.n) {
      ++ins;
      std::vector<double> back((size_t)(batch * f.n));
      if (st.download((double *)f.p, f.n, back.data())) failure(what, "download of an input refused");
      else if (memcmp(back.data(), f.host.data(), 8 * back.size())) failure(what, "an input does not round-trip");
    }
    if (f.kind == 's' && f.n) {
      ++shareds;
      if (memcmp(f.p, f.host.data(), 8 * (size_t)f.n)) failure(what, "a shared array is not on the device");
    }
  }
  if (st.width < widest) failure(what, "staging width below the widest field");
  if (batch == 1 && tr.puts != (ins ? 1 : 0) + shareds) failure(what, "a single trajectory's inputs did not go out with one copy");
  // a download wider than the staging area is refused, and touches nothing
  {
    const int64_t before = tr.touched;
    double sink = 0.0;
    if (!st.download((double *)log.front().p, st.width + 1, &sink) || tr.refused != 1 || tr.touched != before)
      failure(what, "a download wider than the staging width was not refused");
  }
  if (tr.touched > st.bytes) failure(what, "touched bytes behind the measured size");
  // the regions: inside the buffer, aligned, disjoint
  log.emplace_back();
  log.back().kind = 'a'; log.back().p = (char *)st.area; log.back().bytes = 8 * batch * st.width; log.back().align = 8;
  for (size_t i = 0; i < log.size(); ++i) {
    const Field &f = log[i];
    if (f.bytes == 0) continue;
    if ((uintptr_t)f.p % (uintptr_t)f.align) failure(what, "field " + std::to_string(i) + " is misaligned");
    if (f.p < tr.buf || f.p + f.bytes > tr.buf + st.bytes) failure(what, "field " + std::to_string(i) + " leaves the buffer");
    else memset(f.p, (int)i + 1, (size_t)f.bytes);
  }
  for (size_t i = 0; i < log.size(); ++i)
    for (int64_t k = 0; k < log[i].bytes; ++k)
      if ((unsigned char)log[i].p[k] != (unsigned char)(i + 1)) { failure(what, "field " + std::to_string(i) + " was overwritten by another"); break; }
}

int main() {
  const int64_t batches[6][2] = {{1, 1}, {2, 64}, {3, 64}, {64, 64}, {65, 128}, {512, 1088}};  // batch, the library's row stride for it
  for (const auto &bl : batches)
    for (const Site &site : kSites) {
      std::set<std::string> seen;
      for (int s : {2, 4}) for (int c : {1, s}) for (int N : {1, 2, 5}) for (int M : {0, 3}) for (int nq : {1, 7}) for (int K : {1, 4})
        for (unsigned opt = 0; opt < 1u << site.optionals; ++opt) {
          const Shape h{s, c, N, M, nq, K, opt};
          if (site.applies(h)) replay(site, h, bl[0], bl[1], seen);
        }
    }
  printf("%ld statements replayed, %d failures\n", g_checked, g_failures);
  return g_failures || g_checked == 0 ? 1 : 0;
}
