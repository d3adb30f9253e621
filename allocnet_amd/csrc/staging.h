// The staging buffer of a host (trajectory-major) entry point, written ONCE per entry point as a statement over a Pass:
//   Stager st(ctx, batch);
//   rc = st.stage([&](Stager::Pass &p) { p.in(head, 3 * c, &d_head); ... p.out(nco, &d_co); p.rows(1, &d_en); });
// stage() runs the statement twice, as workspace.h's layouts run: on a null base to measure, then on the scratch to set the
// pointers and send the inputs.  The buffer is a staging area of batch * width doubles (the trajectory-major side of every
// transpose; width: the widest field of any in / out) followed by the batch-minor rows in the order of the statement, row stride
// ld.  One trajectory: ld = 1, both layouts coincide, and the inputs are packed into one pinned buffer that goes out with ONE
// copy when the statement ends.  No call site sums fields or names a width.
// Host C++17 only, no HIP include, no device code: the copies and transposes are the Transport's (api_internal.h: HIP;
// tests/cpp/test_staging_layout.cpp: memcpy under a sanitizer).  A Transport has
//   scratch(bytes, &base)  a buffer of at least bytes       pack(off, host, nf)  host -> the pinned pack at off; packed(): the pack
//   put(dev, host, n)      contiguous host -> device        fetch(dev, n, host)  contiguous device -> host, finished on return
//   scatter(host, batch, nf, ld, area, dev)   host [batch][nf] -> area -> dev [nf][ld]
//   gather(dev, batch, nf, ld, area, host)    dev [nf][ld] -> area -> host [batch][nf], finished on return
//   refuse(why)            the error code of an invalid request
// each returning 0 or an error code that stage() / download() pass on.  DESIGN.md section 8i.
#pragma once
#include "workspace.h"

namespace anet {

template <class Transport>
struct Staging {
  Transport tr;
  int64_t batch, ld;
  int64_t width = 0, bytes = 0;  // measured by stage(): the staging width in fields, the whole buffer
  double *area = nullptr;        // batch * width doubles at the head of the buffer

  struct Pass {
    Staging &s;
    Cursor c;  // over the rows; a workspace.h layout may carve from it directly
    int64_t width = 0, packed = 0;
    double *pack_base = nullptr;
    int rc = 0;
    Pass(Staging &s_, void *rows) : s(s_), c(rows) {}
    bool live() const { return c.base && !rc; }
    // nf rows that come from the host array [batch][nf] (nf == 0: no rows, host may be NULL)
    void in(const double *host, int64_t nf, double **dev) {
      out(nf, dev);
      if (!live() || nf == 0) return;
      if (s.batch > 1) { rc = s.tr.scatter(host, s.batch, nf, s.ld, s.area, *dev); return; }
      if (!pack_base) pack_base = *dev;
      const int64_t off = *dev - pack_base;
      if (!(rc = s.tr.pack(off, host, nf))) packed = off + nf;
    }
    // nf rows that will go back through download(): they count towards the staging width
    void out(int64_t nf, double **dev) { at_least(nf); rows(nf, dev); }
    // n device-only rows of T (or rows copied back contiguously); int32 rows are packed, two elements per double
    template <class T> void rows(int64_t n, T **dev) { *dev = c.take<T>(n * s.ld); }
    // a workspace given in doubles, in whole rows
    void doubles(int64_t w, double **dev) { rows((w + s.ld - 1) / s.ld, dev); }
    // n doubles shared by the whole batch, copied contiguously (behind the packed inputs so far)
    void shared(const double *host, int64_t n, double **dev) {
      *dev = c.take<double>(n);
      flush();
      if (live() && n) rc = s.tr.put(*dev, host, n);
    }
    // the staging area must hold batch * nf doubles for a use of its own
    void at_least(int64_t nf) { width = nf > width ? nf : width; }
    // send the packed single-trajectory inputs (no-op otherwise)
    void flush() { if (live() && packed) rc = s.tr.put(pack_base, s.tr.packed(), packed); packed = 0; }
  };

  template <class Statement>
  int stage(Statement &&statement) {
    Pass measure(*this, nullptr);
    statement(measure);
    width = measure.width;
    bytes = (int64_t)sizeof(double) * batch * width + measure.c.bytes;
    void *base = nullptr;
    if (int rc = tr.scratch(bytes, &base)) return rc;
    area = (double *)base;
    Pass carve(*this, area + batch * width);
    statement(carve);
    carve.flush();
    if (!carve.rc && (carve.width != width || carve.c.bytes != measure.c.bytes)) return tr.refuse("staging statement differs between its two passes");
    return carve.rc;
  }

  // rows [nf][ld] on the device -> host [batch][nf]; the stream is idle on return
  int download(const double *dev, int64_t nf, double *host) {
    if (nf > width) return tr.refuse("download wider than the staging width of its statement");
    return batch == 1 ? tr.fetch(dev, nf, host) : tr.gather(dev, batch, nf, ld, area, host);
  }
};

}  // namespace anet
