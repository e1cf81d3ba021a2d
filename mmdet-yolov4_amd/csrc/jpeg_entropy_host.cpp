// Host side of the device Huffman decode (include/yv4.h, "the Huffman scan on the device"): the segment table, the
// packed Huffman tables and the workgroup table of a batch, their validation, and the CPU run of the shared decode
// (jpeg_entropy_core.h).  No HIP call: plain C++, usable without a GPU, and compiled on its own with sanitizers by
// tools/jpeg_entropy_sanitize.cpp.
//
// The bytes are untrusted.  yv4_jpeg_parse has checked every header segment's length against the file before the
// table pass below walks the same segments; the marker walk reads below len only.
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include "yv4.h"
#include "jpeg_entropy_core.h"

namespace yv4 {
void set_error(const char* fmt, ...);
int jpeg_entropy_validate(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_wg* wgs, int N,
                          int64_t nseg, int64_t nwg, int64_t bytes_len, int64_t nhuff, int64_t coef_elems,
                          int64_t* coef_lo, int64_t* coef_hi);
}

namespace {

#define JPEG_FAIL(code, ...)        \
  do {                              \
    ::yv4::set_error(__VA_ARGS__);  \
    return (code);                  \
  } while (0)

// One DHT table (16 counts, then the values) into the packed form.  jpeg_host.cpp's build_huff has accepted the counts.
void pack_huff(yv4_jpeg_huff& h, const uint8_t* counts, const uint8_t* vals, int nvals) {
  memset(&h, 0, sizeof(h));
  memcpy(h.vals, vals, (size_t)nvals);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = counts[l - 1];
    if (l <= 9) {
      for (int i = 0; i < n; ++i) {
        const int first = (code + i) << (9 - l);
        for (int j = 0; j < (1 << (9 - l)); ++j) h.look[first + j] = (uint16_t)((l << 8) | h.vals[k + i]);
      }
    } else {
      h.maxcode[l - 10] = n ? code + n - 1 : -1;
      h.valoff[l - 10] = k - code;
    }
    code = (code + n) << 1;
    k += n;
  }
  h.maxcode[7] = -1;
}

// The DHT segments in front of the scan: the last definition of each (class, slot) as a pointer to its counts.  The
// header segments were validated by yv4_jpeg_parse (which returned YV4_OK for these bytes); every step is checked
// against scan_offset all the same.
void find_tables(const uint8_t* d, size_t scan_offset, const uint8_t* found[2][4]) {
  memset(found, 0, sizeof(const uint8_t*) * 8);
  size_t pos = 2;
  while (pos + 4 <= scan_offset) {
    if (d[pos] != 0xFF) return;
    size_t q = pos + 1;
    while (q < scan_offset && d[q] == 0xFF) ++q;      // fill bytes
    if (q + 3 > scan_offset) return;
    const unsigned m = d[q];
    const size_t seglen = ((size_t)d[q + 1] << 8) | d[q + 2];
    const size_t body = q + 3, next = q + 1 + seglen;
    if (seglen < 2 || next > scan_offset) return;
    if (m == 0xC4) {
      size_t p = body;
      while (p + 17 <= next) {
        const unsigned tc = d[p] >> 4, th = d[p] & 15;
        int nvals = 0;
        for (int i = 0; i < 16; ++i) nvals += d[p + 1 + i];
        if (tc > 1 || th > 3 || nvals > 256 || p + 17 + (size_t)nvals > next) return;
        found[tc][th] = d + p + 1;
        p += 17 + (size_t)nvals;
      }
    }
    if (m == 0xDA) return;
    pos = next;
  }
}

const uint8_t kZigzag[64] = YV4_JPEG_ZIGZAG;

int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace

extern "C" int yv4_jpeg_scan_prepare(const uint8_t* data, size_t len, yv4_jpeg_info* info, yv4_jpeg_scan* scan,
                                     yv4_jpeg_huff* huff, yv4_jpeg_segment* segs, int64_t seg_capacity) {
  if (!data || !info || !scan || !huff || !segs) JPEG_FAIL(YV4_E_INVALID, "jpeg_scan_prepare: null pointer");
  const int st = yv4_jpeg_parse(data, len, info);
  if (st != YV4_OK) return st;
  memset(scan, 0, sizeof(*scan));
  const int64_t total = (int64_t)info->mcus_x * info->mcus_y;
  const int64_t ri = info->restart_interval;
  const int64_t nseg = ri ? ceil_div64(total, ri) : 1;
  if (nseg > 0x7fffffff) JPEG_FAIL(YV4_E_INVALID, "jpeg_scan_prepare: %lld segments", (long long)nseg);
  scan->data_len = (int64_t)len;
  scan->ncoef = info->ncoef;
  scan->nseg = (int32_t)nseg;
  scan->ncomp = info->ncomp;
  scan->mcus_x = info->mcus_x; scan->mcus_y = info->mcus_y;
  scan->hs = info->hs[0]; scan->vs = info->vs[0];
  if (seg_capacity < nseg) {
    ::yv4::set_error("jpeg_scan_prepare: %lld segments, room for %lld", (long long)nseg, (long long)seg_capacity);
    return YV4_E_CAPACITY;
  }

  // the tables the scan references, each packed once
  const uint8_t* found[2][4];
  find_tables(data, (size_t)info->scan_offset, found);
  int slot[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
  int nhuff = 0;
  for (int i = 0; i < info->ncomp; ++i)
    for (int cls = 0; cls < 2; ++cls) {
      const int id = cls ? info->ta[i] : info->td[i];
      if (!found[cls][id]) JPEG_FAIL(YV4_E_INVALID, "jpeg_scan_prepare: Huffman table %d of class %d is missing", id, cls);
      if (slot[cls][id] < 0) {
        const uint8_t* counts = found[cls][id];
        int nvals = 0;
        for (int k = 0; k < 16; ++k) nvals += counts[k];
        pack_huff(huff[nhuff], counts, counts + 16, nvals);
        slot[cls][id] = nhuff++;
      }
      (cls ? scan->ta : scan->td)[i] = slot[cls][id];
    }
  scan->nhuff = nhuff;

  // the marker walk: a segment ends where the bit reader stops, at the first 0xFF that no 0x00 follows, or at the end
  size_t pos = (size_t)info->scan_offset;
  int rst = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    yv4_jpeg_segment& g = segs[s];
    memset(&g, 0, sizeof(g));
    g.begin = (int64_t)pos;
    size_t p = pos;
    for (;;) {
      const uint8_t* f = p < len ? (const uint8_t*)memchr(data + p, 0xFF, len - p) : nullptr;
      if (!f) { p = len; break; }
      p = (size_t)(f - data);
      if (p + 1 < len && data[p + 1] == 0) p += 2; else break;
    }
    g.end = (int64_t)p;
    g.first_mcu = (int32_t)(s * (ri ? ri : total));
    g.mcu_count = (int32_t)(ri && s * ri + ri < total ? ri : total - g.first_mcu);
    if (s + 1 < nseg) {      // RSTn is due: fill bytes, then the marker in order
      while (p + 1 < len && data[p] == 0xFF && data[p + 1] == 0xFF) ++p;
      if (!(p + 1 < len) || data[p] != 0xFF || data[p + 1] != (unsigned)(0xD0 + rst))
        JPEG_FAIL(YV4_E_INVALID, "jpeg: restart marker %d is missing (MCU %lld of %lld)", rst,
                  (long long)g.first_mcu + g.mcu_count, (long long)total);
      pos = p + 2;
      rst = (rst + 1) & 7;
    } else if (p + 1 < len && data[p] == 0xFF && data[p + 1] >= 0xD0 && data[p + 1] <= 0xD7) {
      JPEG_FAIL(YV4_E_INVALID, "jpeg: more entropy-coded data than the header's %lld MCUs", (long long)total);
    }
  }
  return YV4_OK;
}

extern "C" int yv4_jpeg_entropy_workgroups(const yv4_jpeg_scan* scans, int N, yv4_jpeg_wg* wgs, int64_t wg_capacity,
                                           int64_t* count) {
  if (!scans || !count || N <= 0) JPEG_FAIL(YV4_E_INVALID, "jpeg_entropy_workgroups: null pointer or no image");
  int64_t n = 0;
  for (int i = 0; i < N; ++i) {
    if (scans[i].nseg < 1) JPEG_FAIL(YV4_E_INVALID, "jpeg_entropy_workgroups: image %d has no segment", i);
    for (int32_t first = 0; first < scans[i].nseg; first += YV4_JPEG_WG_SEGMENTS, ++n) {
      if (!wgs) continue;
      if (n >= wg_capacity) {
        ::yv4::set_error("jpeg_entropy_workgroups: more than %lld workgroups", (long long)wg_capacity);
        return YV4_E_CAPACITY;
      }
      const int32_t left = scans[i].nseg - first;
      wgs[n].image = i; wgs[n].first_seg = first;
      wgs[n].count = left < YV4_JPEG_WG_SEGMENTS ? left : YV4_JPEG_WG_SEGMENTS;
      wgs[n].reserved = 0;
    }
  }
  *count = n;
  return YV4_OK;
}

#define REQUIRE(cond, ...) do { if (!(cond)) JPEG_FAIL(YV4_E_INVALID, __VA_ARGS__); } while (0)

// Everything the decode indexes with, checked on the host copies: the kernel trusts the device copies.
// -> [*coef_lo, *coef_hi): the batch's coefficient range.
int yv4::jpeg_entropy_validate(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_wg* wgs, int N,
                               int64_t nseg, int64_t nwg, int64_t bytes_len, int64_t nhuff, int64_t coef_elems,
                               int64_t* coef_lo, int64_t* coef_hi) {
  REQUIRE(N > 0 && nseg > 0 && nwg > 0 && bytes_len > 0 && nhuff > 0 && coef_elems > 0,
          "jpeg_entropy: empty batch, table or buffer");
  REQUIRE(nseg < (1ll << 31) && nwg < (1ll << 31), "jpeg_entropy: the batch is too large for one launch");
  int64_t seg = 0, wg = 0, lo = coef_elems, hi = 0;
  for (int n = 0; n < N; ++n) {
    const yv4_jpeg_scan& c = scans[n];
    REQUIRE(c.ncomp == 1 || c.ncomp == 3, "jpeg_entropy: image %d: component count %d", n, c.ncomp);
    const bool samp_ok = c.ncomp == 1 ? (c.hs == 1 && c.vs == 1)
                                      : ((c.hs == 1 && c.vs == 1) || (c.hs == 2 && c.vs == 1) || (c.hs == 2 && c.vs == 2));
    REQUIRE(samp_ok, "jpeg_entropy: image %d: sampling %dx%d", n, c.hs, c.vs);
    REQUIRE(c.mcus_x >= 1 && c.mcus_x <= 8192 && c.mcus_y >= 1 && c.mcus_y <= 8192, "jpeg_entropy: image %d: MCU grid", n);
    const int64_t total = (int64_t)c.mcus_x * c.mcus_y;
    const int64_t blocks = total * (c.hs * c.vs + (c.ncomp == 3 ? 2 : 0));
    REQUIRE(c.ncoef == 64 * blocks, "jpeg_entropy: image %d: ncoef does not follow from its MCU grid", n);
    REQUIRE(c.coef_off >= 0 && (c.coef_off & 63) == 0 && c.coef_off <= coef_elems - c.ncoef,
            "jpeg_entropy: image %d: its coefficients leave the buffer", n);
    REQUIRE(c.data_len > 0 && c.data_off >= 0 && c.data_off <= bytes_len - c.data_len,
            "jpeg_entropy: image %d: its file leaves the byte buffer", n);
    REQUIRE(c.nhuff >= 1 && c.nhuff <= YV4_JPEG_MAX_HUFF && c.huff_base >= 0 && c.huff_base <= nhuff - c.nhuff,
            "jpeg_entropy: image %d: its Huffman tables leave the table buffer", n);
    for (int i = 0; i < c.ncomp; ++i)
      REQUIRE(c.td[i] >= 0 && c.td[i] < c.nhuff && c.ta[i] >= 0 && c.ta[i] < c.nhuff,
              "jpeg_entropy: image %d: Huffman table index of component %d", n, i);
    REQUIRE(c.nseg >= 1 && c.seg_base == seg && c.nseg <= nseg - seg, "jpeg_entropy: image %d: seg_base / nseg", n);
    int64_t mcu = 0;
    for (int32_t s = 0; s < c.nseg; ++s) {
      const yv4_jpeg_segment& g = segs[seg + s];
      REQUIRE(g.begin >= 0 && g.begin <= g.end && g.end <= c.data_len,
              "jpeg_entropy: image %d: segment %d leaves the file", n, s);
      REQUIRE(g.first_mcu == mcu && g.mcu_count >= 1 && g.mcu_count <= total - mcu,
              "jpeg_entropy: image %d: the MCU range of segment %d", n, s);
      REQUIRE(g.bit_off == 0 && g.reserved == 0 && g.pred[0] == 0 && g.pred[1] == 0 && g.pred[2] == 0 && g.pred[3] == 0,
              "jpeg_entropy: image %d: segment %d carries an entry state (not built: must be zero)", n, s);
      mcu += g.mcu_count;
    }
    REQUIRE(mcu == total, "jpeg_entropy: image %d: its segments hold %lld of %lld MCUs", n, (long long)mcu, (long long)total);
    for (int32_t first = 0; first < c.nseg; first += YV4_JPEG_WG_SEGMENTS, ++wg) {
      REQUIRE(wg < nwg, "jpeg_entropy: image %d: the workgroup table ends early", n);
      const int32_t left = c.nseg - first;
      REQUIRE(wgs[wg].image == n && wgs[wg].first_seg == first &&
                  wgs[wg].count == (left < YV4_JPEG_WG_SEGMENTS ? left : YV4_JPEG_WG_SEGMENTS),
              "jpeg_entropy: workgroup %lld is not the next run of image %d", (long long)wg, n);
    }
    seg += c.nseg;
    if (c.coef_off < lo) lo = c.coef_off;
    if (c.coef_off + c.ncoef > hi) hi = c.coef_off + c.ncoef;
  }
  REQUIRE(seg == nseg && wg == nwg, "jpeg_entropy: %lld segments and %lld workgroups for tables of %lld and %lld",
          (long long)seg, (long long)wg, (long long)nseg, (long long)nwg);
  *coef_lo = lo; *coef_hi = hi;
  return YV4_OK;
}

extern "C" int yv4_jpeg_entropy_decode_segments(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs,
                                                const yv4_jpeg_wg* wgs, int N, int64_t nseg, int64_t nwg,
                                                const uint8_t* bytes, int64_t bytes_len, const yv4_jpeg_huff* huff,
                                                int64_t nhuff, int16_t* coef, int64_t coef_elems, int32_t* status) {
  REQUIRE(scans && segs && wgs && bytes && huff && coef && status, "jpeg_entropy_decode_segments: null pointer");
  int64_t lo, hi;
  const int st = yv4::jpeg_entropy_validate(scans, segs, wgs, N, nseg, nwg, bytes_len, nhuff, coef_elems, &lo, &hi);
  if (st != YV4_OK) return st;
  memset(coef + lo, 0, (size_t)(hi - lo) * sizeof(int16_t));
  memset(status, 0, (size_t)N * sizeof(int32_t));
  for (int64_t w = 0; w < nwg; ++w) {      // the kernel's mapping: workgroup w, lane l
    const yv4_jpeg_scan& c = scans[wgs[w].image];
    for (int l = 0; l < wgs[w].count; ++l) {
      const int e = yv4::jpeg::decode_segment(c, segs[c.seg_base + wgs[w].first_seg + l], bytes + c.data_off,
                                              huff + c.huff_base, kZigzag, coef + c.coef_off);
      if (e > status[wgs[w].image]) status[wgs[w].image] = e;
    }
  }
  return YV4_OK;
}

extern "C" const char* yv4_jpeg_entropy_strerror(int code) {
  switch (code) {
    case 0: return "no error";
    case YV4_JPEG_ERR_OVERRUN: return "the entropy-coded data ends inside a block";
    case YV4_JPEG_ERR_CODE: return "a code that is in no Huffman table";
    case YV4_JPEG_ERR_DC_CATEGORY: return "a DC magnitude category above 11";
    case YV4_JPEG_ERR_INDEX: return "a coefficient index past 63";
    case YV4_JPEG_ERR_TRAILING: return "data where a restart marker or the end of the scan is due";
  }
  return "unknown error code";
}
