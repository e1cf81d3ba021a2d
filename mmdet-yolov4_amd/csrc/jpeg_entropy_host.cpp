// Host side of the device Huffman decode (include/yv4.h, "the Huffman scan on the device"): the segment table, the
// packed Huffman tables and the workgroup table of a batch, their validation, and the CPU run of the shared decode
// (jpeg_entropy_core.h); and the same for the chunk decode: the chunk tables, their validation and the whole method on
// the CPU (yv4_jpeg_chunks_build, yv4_jpeg_entropy_decode_sync).  No HIP call: plain C++, usable without a GPU, and
// compiled on its own with sanitizers by tools/jpeg_entropy_sanitize.cpp and tools/jpeg_entropy_sync_sanitize.cpp.
//
// The bytes are untrusted.  The header parse (jpeg_host.cpp) has checked every header segment's length against the file
// and hands over where the Huffman tables it accepted lie; the marker walk reads below len only.
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include "yv4.h"
#include "jpeg_common.h"
#include "jpeg_entropy_core.h"

namespace {

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

const uint8_t kZigzag[64] = YV4_JPEG_ZIGZAG;

// One run of a workgroup table (for_each_run): the builders' store, which only counts without a table, and the
// validators' comparison.
int put_run(const char* who, yv4_jpeg_wg* wgs, int64_t capacity, int64_t& n, int image, int64_t first, int64_t count) {
  if (wgs) {
    if (n >= capacity) {
      ::yv4::set_error("%s: more than %lld workgroups", who, (long long)capacity);
      return YV4_E_CAPACITY;
    }
    wgs[n] = {image, (int32_t)first, (int32_t)count, 0};
  }
  ++n;
  return YV4_OK;
}

bool is_run(const yv4_jpeg_wg& w, int image, int64_t first, int64_t count) {
  return w.image == image && w.first_seg == first && w.count == count;
}

}  // namespace

extern "C" int yv4_jpeg_scan_prepare(const uint8_t* data, size_t len, yv4_jpeg_info* info, yv4_jpeg_scan* scan,
                                     yv4_jpeg_huff* huff, yv4_jpeg_segment* segs, int64_t seg_capacity) {
  if (!data || !info || !scan || !huff || !segs) JPEG_FAIL(YV4_E_INVALID, "jpeg_scan_prepare: null pointer");
  const uint8_t* dht[2][4];      // the one header walk: the info, and where the tables it accepted lie
  const int st = yv4::jpeg_parse_tables(data, len, info, dht);
  if (st != YV4_OK) return st;
  memset(scan, 0, sizeof(*scan));
  const int64_t total = (int64_t)info->mcus_x * info->mcus_y;
  const int64_t ri = info->restart_interval;
  const int64_t nseg = ri ? (total + ri - 1) / ri : 1;
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

  // the tables the scan references, each packed once (the parse has refused a scan that names a missing one)
  int slot[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
  int nhuff = 0;
  for (int i = 0; i < info->ncomp; ++i)
    for (int cls = 0; cls < 2; ++cls) {
      const int id = cls ? info->ta[i] : info->td[i];
      if (!dht[cls][id]) JPEG_FAIL(YV4_E_INVALID, "jpeg_scan_prepare: Huffman table %d of class %d is missing", id, cls);
      if (slot[cls][id] < 0) {
        const uint8_t* counts = dht[cls][id];
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
    const int st = yv4::for_each_run(0, scans[i].nseg, YV4_JPEG_WG_SEGMENTS, [&](int64_t first, int64_t cnt) {
      return put_run("jpeg_entropy_workgroups", wgs, wg_capacity, n, i, first, cnt);
    });
    if (st != YV4_OK) return st;
  }
  *count = n;
  return YV4_OK;
}

// Everything the decode indexes with, checked on the host copies: the kernel trusts the device copies.
// -> [*coef_lo, *coef_hi): the batch's coefficient range.
int yv4::jpeg_entropy_validate(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_wg* wgs, int N,
                               int64_t nseg, int64_t nwg, int64_t bytes_len, int64_t nhuff, int64_t coef_elems,
                               int64_t* coef_lo, int64_t* coef_hi) {
  // wgs == nullptr: the caller has a workgroup table of another kind (the chunk decode), which it checks itself
  REQUIRE(N > 0 && nseg > 0 && (nwg > 0 || !wgs) && bytes_len > 0 && nhuff > 0 && coef_elems > 0,
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
    const int st = for_each_run(0, wgs ? c.nseg : 0, YV4_JPEG_WG_SEGMENTS, [&](int64_t first, int64_t cnt) -> int {
      REQUIRE(wg < nwg, "jpeg_entropy: image %d: the workgroup table ends early", n);
      REQUIRE(is_run(wgs[wg], n, first, cnt), "jpeg_entropy: workgroup %lld is not the next run of image %d", (long long)wg, n);
      ++wg;
      return YV4_OK;
    });
    if (st != YV4_OK) return st;
    seg += c.nseg;
    if (c.coef_off < lo) lo = c.coef_off;
    if (c.coef_off + c.ncoef > hi) hi = c.coef_off + c.ncoef;
  }
  REQUIRE(seg == nseg && (wg == nwg || !wgs), "jpeg_entropy: %lld segments and %lld workgroups for tables of %lld and %lld",
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

// ---- self-synchronising chunks (include/yv4.h) ----------------------------------------------------------------------------

extern "C" int yv4_jpeg_chunks_build(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, int N, int64_t nseg,
                                     int32_t chunk_bytes, yv4_jpeg_chunk* chunks, int64_t chunk_capacity,
                                     int32_t* seg_first, yv4_jpeg_wg* wgs, int64_t wg_capacity, int64_t* nchunk,
                                     int64_t* nwg) {
  REQUIRE(scans && segs && nchunk && nwg && N > 0 && nseg > 0, "jpeg_chunks_build: null pointer or no image");
  REQUIRE(chunk_bytes >= YV4_JPEG_MIN_CHUNK_BYTES && chunk_bytes <= YV4_JPEG_MAX_CHUNK_BYTES,
          "jpeg_chunks_build: chunk_bytes %d is not in %d .. %d", chunk_bytes, YV4_JPEG_MIN_CHUNK_BYTES,
          YV4_JPEG_MAX_CHUNK_BYTES);
  REQUIRE(!chunks || (seg_first && wgs), "jpeg_chunks_build: chunks without seg_first and wgs");
  int64_t nc = 0, nw = 0, seg = 0;
  for (int n = 0; n < N; ++n) {
    const yv4_jpeg_scan& c = scans[n];
    REQUIRE(c.nseg >= 1 && c.seg_base == seg && c.nseg <= nseg - seg, "jpeg_chunks_build: image %d: seg_base / nseg", n);
    const int64_t image_first = nc;
    for (int32_t s = 0; s < c.nseg; ++s, ++seg) {
      const yv4_jpeg_segment& g = segs[seg];
      REQUIRE(g.begin >= 0 && g.begin <= g.end, "jpeg_chunks_build: image %d: segment %d has end < begin", n, s);
      const int64_t cnt = yv4::jpeg_chunks_of(g, chunk_bytes);
      REQUIRE(nc + cnt < (1ll << 31), "jpeg_chunks_build: the batch has 2^31 chunks or more");
      if (chunks) {
        if (nc + cnt > chunk_capacity) {
          ::yv4::set_error("jpeg_chunks_build: more than %lld chunks", (long long)chunk_capacity);
          return YV4_E_CAPACITY;
        }
        seg_first[seg] = (int32_t)nc;
        for (int64_t i = 0; i < cnt; ++i) {
          yv4_jpeg_chunk& k = chunks[nc + i];
          k.image = n; k.seg = (int32_t)seg; k.index = (int32_t)i; k.count = (int32_t)cnt;
        }
      }
      nc += cnt;
    }
    const int st = yv4::for_each_run(image_first, nc, YV4_JPEG_WG_CHUNKS, [&](int64_t first, int64_t cnt) {
      return put_run("jpeg_chunks_build", chunks ? wgs : nullptr, wg_capacity, nw, n, first, cnt);
    });
    if (st != YV4_OK) return st;
  }
  REQUIRE(seg == nseg, "jpeg_chunks_build: %lld segments for a table of %lld", (long long)seg, (long long)nseg);
  if (chunks) seg_first[nseg] = (int32_t)nc;
  *nchunk = nc; *nwg = nw;
  return YV4_OK;
}

namespace yv4 {
// Everything the chunk decode indexes with, on the host copies: the scans and segments as the segment decode checks
// them, then every entry of the chunk, seg_first and workgroup tables against what yv4_jpeg_chunks_build makes.
int jpeg_sync_validate(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_chunk* chunks,
                       const int32_t* seg_first, const yv4_jpeg_wg* wgs, int N, int64_t nseg, int64_t nchunk, int64_t nwg,
                       int64_t bytes_len, int64_t nhuff, int32_t chunk_bytes, int32_t max_rounds, int64_t coef_elems,
                       int64_t* coef_lo, int64_t* coef_hi) {
  REQUIRE(chunk_bytes >= YV4_JPEG_MIN_CHUNK_BYTES && chunk_bytes <= YV4_JPEG_MAX_CHUNK_BYTES,
          "jpeg_entropy_sync: chunk_bytes %d is not in %d .. %d", chunk_bytes, YV4_JPEG_MIN_CHUNK_BYTES,
          YV4_JPEG_MAX_CHUNK_BYTES);
  REQUIRE(max_rounds >= 0 && max_rounds <= YV4_JPEG_MAX_ROUNDS, "jpeg_entropy_sync: max_rounds %d is not in 0 .. %d",
          max_rounds, YV4_JPEG_MAX_ROUNDS);
  REQUIRE(nchunk > 0 && nwg > 0 && nchunk < (1ll << 31) && nwg < (1ll << 31), "jpeg_entropy_sync: empty or oversized chunk table");
  const int st = jpeg_entropy_validate(scans, segs, nullptr, N, nseg, 0, bytes_len, nhuff, coef_elems, coef_lo, coef_hi);
  if (st != YV4_OK) return st;
  int64_t nc = 0, nw = 0;
  for (int n = 0; n < N; ++n) {
    const yv4_jpeg_scan& c = scans[n];
    const int64_t image_first = nc;
    for (int32_t s = 0; s < c.nseg; ++s) {
      const int64_t seg = c.seg_base + s;
      const int64_t cnt = jpeg_chunks_of(segs[seg], chunk_bytes);
      REQUIRE(cnt <= nchunk - nc, "jpeg_entropy_sync: image %d: the chunk table ends early", n);
      REQUIRE(seg_first[seg] == nc, "jpeg_entropy_sync: image %d: seg_first of segment %d", n, s);
      for (int64_t i = 0; i < cnt; ++i) {
        const yv4_jpeg_chunk& k = chunks[nc + i];
        REQUIRE(k.image == n && k.seg == seg && k.index == i && k.count == cnt,
                "jpeg_entropy_sync: chunk %lld is not chunk %lld of segment %d of image %d", (long long)(nc + i),
                (long long)i, s, n);
      }
      nc += cnt;
    }
    const int st = for_each_run(image_first, nc, YV4_JPEG_WG_CHUNKS, [&](int64_t first, int64_t cnt) -> int {
      REQUIRE(nw < nwg, "jpeg_entropy_sync: image %d: the workgroup table ends early", n);
      REQUIRE(is_run(wgs[nw], n, first, cnt), "jpeg_entropy_sync: workgroup %lld is not the next run of image %d", (long long)nw, n);
      ++nw;
      return YV4_OK;
    });
    if (st != YV4_OK) return st;
  }
  REQUIRE(nc == nchunk && nw == nwg && seg_first[nseg] == nchunk,
          "jpeg_entropy_sync: %lld chunks and %lld workgroups for tables of %lld and %lld", (long long)nc, (long long)nw,
          (long long)nchunk, (long long)nwg);
  return YV4_OK;
}
}  // namespace yv4

extern "C" int yv4_jpeg_entropy_decode_sync(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs,
                                            const yv4_jpeg_chunk* chunks, const int32_t* seg_first, const yv4_jpeg_wg* wgs,
                                            int N, int64_t nseg, int64_t nchunk, int64_t nwg, const uint8_t* bytes,
                                            int64_t bytes_len, const yv4_jpeg_huff* huff, int64_t nhuff,
                                            int32_t chunk_bytes, int32_t max_rounds, yv4_jpeg_entry* entries,
                                            int16_t* coef, int64_t coef_elems, int32_t* status, int32_t* undecided,
                                            int32_t* rounds) {
  REQUIRE(scans && segs && chunks && seg_first && wgs && bytes && huff && entries && coef && status && undecided,
          "jpeg_entropy_decode_sync: null pointer");
  int64_t lo, hi;
  const int st = yv4::jpeg_sync_validate(scans, segs, chunks, seg_first, wgs, N, nseg, nchunk, nwg, bytes_len, nhuff,
                                         chunk_bytes, max_rounds, coef_elems, &lo, &hi);
  if (st != YV4_OK) return st;
  memset(coef + lo, 0, (size_t)(hi - lo) * sizeof(int16_t));
  memset(status, 0, (size_t)N * sizeof(int32_t));
  memset(undecided, 0, (size_t)N * sizeof(int32_t));
  using namespace yv4::jpeg;
  // 1. sync: the kernel's mapping, workgroup w, lane l, one pass over the table per round.  The exit word a round reads
  // is the one the round before wrote, so the order of the lanes within a round does not matter here either.
  int32_t last_change = 0;
  for (int r = 0; r <= max_rounds; ++r)
    for (int64_t w = 0; w < nwg; ++w) {
      const yv4_jpeg_scan& c = scans[wgs[w].image];
      for (int l = 0; l < wgs[w].count; ++l) {
        const int64_t g = (int64_t)wgs[w].first_seg + l;
        const yv4_jpeg_chunk& k = chunks[g];
        const uint64_t prev = r > 0 && k.index > 0 ? entries[g - 1].exit[(r + 1) & 1] : kChunkInvalid;
        const uint64_t before = r > 0 ? entries[g].entry : 0;
        sync_chunk(c, segs[k.seg], bytes + c.data_off, huff + c.huff_base, kZigzag, k, chunk_bytes, r, prev, &entries[g]);
        if (r > 0 && entries[g].entry != before) last_change = r;
      }
    }
  if (rounds) *rounds = last_change;
  // 2. the exclusive sums over each segment's chunks, and the checks
  const int fin = max_rounds & 1;
  for (int64_t s = 0; s < nseg; ++s) {
    int64_t first = 0;
    uint32_t dcs[3] = {0, 0, 0};
    for (int64_t g = seg_first[s]; g < seg_first[s + 1]; ++g) {
      const yv4_jpeg_chunk& k = chunks[g];
      const uint64_t prev = k.index > 0 ? entries[g - 1].exit[fin] : kChunkInvalid;
      if (!check_chunk(scans[k.image], segs[s], k, fin, prev, first, dcs, &entries[g])) undecided[k.image] = 1;
      first += entries[g].nblk;
      for (int j = 0; j < 3; ++j) dcs[j] += entries[g].dc[j];
    }
  }
  // 3. the storing decode of the decided images
  for (int64_t g = 0; g < nchunk; ++g) {
    const yv4_jpeg_chunk& k = chunks[g];
    if (undecided[k.image]) continue;
    const yv4_jpeg_scan& c = scans[k.image];
    ChunkPass p;
    const int e = decode_chunk<true>(c, segs[k.seg], bytes + c.data_off, huff + c.huff_base, kZigzag, k.index, k.count,
                                     chunk_bytes, entries[g].entry, entries[g].first_block, entries[g].pred,
                                     coef + c.coef_off, &p);
    if (e || p.exit != entries[g].exit[fin] || p.nblk != entries[g].nblk) undecided[k.image] = 2;
  }
  // 4. what is not proven goes to the one lane per segment decode, which decides the status
  for (int n = 0; n < N; ++n) {
    if (!undecided[n]) continue;
    const yv4_jpeg_scan& c = scans[n];
    memset(coef + c.coef_off, 0, (size_t)c.ncoef * sizeof(int16_t));
    for (int32_t s = 0; s < c.nseg; ++s) {
      const int e = decode_segment(c, segs[c.seg_base + s], bytes + c.data_off, huff + c.huff_base, kZigzag, coef + c.coef_off);
      if (e > status[n]) status[n] = e;
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
