// Stand-alone sanitizer driver for the device Huffman decode's host side and shared core
// (mmdet-yolov4_amd/csrc/jpeg_entropy_host.cpp, jpeg_entropy_core.h -- the code the kernel of jpeg_entropy.hip runs).
//
// Build and run on the CPU, never loaded into Python and never on a GPU machine:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Immdet-yolov4_amd/csrc \
//       tools/jpeg_entropy_sanitize.cpp mmdet-yolov4_amd/csrc/jpeg_host.cpp mmdet-yolov4_amd/csrc/jpeg_entropy_host.cpp \
//       -o /tmp/jpeg_entropy_sanitize
//   python tools/jpeg_fixtures_dump.py /tmp/jpeg_fixtures && /tmp/jpeg_entropy_sanitize /tmp/jpeg_fixtures/*.jpg
//
// For every file given: yv4_jpeg_scan_prepare + yv4_jpeg_entropy_workgroups + yv4_jpeg_entropy_decode_segments on the
// file as it is, on every prefix of it, and on every single-byte change (XOR 0xFF, +1 and one set bit) inside the
// header segments and the first bytes of the scan -- the changes tools/jpeg_sanitize.cpp makes -- plus one flipped bit
// in every byte of the scan.  The file, the segment table, the packed tables and the coefficient buffer are exact-length
// heap blocks, so AddressSanitizer sees any read or write past any of them.  Every outcome is held against the host
// decoder yv4_jpeg_entropy_decode: the same status class, and on success the same coefficients.  Exit status 0:
// nothing was reported; the counts of each outcome are printed.
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "yv4.h"

namespace yv4 {
static char g_err[512];
void set_error(const char* fmt, ...) {      // the library's is in api.hip
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace yv4

static long g_count[5];      // OK, INVALID, UNSUPPORTED, (LAUNCH), CAPACITY
static long g_by_code[8];    // YV4_JPEG_ERR_* seen in a status word

static void die(const char* what, long a, long b) {
  fprintf(stderr, "%s (%ld, %ld): %s\n", what, a, b, yv4::g_err);
  exit(2);
}

// -> the status class of the segment decode of one input
static int run(const uint8_t* src, size_t len) {
  uint8_t* data = (uint8_t*)malloc(len ? len : 1);      // exact length: a read past it is a heap overflow
  memcpy(data, src, len);
  yv4_jpeg_info info, info2;
  int want = yv4_jpeg_parse(data, len, &info);
  int16_t* ref = nullptr;
  const bool small = want == YV4_OK && info.ncoef <= (1 << 24);      // a changed size field: no gigabytes
  if (small) {
    ref = (int16_t*)malloc((size_t)info.ncoef * sizeof(int16_t));
    want = yv4_jpeg_entropy_decode(data, len, &info2, ref, info.ncoef);
  } else if (want == YV4_OK) {
    free(data);
    ++g_count[-YV4_E_CAPACITY];
    return YV4_E_CAPACITY;
  }

  yv4_jpeg_scan* scan = (yv4_jpeg_scan*)malloc(sizeof(yv4_jpeg_scan));
  yv4_jpeg_huff* huff = (yv4_jpeg_huff*)malloc(sizeof(yv4_jpeg_huff) * YV4_JPEG_MAX_HUFF);
  yv4_jpeg_segment one;
  int st = yv4_jpeg_scan_prepare(data, len, &info2, scan, huff, &one, 0);      // the count, through the capacity path
  yv4_jpeg_segment* segs = nullptr;
  if (st == YV4_E_CAPACITY) {
    const int64_t nseg = scan->nseg;
    if (nseg < 1 || nseg > (int64_t)8192 * 8192) die("prepare reported a segment count of", (long)nseg, 0);
    segs = (yv4_jpeg_segment*)malloc((size_t)nseg * sizeof(yv4_jpeg_segment));
    st = yv4_jpeg_scan_prepare(data, len, &info2, scan, huff, segs, nseg);
    if (st == YV4_OK && scan->nseg != nseg) die("prepare changed its segment count", (long)nseg, scan->nseg);
  } else if (st == YV4_OK) {
    die("prepare accepted a capacity of 0", 0, 0);
  }
  if (st == YV4_OK && small) {
    // pack the tables to exactly nhuff entries, so that an index past them is a heap overflow
    yv4_jpeg_huff* packed = (yv4_jpeg_huff*)malloc(sizeof(yv4_jpeg_huff) * (size_t)scan->nhuff);
    memcpy(packed, huff, sizeof(yv4_jpeg_huff) * (size_t)scan->nhuff);
    int64_t nwg = 0;
    if (yv4_jpeg_entropy_workgroups(scan, 1, nullptr, 0, &nwg) != YV4_OK) die("workgroups count", 0, 0);
    yv4_jpeg_wg* wgs = (yv4_jpeg_wg*)malloc((size_t)nwg * sizeof(yv4_jpeg_wg));
    if (yv4_jpeg_entropy_workgroups(scan, 1, wgs, nwg, &nwg) != YV4_OK) die("workgroups", (long)nwg, 0);
    int16_t* coef = (int16_t*)malloc((size_t)scan->ncoef * sizeof(int16_t));
    memset(coef, 0x5a, (size_t)scan->ncoef * sizeof(int16_t));
    int32_t status = -1;
    st = yv4_jpeg_entropy_decode_segments(scan, segs, wgs, 1, scan->nseg, nwg, data, (int64_t)len, packed, scan->nhuff, coef,
                                          scan->ncoef, &status);
    if (st != YV4_OK) die("decode_segments refused prepare's own tables", st, 0);
    if (status < 0 || status > YV4_JPEG_ERR_TRAILING) die("status word", status, 0);
    ++g_by_code[status];
    if (status) st = YV4_E_INVALID;
    else if (want == YV4_OK && memcmp(coef, ref, (size_t)scan->ncoef * sizeof(int16_t)) != 0)
      die("the coefficients differ from the host decoder's", (long)len, 0);
    free(coef);
    free(wgs);
    free(packed);
  }
  if (small || want != YV4_OK) {
    if (st != want) die("status class differs from the host decoder's: got / want", st, want);
  }
  free(segs);
  free(huff);
  free(scan);
  free(ref);
  free(data);
  if (st > 0 || st < -4) die("unknown status", st, 0);
  ++g_count[-st];
  return st;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> buf;
    uint8_t chunk[4096];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    fclose(f);
    yv4_jpeg_info info;
    const int st = yv4_jpeg_parse(buf.data(), buf.size(), &info);
    run(buf.data(), buf.size());
    for (size_t n = 0; n < buf.size(); ++n) run(buf.data(), n);                       // every prefix
    // every byte of the headers and the first 64 bytes of the scan (the whole file if the headers are refused)
    const size_t scan = st == YV4_OK ? (size_t)info.scan_offset : buf.size();
    size_t span = scan + 64;
    if (span > buf.size()) span = buf.size();
    for (size_t i = 0; i < span; ++i) {
      const uint8_t keep = buf[i];
      const uint8_t variants[3] = {(uint8_t)(keep ^ 0xFF), (uint8_t)(keep + 1), (uint8_t)(keep ^ (1u << (i & 7)))};
      for (int v = 0; v < 3; ++v) {
        buf[i] = variants[v];
        run(buf.data(), buf.size());
      }
      buf[i] = keep;
    }
    for (size_t i = span; i < buf.size(); ++i) {      // the rest of the scan: one bit per byte
      buf[i] ^= (uint8_t)(1u << (i & 7));
      run(buf.data(), buf.size());
      buf[i] ^= (uint8_t)(1u << (i & 7));
    }
  }
  printf("ok %ld  invalid %ld  unsupported %ld  capacity %ld\n", g_count[0], g_count[1], g_count[2], g_count[4]);
  printf("status words: none %ld  overrun %ld  code %ld  dc-category %ld  index %ld  trailing %ld\n", g_by_code[0],
         g_by_code[1], g_by_code[2], g_by_code[3], g_by_code[4], g_by_code[5]);
  return 0;
}
