// Stand-alone sanitizer driver for the self-synchronising chunk decode of the Huffman scan on the CPU
// (mmdet-yolov4_amd/csrc/jpeg_entropy_host.cpp: yv4_jpeg_chunks_build, yv4_jpeg_entropy_decode_sync; jpeg_entropy_core.h:
// the chunk pass, the round and the checks the kernels of jpeg_entropy.hip run).
//
// Build and run on the CPU, never loaded into Python and never on a GPU machine:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Immdet-yolov4_amd/csrc \
//       tools/jpeg_entropy_sync_sanitize.cpp mmdet-yolov4_amd/csrc/jpeg_host.cpp \
//       mmdet-yolov4_amd/csrc/jpeg_entropy_host.cpp -o /tmp/jpeg_entropy_sync_sanitize
//   python tools/jpeg_fixtures_dump.py /tmp/jpeg_fixtures && /tmp/jpeg_entropy_sync_sanitize /tmp/jpeg_fixtures/*.jpg
//
// For every file given: the file as it is, every prefix of it, three changes of every byte of the header segments and
// of the first 64 bytes of the scan (XOR 0xFF, +1 and one set bit) and one flipped bit in every other byte of the scan
// -- the inputs of tools/jpeg_entropy_sanitize.cpp.  The file itself and the header changes run at each of chunk_bytes 4
// (the smallest allowed), 16 and 256 times max_rounds 0, 1 and 48 (the default); the prefixes and the scan-byte flips,
// which are most of the inputs, take those nine pairs in turn, one pair per input.  The file, every table, the entry
// records and the coefficient buffer are exact-length heap blocks, so AddressSanitizer sees any read or write past any
// of them.  Every outcome is held against the host decoder yv4_jpeg_entropy_decode: the same status class, and on
// success the same coefficients.  Exit status 0: nothing was reported; the counts of inputs, of decodes and of images
// that took the second decode are printed (per process: the files can be spread over several).
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

static const int32_t kChunkBytes[3] = {YV4_JPEG_MIN_CHUNK_BYTES, 16, 256};
static const int32_t kRounds[3] = {0, 1, 48};
static long g_inputs, g_count[5];      // OK, INVALID, UNSUPPORTED, (LAUNCH), CAPACITY
static long g_decodes, g_fallback, g_fallback_ok, g_multi_chunk;

static void die(const char* what, long a, long b) {
  fprintf(stderr, "%s (%ld, %ld): %s\n", what, a, b, yv4::g_err);
  exit(2);
}

// -> the status class of the chunk decode of one input (the same at every chunk size and round count, or die)
// `pair`: 0 .. 8 selects one (chunk size, round count) pair, -1 runs all nine
static int run(const uint8_t* src, size_t len, int pair = -1) {
  ++g_inputs;
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
  int st = yv4_jpeg_scan_prepare(data, len, &info2, scan, huff, &one, 0);
  yv4_jpeg_segment* segs = nullptr;
  if (st == YV4_E_CAPACITY) {
    const int64_t nseg = scan->nseg;
    if (nseg < 1 || nseg > (int64_t)8192 * 8192) die("prepare reported a segment count of", (long)nseg, 0);
    segs = (yv4_jpeg_segment*)malloc((size_t)nseg * sizeof(yv4_jpeg_segment));
    st = yv4_jpeg_scan_prepare(data, len, &info2, scan, huff, segs, nseg);
  } else if (st == YV4_OK) {
    die("prepare accepted a capacity of 0", 0, 0);
  }
  if (st == YV4_OK && small) {
    yv4_jpeg_huff* packed = (yv4_jpeg_huff*)malloc(sizeof(yv4_jpeg_huff) * (size_t)scan->nhuff);
    memcpy(packed, huff, sizeof(yv4_jpeg_huff) * (size_t)scan->nhuff);
    int16_t* coef = (int16_t*)malloc((size_t)scan->ncoef * sizeof(int16_t));
    int cls = 1;
    for (int ci = 0; ci < 3; ++ci) {
      if (pair >= 0 && pair / 3 != ci) continue;
      const int32_t cb = kChunkBytes[ci];
      int64_t nchunk = 0, nwg = 0;
      if (yv4_jpeg_chunks_build(scan, segs, 1, scan->nseg, cb, nullptr, 0, nullptr, nullptr, 0, &nchunk, &nwg) != YV4_OK)
        die("chunks_build count", cb, 0);
      yv4_jpeg_chunk* chunks = (yv4_jpeg_chunk*)malloc((size_t)nchunk * sizeof(yv4_jpeg_chunk));
      int32_t* seg_first = (int32_t*)malloc((size_t)(scan->nseg + 1) * sizeof(int32_t));
      yv4_jpeg_wg* wgs = (yv4_jpeg_wg*)malloc((size_t)nwg * sizeof(yv4_jpeg_wg));
      yv4_jpeg_entry* entries = (yv4_jpeg_entry*)malloc((size_t)nchunk * sizeof(yv4_jpeg_entry));
      if (yv4_jpeg_chunks_build(scan, segs, 1, scan->nseg, cb, chunks, nchunk - 1, seg_first, wgs, nwg, &nchunk, &nwg) !=
          YV4_E_CAPACITY)
        die("chunks_build accepted a capacity one short", cb, (long)nchunk);
      if (yv4_jpeg_chunks_build(scan, segs, 1, scan->nseg, cb, chunks, nchunk, seg_first, wgs, nwg, &nchunk, &nwg) != YV4_OK)
        die("chunks_build", cb, (long)nchunk);
      for (int ri = 0; ri < 3; ++ri) {
        if (pair >= 0 && pair % 3 != ri) continue;
        memset(coef, 0x5a, (size_t)scan->ncoef * sizeof(int16_t));
        memset(entries, 0xa5, (size_t)nchunk * sizeof(yv4_jpeg_entry));
        int32_t status = -1, undecided = -1, rounds = -1;
        const int e = yv4_jpeg_entropy_decode_sync(scan, segs, chunks, seg_first, wgs, 1, scan->nseg, nchunk, nwg, data,
                                                   (int64_t)len, packed, scan->nhuff, cb, kRounds[ri], entries, coef,
                                                   scan->ncoef, &status, &undecided, &rounds);
        if (e != YV4_OK) die("decode_sync refused the builders' own tables", e, cb);
        if (status < 0 || status > YV4_JPEG_ERR_TRAILING || undecided < 0 || rounds < 0 || rounds > kRounds[ri])
          die("status / undecided / rounds word", status, undecided);
        if (status && !undecided) die("a status code without the second decode", status, cb);
        ++g_decodes;
        if (nchunk > scan->nseg) ++g_multi_chunk;
        if (undecided) { ++g_fallback; if (!status) ++g_fallback_ok; }
        const int got = status ? YV4_E_INVALID : YV4_OK;
        if (got != want) die("status class differs from the host decoder's: got / want", got, want);
        if (got == YV4_OK && memcmp(coef, ref, (size_t)scan->ncoef * sizeof(int16_t)) != 0)
          die("the coefficients differ from the host decoder's", (long)len, cb);
        cls = got;
      }
      free(entries);
      free(wgs);
      free(seg_first);
      free(chunks);
    }
    st = cls;
    free(coef);
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
    for (size_t n = 0; n < buf.size(); ++n) run(buf.data(), n, (int)(n % 9));         // every prefix
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
      run(buf.data(), buf.size(), (int)(i % 9));
      buf[i] ^= (uint8_t)(1u << (i & 7));
    }
  }
  printf("inputs %ld: ok %ld  invalid %ld  unsupported %ld  capacity %ld\n", g_inputs, g_count[0], g_count[1], g_count[2],
         g_count[4]);
  printf("chunk decodes %ld, %ld of them with a segment of several chunks\n", g_decodes,
         g_multi_chunk);
  printf("second decode taken %ld times, %ld of them on an input that then decoded without error\n", g_fallback,
         g_fallback_ok);
  return 0;
}
