// Stand-alone sanitizer driver for the JPEG decoder's host half (mmdet-yolov4_amd/csrc/jpeg_host.cpp).
//
// Build and run on the CPU, never loaded into Python and never on a GPU machine:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/jpeg_sanitize.cpp mmdet-yolov4_amd/csrc/jpeg_host.cpp -o /tmp/jpeg_sanitize
//   python tools/jpeg_fixtures_dump.py /tmp/jpeg_fixtures && /tmp/jpeg_sanitize /tmp/jpeg_fixtures/*.jpg
//
// For every file given: parse and entropy-decode it as it is, every prefix of it, and every single-byte change
// (XOR 0xFF, +1 and one set bit) inside the header segments and the first bytes of the scan.  The coefficient buffer
// is exactly info.ncoef elements on the heap, the input an exact-length heap copy, so AddressSanitizer sees any read
// or write past either.  A file that carries an APP1 segment (the EXIF fixtures of tests/golden/jpeg_exif.npz, which
// jpeg_fixtures_dump.py writes as well) gets one more pass: the same three changes of every byte of every APP1 segment
// through yv4_jpeg_parse alone, whose orientation must stay within 0 .. 8 and whose other fields must not depend on the
// segment's payload.  Exit status 0: nothing was reported; the counts of each return code are printed.
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
static long g_app1_inputs, g_app1_files, g_orient[9];

// parse only, on an exact-length heap copy -> status; info is filled
static int parse_copy(const uint8_t* src, size_t len, yv4_jpeg_info* info) {
  uint8_t* data = (uint8_t*)malloc(len ? len : 1);
  memcpy(data, src, len);
  const int st = yv4_jpeg_parse(data, len, info);
  free(data);
  if (st == YV4_OK && (info->orientation < 0 || info->orientation > 8)) {
    fprintf(stderr, "parse returned orientation %d\n", info->orientation);
    exit(2);
  }
  return st;
}

// every byte of every APP1 payload (after its length field), three changes each, through the parse alone
static void app1_pass(std::vector<uint8_t>& buf) {
  yv4_jpeg_info base;
  if (parse_copy(buf.data(), buf.size(), &base) != YV4_OK) return;
  ++g_orient[base.orientation];
  bool any = false;
  size_t pos = 2;
  while (pos + 4 <= buf.size() && pos < (size_t)base.scan_offset && buf[pos] == 0xFF) {
    const unsigned m = buf[pos + 1];
    const size_t seglen = ((size_t)buf[pos + 2] << 8) | buf[pos + 3];
    if (seglen < 2 || pos + 2 + seglen > buf.size()) break;
    if (m == 0xE1) {
      any = true;
      for (size_t i = pos + 4; i < pos + 2 + seglen; ++i) {
        const uint8_t keep = buf[i];
        const uint8_t variants[3] = {(uint8_t)(keep ^ 0xFF), (uint8_t)(keep + 1), (uint8_t)(keep ^ (1u << (i & 7)))};
        for (int v = 0; v < 3; ++v) {
          buf[i] = variants[v];
          yv4_jpeg_info info;
          const int st = parse_copy(buf.data(), buf.size(), &info);
          ++g_app1_inputs;
          info.orientation = base.orientation;
          if (st != YV4_OK || memcmp(&info, &base, sizeof(info)) != 0) {
            fprintf(stderr, "a change inside an APP1 payload (offset %zu) changed more than the orientation\n", i);
            exit(2);
          }
        }
        buf[i] = keep;
      }
    }
    pos += 2 + seglen;
  }
  if (any) ++g_app1_files;
}

static int run(const uint8_t* src, size_t len) {
  uint8_t* data = (uint8_t*)malloc(len ? len : 1);      // exact length: a read past it is a heap overflow
  memcpy(data, src, len);
  yv4_jpeg_info info, info2;
  int st = yv4_jpeg_parse(data, len, &info);
  if (st == YV4_OK) {
    if (info.orientation < 0 || info.orientation > 8) {
      fprintf(stderr, "parse returned orientation %d\n", info.orientation);
      exit(2);
    }
    if (info.ncoef <= 0 || info.ncoef > (int64_t)64 * 3 * 8192 * 8192) {
      fprintf(stderr, "parse returned OK with ncoef %lld\n", (long long)info.ncoef);
      exit(2);
    }
    if (info.ncoef > (1 << 24)) {       // a changed size field: show the capacity path instead of allocating gigabytes
      int16_t one;
      st = yv4_jpeg_entropy_decode(data, len, &info2, &one, 1);
      if (st != YV4_E_CAPACITY) {
        fprintf(stderr, "capacity 1 for %lld coefficients returned %d\n", (long long)info.ncoef, st);
        exit(2);
      }
    } else {
      int16_t* coef = (int16_t*)malloc((size_t)info.ncoef * sizeof(int16_t));
      memset(coef, 0x5a, (size_t)info.ncoef * sizeof(int16_t));
      st = yv4_jpeg_entropy_decode(data, len, &info2, coef, info.ncoef);
      if (memcmp(&info, &info2, sizeof(info)) != 0) {
        fprintf(stderr, "parse and entropy_decode disagree about the header\n");
        exit(2);
      }
      free(coef);
    }
  }
  free(data);
  if (st > 0 || st < -4) {
    fprintf(stderr, "unknown status %d\n", st);
    exit(2);
  }
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
    size_t span = st == YV4_OK ? (size_t)info.scan_offset + 64 : buf.size();
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
    app1_pass(buf);
  }
  printf("APP1: %ld files, %ld changed inputs; orientation of the files as given:", g_app1_files, g_app1_inputs);
  for (int o = 0; o <= 8; ++o) printf(" %d:%ld", o, g_orient[o]);
  printf("\n");
  printf("ok %ld  invalid %ld  unsupported %ld  capacity %ld\n", g_count[0], g_count[1], g_count[2], g_count[4]);
  return 0;
}
