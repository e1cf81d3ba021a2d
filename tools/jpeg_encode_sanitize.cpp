// Stand-alone sanitizer driver for the JPEG encoder's host side and shared core
// (mmdet-yolov4_amd/csrc/jpeg_enc_host.cpp, jpeg_enc_core.h -- the code the kernels of jpeg_enc.hip run).
//
// Build and run on the CPU, never loaded into Python and never on a GPU machine:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Immdet-yolov4_amd/csrc \
//       tools/jpeg_encode_sanitize.cpp mmdet-yolov4_amd/csrc/jpeg_enc_host.cpp mmdet-yolov4_amd/csrc/jpeg_host.cpp \
//       -o /tmp/jpeg_encode_sanitize
//   python tools/jpeg_encode_fixtures_dump.py /tmp/jpeg_encode_fixtures && /tmp/jpeg_encode_sanitize /tmp/jpeg_encode_fixtures/*.bin
//
// A .bin file is one case of tests/golden/jpeg_encode.npz: int32 height, width, channels, quality, hs, vs, file length;
// the pixels (R G B, or the gray plane); libjpeg-turbo's file.  For every case: yv4_jpeg_encode_layout, the whole method
// on the CPU (yv4_jpeg_encode_host) and yv4_jpeg_encode_header, every buffer an exact-length heap block so that
// AddressSanitizer sees any access past one, and the result held against the file, byte for byte.  Then the second
// stage once more over coefficients that no encoder makes (every one -32768 .. 32767 from a fixed generator): the bound
// the output is sized by must hold for those too.  Exit status 0: nothing was reported.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
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

static void die(const char* file, const char* what) {
  fprintf(stderr, "%s: %s: %s\n", file, what, yv4::g_err);
  exit(2);
}

static void run(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) die(path, "cannot open");
  int32_t head[7];
  if (fread(head, sizeof(head), 1, f) != 1) die(path, "short header");
  const size_t npix = (size_t)head[0] * head[1] * head[2];
  uint8_t* pix = (uint8_t*)malloc(npix);
  uint8_t* want = (uint8_t*)malloc((size_t)head[6]);
  if (fread(pix, 1, npix, f) != npix || fread(want, 1, (size_t)head[6], f) != (size_t)head[6]) die(path, "short file");
  fclose(f);

  yv4_jpeg_enc_image im;
  memset(&im, 0, sizeof(im));
  im.height = head[0]; im.width = head[1]; im.channels = head[2]; im.quality = head[3]; im.hs = head[4]; im.vs = head[5];
  int64_t totals[6];
  if (yv4_jpeg_encode_layout(&im, 1, totals) != YV4_OK) die(path, "layout");
  if ((size_t)totals[0] < npix) die(path, "pixel total");
  int16_t* coef = (int16_t*)malloc((size_t)totals[1] * 2);
  uint8_t* work = (uint8_t*)malloc((size_t)totals[2]);
  uint8_t* out = (uint8_t*)malloc((size_t)totals[3]);
  int64_t size = 0;
  // the pixel buffer is exactly the image: layout's total is 256-byte aligned, the validation only needs the last row
  if (yv4_jpeg_encode_host(&im, 1, 3, pix, (int64_t)npix, 1, coef, totals[1], work, totals[2], out, totals[3], &size) != YV4_OK)
    die(path, "encode_host");
  uint8_t* header = (uint8_t*)malloc(YV4_JPEG_ENC_HEADER_MAX);
  int64_t hlen = 0;
  if (yv4_jpeg_encode_header(&im, header, YV4_JPEG_ENC_HEADER_MAX, &hlen) != YV4_OK) die(path, "encode_header");
  if (hlen + size + 2 != head[6] || memcmp(header, want, (size_t)hlen) != 0 ||
      memcmp(out + im.out_off, want + hlen, (size_t)size) != 0 || want[head[6] - 2] != 0xFF || want[head[6] - 1] != 0xD9) {
    yv4::set_error("%lld + %lld + 2 bytes, libjpeg-turbo's file has %d", (long long)hlen, (long long)size, head[6]);
    die(path, "the file differs");
  }
  // the host decoder reads the same coefficients back from the file
  yv4_jpeg_info info;
  int16_t* back = (int16_t*)malloc((size_t)totals[1] * 2);
  if (yv4_jpeg_entropy_decode(want, (size_t)head[6], &info, back, totals[1]) != YV4_OK || info.ncoef != totals[1] ||
      memcmp(back, coef, (size_t)totals[1] * 2) != 0)
    die(path, "the coefficients differ from the host decoder's");

  // stage 2 over arbitrary coefficients: the derived bound holds whatever the buffer contains
  uint32_t s = 12345u + (uint32_t)head[6];
  for (int64_t k = 0; k < totals[1]; ++k) {
    s = s * 1664525u + 1013904223u;
    coef[k] = (int16_t)(s >> 16);
  }
  if (yv4_jpeg_encode_host(&im, 1, 2, nullptr, 0, 1, coef, totals[1], work, totals[2], out, totals[3], &size) != YV4_OK)
    die(path, "encode_host on arbitrary coefficients");
  if (size > im.out_cap) die(path, "more bytes than the bound");
  free(back); free(header); free(out); free(work); free(coef); free(want); free(pix);
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) run(argv[i]);
  // the refusals: nothing is written for a table that does not validate
  yv4_jpeg_enc_image im;
  memset(&im, 0, sizeof(im));
  im.height = 16; im.width = 16; im.channels = 3; im.quality = 0; im.hs = 2; im.vs = 2;
  int64_t totals[6];
  if (yv4_jpeg_encode_layout(&im, 1, totals) != YV4_E_INVALID) die("refusals", "quality 0 accepted");
  im.quality = 90;
  if (yv4_jpeg_encode_layout(&im, 1, totals) != YV4_OK) die("refusals", "layout");
  if (yv4_jpeg_encode_validate(&im, 1, totals[0], totals[1], totals[2], im.out_off + im.out_cap - 1) != YV4_E_INVALID)
    die("refusals", "an output buffer that ends inside the image's region accepted");
  printf("%d cases: every file equal to libjpeg-turbo's, nothing reported\n", argc - 1);
  return 0;
}
