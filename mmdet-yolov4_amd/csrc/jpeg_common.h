// What the JPEG decoder's three host-side sources share (jpeg_host.cpp, jpeg_entropy_host.cpp, jpeg_entropy.hip): the
// error macros, the zigzag order, the prototypes of the internal entries that cross a file, and the one enumeration of
// workgroup runs and of a segment's chunks that a table's builder and its validator both go through.  Internal: not
// part of include/yv4.h.
#ifndef YV4_JPEG_COMMON_H_
#define YV4_JPEG_COMMON_H_
#include <stdint.h>
#include <stddef.h>

#include "yv4.h"

// natural-order index of the k-th coefficient of the scan (the kernels keep a copy in LDS, next to the Huffman tables)
#define YV4_JPEG_ZIGZAG                                                                                      \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,                     \
   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,                     \
   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

#define JPEG_FAIL(code, ...)        \
  do {                              \
    ::yv4::set_error(__VA_ARGS__);  \
    return (code);                  \
  } while (0)
#define REQUIRE(cond, ...) do { if (!(cond)) JPEG_FAIL(YV4_E_INVALID, __VA_ARGS__); } while (0)

namespace yv4 {

void set_error(const char* fmt, ...);

// yv4_jpeg_parse, which also says where the Huffman tables lie: dht[class][slot] is the address of the 16 counts of the
// last definition of that table in front of the scan (the values follow them), or null.  Defined in jpeg_host.cpp.
int jpeg_parse_tables(const uint8_t* data, size_t len, yv4_jpeg_info* info, const uint8_t* dht[2][4]);

// Everything the segment / the chunk decode indexes with, checked on the host copies (jpeg_entropy_host.cpp).
int jpeg_entropy_validate(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_wg* wgs, int N,
                          int64_t nseg, int64_t nwg, int64_t bytes_len, int64_t nhuff, int64_t coef_elems,
                          int64_t* coef_lo, int64_t* coef_hi);
int jpeg_sync_validate(const yv4_jpeg_scan* scans, const yv4_jpeg_segment* segs, const yv4_jpeg_chunk* chunks,
                       const int32_t* seg_first, const yv4_jpeg_wg* wgs, int N, int64_t nseg, int64_t nchunk, int64_t nwg,
                       int64_t bytes_len, int64_t nhuff, int32_t chunk_bytes, int32_t max_rounds, int64_t coef_elems,
                       int64_t* coef_lo, int64_t* coef_hi);

// The workgroups of one image: [first, end) cut into runs of at most `per`, f(first of the run, its count) for each in
// order.  A status of f other than YV4_OK ends the walk and is returned.
template <class F>
inline int for_each_run(int64_t first, int64_t end, int64_t per, F f) {
  for (; first < end; first += per) {
    const int64_t left = end - first;
    const int st = f(first, left < per ? left : per);
    if (st != YV4_OK) return st;
  }
  return YV4_OK;
}

// The chunks of one segment: every chunk_bytes raw bytes one, an empty segment one as well.
inline int64_t jpeg_chunks_of(const yv4_jpeg_segment& g, int32_t chunk_bytes) {
  const int64_t n = (g.end - g.begin + chunk_bytes - 1) / chunk_bytes;
  return n < 1 ? 1 : n;
}

}  // namespace yv4
#endif  // YV4_JPEG_COMMON_H_
