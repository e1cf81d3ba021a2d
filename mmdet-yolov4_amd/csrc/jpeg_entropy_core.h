// The Huffman scan decode of the baseline JPEG decoder as one body for the host and the device: the bit reader and the
// block decode of jpeg_host.cpp (BitReader, decode_symbol, receive_extend, decode_block) restated over plain pointers
// and the packed table form (yv4_jpeg_huff), plus the loop over one segment's MCUs.  csrc/jpeg_entropy.hip runs it one
// lane per segment, csrc/jpeg_entropy_host.cpp on the CPU over the same tables (yv4_jpeg_entropy_decode_segments), so
// that the tests without a GPU and tools/jpeg_entropy_sanitize.cpp exercise the code the kernel runs.  jpeg_host.cpp is
// the oracle: for every file both give the same coefficients, and they fail on the same files.
// The second half of the file is the chunk decode (many lanes per segment) over the same reader and symbol decode.
//
// A segment is a run of whole MCUs whose bytes [begin, end) start on a byte boundary in the initial state (DC
// predictors zero, first block of an MCU).  The bytes are untrusted; the counts (MCU range, block grid) were validated
// by the host.  Every read stays inside [begin, end), every loop is bounded by a validated count (MCUs, at most 10
// blocks per MCU, 64 coefficients per block, 7 code lengths), every store lands on a block of the image's own grid.
#ifndef YV4_JPEG_ENTROPY_CORE_H_
#define YV4_JPEG_ENTROPY_CORE_H_
#include <stdint.h>

#include "yv4.h"
#include "jpeg_common.h"      // YV4_JPEG_ZIGZAG

#if defined(__HIPCC__) && defined(__HIP__)
#define YV4_JPEG_HD __host__ __device__ __forceinline__
#else
#define YV4_JPEG_HD inline
#endif

namespace yv4 {
namespace jpeg {

// MSB-first bit reader over one segment.  0xFF00 is the data byte 0xFF; at any other marker, or at the end of the
// segment's bytes, the reader stops advancing and feeds zero bits, counting them: a block whose decode reached into
// them was cut short.
struct BitReader {
  const uint8_t* d;
  int64_t pos, end;
  uint64_t acc;
  int nbits, fake;
  bool stopped;

  YV4_JPEG_HD void fill() {
    while (nbits <= 56) {
      unsigned byte = 0;
      if (!stopped) {
        if (pos < end) {
          byte = d[pos];
          if (byte != 0xFF) ++pos;
          else if (pos + 1 < end && d[pos + 1] == 0) pos += 2;
          else stopped = true;
        } else {
          stopped = true;
        }
      }
      if (stopped) { byte = 0; if (fake < (1 << 20)) fake += 8; }
      acc = (acc << 8) | byte;
      nbits += 8;
    }
  }
  YV4_JPEG_HD unsigned peek(int n) const { return (unsigned)((acc >> (nbits - n)) & ((1u << n) - 1u)); }   // 1 <= n <= 16 <= nbits
  YV4_JPEG_HD void skip(int n) { nbits -= n; }
  YV4_JPEG_HD bool overrun() const { return nbits < fake; }
  YV4_JPEG_HD int real_bits() const { return nbits - fake; }
};

// -> symbol, or -1 for a code in no table.  Codes of up to 9 bits come from the lookahead; longer ones from the
// canonical bounds of lengths 10..16 (maxcode / valoff index 0 is length 10).
YV4_JPEG_HD int decode_symbol(BitReader& b, const yv4_jpeg_huff& h) {
  b.fill();
  const unsigned e = h.look[b.peek(9)];
  if (e) {
    b.skip((int)(e >> 8));
    return (int)(e & 255);
  }
  const int code16 = (int)b.peek(16);
  for (int l = 10; l <= 16; ++l) {
    const int code = code16 >> (16 - l);
    if (code <= h.maxcode[l - 10]) {
      b.skip(l);
      return h.vals[(h.valoff[l - 10] + code) & 255];      // in 0 .. nvals - 1 for a table yv4_jpeg_scan_prepare packed
    }
  }
  return -1;
}

// the s-bit magnitude field -> signed value (T.81 F.2.2.1 EXTEND).  No refill: decode_symbol's left at least
// 57 - 16 bits behind the code, and s <= 15.
YV4_JPEG_HD int receive_extend(BitReader& b, int s) {
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block: blk[0] and the nonzero AC coefficients are written (the block was zero-filled before).  -> 0 or a
// YV4_JPEG_ERR_* code.
YV4_JPEG_HD int decode_block(BitReader& b, const yv4_jpeg_huff& dc, const yv4_jpeg_huff& ac, const uint8_t* zigzag,
                             int& pred, int16_t* blk) {
  int s = decode_symbol(b, dc);
  if (s < 0) return YV4_JPEG_ERR_CODE;
  if (s > 11) return YV4_JPEG_ERR_DC_CATEGORY;
  if (s) pred += receive_extend(b, s);
  pred = (int16_t)pred;      // libjpeg stores the running value as a 16-bit coefficient: wrap, do not grow
  blk[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return YV4_JPEG_ERR_CODE;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;      // EOB
      k += 16;                 // ZRL
      continue;
    }
    k += r;
    if (k > 63) return YV4_JPEG_ERR_INDEX;
    blk[zigzag[k]] = (int16_t)receive_extend(b, s);
    ++k;
  }
  if (b.overrun()) return YV4_JPEG_ERR_OVERRUN;
  return 0;
}

// One segment of image `sc`: `bytes` is the image's file, `tabs` its packed tables (sc.nhuff of them), `zigzag` the 64
// entries of YV4_JPEG_ZIGZAG, `coef` the image's first coefficient.  -> 0 or a YV4_JPEG_ERR_* code; on an error the
// segment stops where it is.
YV4_JPEG_HD int decode_segment(const yv4_jpeg_scan& sc, const yv4_jpeg_segment& sg, const uint8_t* bytes,
                               const yv4_jpeg_huff* tabs, const uint8_t* zigzag, int16_t* coef) {
  BitReader b = {bytes, sg.begin, sg.end, 0, 0, 0, false};
  const int nc = sc.ncomp;
  const int64_t bw0 = (int64_t)sc.mcus_x * sc.hs, nb0 = bw0 * ((int64_t)sc.mcus_y * sc.vs);
  const int64_t nb1 = (int64_t)sc.mcus_x * sc.mcus_y;       // a chroma plane: one block per MCU
  int pred0 = 0, pred1 = 0, pred2 = 0;
  int my = sg.first_mcu / sc.mcus_x, mx = sg.first_mcu - my * sc.mcus_x;
  for (int m = 0; m < sg.mcu_count; ++m) {
    for (int v = 0; v < sc.vs; ++v)
      for (int h = 0; h < sc.hs; ++h) {
        const int64_t by = (int64_t)my * sc.vs + v, bx = (int64_t)mx * sc.hs + h;
        const int st = decode_block(b, tabs[sc.td[0]], tabs[sc.ta[0]], zigzag, pred0, coef + 64 * (by * bw0 + bx));
        if (st) return st;
      }
    if (nc == 3) {
      const int64_t cb = (int64_t)my * sc.mcus_x + mx;
      int st = decode_block(b, tabs[sc.td[1]], tabs[sc.ta[1]], zigzag, pred1, coef + 64 * (nb0 + cb));
      if (st) return st;
      st = decode_block(b, tabs[sc.td[2]], tabs[sc.ta[2]], zigzag, pred2, coef + 64 * (nb0 + nb1 + cb));
      if (st) return st;
    }
    if (++mx == sc.mcus_x) { mx = 0; ++my; }
  }
  // what follows the last MCU is padding to the byte boundary: a whole byte more is data where a restart marker (or
  // the end of the scan) is due
  b.fill();
  if (b.real_bits() >= 8) return YV4_JPEG_ERR_TRAILING;
  return 0;
}

// ---- chunks: entry points inside a segment (include/yv4.h, "self-synchronising chunks") --------------------------------
// A segment's bytes are cut into chunks of chunk_bytes raw bytes; a coded symbol (a Huffman code and its magnitude
// bits) belongs to the chunk in which its first bit lies.  The decoder state at a symbol boundary is packed into one
// word, so that "the chain closes" is one comparison:
//   (bit position in the file: byte * 8 + bit) << 16 | block index within the MCU << 8 | zigzag index k
// k = 0: a DC symbol is next.  The position is canonical: its byte is never the 0x00 of a stuffed 0xFF00 pair.
constexpr uint64_t kChunkInvalid = ~0ull;      // the exit of a pass that met an error: no state, adopted by nobody

YV4_JPEG_HD uint64_t chunk_state(int64_t byte, int bit, int blk, int k) {
  return ((uint64_t)(byte * 8 + bit) << 16) | ((uint64_t)blk << 8) | (uint64_t)k;
}

YV4_JPEG_HD int blocks_per_mcu(const yv4_jpeg_scan& sc) { return sc.hs * sc.vs + (sc.ncomp == 3 ? 2 : 0); }

// byte range of chunk `index` of a segment: [*cb, *ce)
YV4_JPEG_HD void chunk_range(const yv4_jpeg_segment& sg, int32_t index, int32_t chunk_bytes, int64_t* cb, int64_t* ce) {
  *cb = sg.begin + (int64_t)index * chunk_bytes;
  *ce = *cb + chunk_bytes < sg.end ? *cb + chunk_bytes : sg.end;
}

// The state a chunk is first decoded from.  Chunk 0 starts in the segment's true state.  Every other chunk guesses: its
// first bit, block 0, a DC symbol next -- and looks one byte back: a chunk that begins on the 0x00 of a stuffed pair
// begins, canonically, one byte later.  index > 0 puts cb - 1 inside the segment.
YV4_JPEG_HD uint64_t chunk_guess(const yv4_jpeg_segment& sg, const uint8_t* bytes, int32_t index, int32_t chunk_bytes) {
  int64_t cb, ce;
  chunk_range(sg, index, chunk_bytes, &cb, &ce);
  if (index > 0 && cb < sg.end && bytes[cb] == 0 && bytes[cb - 1] == 0xFF) ++cb;
  return chunk_state(cb, 0, 0, 0);
}

// first coefficient of block `ordinal` (counted from the segment's first MCU) of image sc.  ordinal is below
// sg.mcu_count * blocks_per_mcu, which the host validated against the grid.
YV4_JPEG_HD int64_t chunk_block_offset(const yv4_jpeg_scan& sc, const yv4_jpeg_segment& sg, int64_t ordinal) {
  const int nluma = sc.hs * sc.vs, bpm = blocks_per_mcu(sc);
  const int64_t mcu = sg.first_mcu + ordinal / bpm;
  const int bi = (int)(ordinal % bpm);
  const int64_t my = mcu / sc.mcus_x, mx = mcu - my * sc.mcus_x;
  const int64_t bw0 = (int64_t)sc.mcus_x * sc.hs;
  if (bi < nluma) {
    const int v = bi / sc.hs, h = bi - v * sc.hs;
    return 64 * ((my * sc.vs + v) * bw0 + (mx * sc.hs + h));
  }
  const int64_t nb0 = bw0 * ((int64_t)sc.mcus_y * sc.vs), nb1 = (int64_t)sc.mcus_x * sc.mcus_y;
  return 64 * (nb0 + (bi - nluma) * nb1 + my * sc.mcus_x + mx);
}

// what one pass over a chunk leaves
struct ChunkPass {
  uint64_t exit;        // the state at the first symbol that starts at or behind the chunk's end; kChunkInvalid
  int32_t nblk;         // blocks completed
  uint32_t dc[3];       // per component: the sum of the DC differences decoded (wraps; the low 16 bits count)
  int tail_real;        // real bits left behind the exit (exact below 8)
};

// One pass over chunk `index` of segment sg from state `entry` (at or behind the chunk's first byte).  kStore = false
// is the speculative / counting form: nothing is stored, an error (a code in no table, an index past 63, a DC category
// above 11, a symbol that reaches past the segment's bytes) only says that the entry was wrong, and leaves
// exit = kChunkInvalid.  kStore = true is the storing form, run from a proven entry: `ordinal` is the block the entry
// lies in, pred the DC predictors there; DC terms and nonzero AC terms go into the zero-filled planes as decode_block
// writes them, and an error is returned as its YV4_JPEG_ERR_* code.
// A pass cannot know where the segment's padding begins without the block count.  So where fewer than 8 real bits are
// left -- what decode_segment takes for padding once the MCUs are done -- a symbol that fails in any way (no code, or
// one that reaches past the segment's bytes) ends the pass in front of it, in both forms, with the state there as the
// exit; the storing form also ends at the segment's last block.  The chunks behind adopt that state, fail on the same
// symbol and leave the same state, so the chain still closes; the caller holds the segment's block total against the
// MCU count and the last chunk's tail_real against decode_segment's rule.
// Bounds: at most max_symbols = 8 * chunk_bytes + 32 symbols (each consumes at least one bit, the entry lies less than
// a symbol in front of the chunk, and the pass ends at the first symbol behind it); every read inside
// [sg.begin, sg.end); every store on a block below seg_blocks.
template <bool kStore>
YV4_JPEG_HD int decode_chunk(const yv4_jpeg_scan& sc, const yv4_jpeg_segment& sg, const uint8_t* bytes,
                             const yv4_jpeg_huff* tabs, const uint8_t* zigzag, int32_t index, int32_t count,
                             int32_t chunk_bytes, uint64_t entry, int64_t ordinal, const int16_t* pred_in, int16_t* coef,
                             ChunkPass* out) {
  const int nluma = sc.hs * sc.vs, bpm = blocks_per_mcu(sc);
  const int64_t seg_blocks = (int64_t)sg.mcu_count * bpm;
  int64_t cb, cend;
  chunk_range(sg, index, chunk_bytes, &cb, &cend);
  int64_t cur = (int64_t)(entry >> 19);
  int bit = (int)(entry >> 16) & 7, blk = (int)(entry >> 8) & 255, k = (int)entry & 255;
  if (cur < sg.begin) cur = sg.begin;      // never: every state this file produces lies inside its segment
  if (cur > sg.end) cur = sg.end;
  if (blk >= bpm) blk = 0;
  // the component's tables by selection, not by an index into sc.td / sc.ta: those stay in registers
  const int td0 = sc.td[0], td1 = sc.td[1], td2 = sc.td[2], ta0 = sc.ta[0], ta1 = sc.ta[1], ta2 = sc.ta[2];
  int comp = blk < nluma ? 0 : blk - nluma + 1;
  int pred0 = 0, pred1 = 0, pred2 = 0;
  if (kStore) { pred0 = pred_in[0]; pred1 = pred_in[1]; pred2 = pred_in[2]; }
  if (ordinal < 0 || ordinal > seg_blocks) ordinal = seg_blocks;      // never for a proven chunk: no block to store to
  int16_t* blkp = coef;
  if (kStore && ordinal < seg_blocks) blkp = coef + chunk_block_offset(sc, sg, ordinal);
  out->exit = kChunkInvalid;
  out->nblk = 0;
  out->dc[0] = out->dc[1] = out->dc[2] = 0;
  out->tail_real = 64;

  BitReader b = {bytes, cur, sg.end, 0, 0, 0, false};
  b.fill();
  b.skip(bit);
  if (b.overrun()) return YV4_JPEG_ERR_OVERRUN;
  int nblk = 0, tail_real = -1;
  uint32_t dc0 = 0, dc1 = 0, dc2 = 0;
  const int max_symbols = 8 * chunk_bytes + 32;
  int n = 0;
  for (; n < max_symbols; ++n) {
    if (cur >= cend) break;                                   // the next symbol belongs to a later chunk
    if (kStore && k == 0 && ordinal >= seg_blocks) break;     // the segment's last block is done
    b.fill();
    const int have = b.nbits, real = b.real_bits();
    int nk = k, value = 0, fail = 0;
    bool stored = false;
    if (k == 0) {
      const int s = decode_symbol(b, tabs[comp == 0 ? td0 : comp == 1 ? td1 : td2]);
      if (s < 0) fail = YV4_JPEG_ERR_CODE;
      else if (s > 11) fail = YV4_JPEG_ERR_DC_CATEGORY;
      else if (s) value = receive_extend(b, s);
      nk = 1;
    } else {
      const int rs = decode_symbol(b, tabs[comp == 0 ? ta0 : comp == 1 ? ta1 : ta2]);
      const int r = rs >> 4, s = rs & 15;
      if (rs < 0) {
        fail = YV4_JPEG_ERR_CODE;
      } else if (s == 0) {
        nk = r != 15 ? 64 : k + 16;      // EOB / ZRL
      } else {
        nk = k + r;
        if (nk > 63) fail = YV4_JPEG_ERR_INDEX;
        else value = receive_extend(b, s);
        stored = true;
      }
    }
    if (!fail && b.overrun()) fail = YV4_JPEG_ERR_OVERRUN;      // the symbol reaches past the segment's bytes
    if (fail) {
      if (real >= 8) return fail;
      tail_real = real;      // below 8 the reader had stopped: exact.  The pass ends in front of the symbol
      break;
    }
    if (k == 0) {
      if (comp == 0) { dc0 += (uint32_t)value; pred0 = (int16_t)(pred0 + value); if (kStore) blkp[0] = (int16_t)pred0; }
      else if (comp == 1) { dc1 += (uint32_t)value; pred1 = (int16_t)(pred1 + value); if (kStore) blkp[0] = (int16_t)pred1; }
      else { dc2 += (uint32_t)value; pred2 = (int16_t)(pred2 + value); if (kStore) blkp[0] = (int16_t)pred2; }
    } else if (stored) {
      if (kStore) blkp[zigzag[nk]] = (int16_t)value;
      ++nk;
    }
    k = nk;
    if (k >= 64) {      // the block is complete
      k = 0;
      ++nblk;
      if (++blk == bpm) blk = 0;
      comp = blk < nluma ? 0 : blk - nluma + 1;
      if (kStore) {
        ++ordinal;
        blkp = ordinal < seg_blocks ? coef + chunk_block_offset(sc, sg, ordinal) : coef;
      }
    }
    // the cursor follows the bits the symbol took: at most 31 + 7 of them, so at most four bytes
    bit += have - b.nbits;
    for (int i = 0; i < 5 && bit >= 8; ++i) {
      bit -= 8;
      if (cur < sg.end) cur += (bytes[cur] == 0xFF) ? 2 : 1;
    }
    if (cur > sg.end) cur = sg.end;
  }
  if (n == max_symbols && cur < cend) return YV4_JPEG_ERR_OVERRUN;      // cannot happen: every symbol takes a bit
  if (tail_real < 0) {
    b.fill();
    tail_real = b.real_bits();
  }
  out->exit = chunk_state(cur, bit, blk, k);
  out->nblk = nblk;
  out->dc[0] = dc0; out->dc[1] = dc1; out->dc[2] = dc2;
  out->tail_real = tail_real;
  return 0;
}

// One synchronisation round for chunk ck, whose record is e[0]; `prev` is the record of the chunk before it in the
// same segment (unused for index 0), `in` / `out` select the exit words read and written (a round reads what the round
// before wrote, so that no lane reads a word another lane of the same round writes).  Round 0 decodes every chunk from
// its guess.  A later round re-decodes a chunk only if the chunk before it left a state that differs from the entry
// it was decoded from; that state then replaces the entry.
YV4_JPEG_HD void sync_chunk(const yv4_jpeg_scan& sc, const yv4_jpeg_segment& sg, const uint8_t* bytes,
                            const yv4_jpeg_huff* tabs, const uint8_t* zigzag, const yv4_jpeg_chunk& ck,
                            int32_t chunk_bytes, int round, uint64_t prev_exit, yv4_jpeg_entry* e) {
  const int in = (round + 1) & 1, out = round & 1;
  uint64_t entry;
  if (round == 0) {
    entry = chunk_guess(sg, bytes, ck.index, chunk_bytes);
  } else {
    if (ck.index == 0 || prev_exit == kChunkInvalid || prev_exit == e->entry) {
      e->exit[out] = e->exit[in];
      return;
    }
    entry = prev_exit;
  }
  ChunkPass p;
  const int err = decode_chunk<false>(sc, sg, bytes, tabs, zigzag, ck.index, ck.count, chunk_bytes, entry, 0, nullptr,
                                      nullptr, &p);
  e->entry = entry;
  e->exit[out] = err ? kChunkInvalid : p.exit;
  e->nblk = p.nblk;
  e->dc[0] = (uint16_t)p.dc[0]; e->dc[1] = (uint16_t)p.dc[1]; e->dc[2] = (uint16_t)p.dc[2];
  e->tail = (uint16_t)(p.tail_real < 8 ? 1 : 0);
  e->first_block = 0;
  e->pred[0] = e->pred[1] = e->pred[2] = 0;
  e->reserved = 0;
}

// The checks on chunk ck once the exclusive sums over its segment are known: `first` blocks and DC sums dcs before it,
// `prev_exit` the final exit of the chunk before it.  Writes first_block / pred and -> true if the chunk is proven.
YV4_JPEG_HD bool check_chunk(const yv4_jpeg_scan& sc, const yv4_jpeg_segment& sg, const yv4_jpeg_chunk& ck, int fin,
                             uint64_t prev_exit, int64_t first, const uint32_t* dcs, yv4_jpeg_entry* e) {
  const int bpm = blocks_per_mcu(sc);
  const int64_t seg_blocks = (int64_t)sg.mcu_count * bpm;
  const uint64_t exit = e->exit[fin];
  bool ok = exit != kChunkInvalid;
  if (ck.index > 0) ok = ok && prev_exit == e->entry;                       // the chain closes
  ok = ok && first <= seg_blocks && first + e->nblk <= seg_blocks;
  ok = ok && (int)((e->entry >> 8) & 255) == (int)(first % bpm);            // block index against block ordinal
  if (ck.index == ck.count - 1)                                             // the segment ends as decode_segment ends
    ok = ok && first + e->nblk == seg_blocks && (exit & 0xFFFF) == 0 && e->tail == 1;
  e->first_block = ok ? (int32_t)first : -1;
  e->pred[0] = (int16_t)dcs[0]; e->pred[1] = (int16_t)dcs[1]; e->pred[2] = (int16_t)dcs[2];
  return ok;
}

}  // namespace jpeg
}  // namespace yv4
#endif  // YV4_JPEG_ENTROPY_CORE_H_
