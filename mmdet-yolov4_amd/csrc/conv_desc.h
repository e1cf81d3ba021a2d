// The descriptor check of every convolution entry point (forward fp32 / 16-bit / fp8, their split-K and scattered
// forms, the stem, the weight gradient).  Plain C++ without a HIP call: tools/conv_desc_check.cpp compiles it on its own.
// What an entry alone knows stays with the entry: pointers and their alignment, dtypes, 4 GiB addressability, the
// workspace, whether a forced tile applies, the stem's shape rule.
#pragma once
#include "yv4.h"

namespace yv4 {

void set_error(const char* fmt, ...);

// What differs between the entries, and nothing else.
struct ConvDescRules {
  int align;                  // Cin, x_cstride, x_coff are multiples of it: 4 (fp32), 8 (16-bit), 16 (fp8), 1 (stem: own rule)
  bool residual = false;      // a residual view is present
  bool align_cout = false;    // Cout is a multiple of `align` too (weight gradient: dY is an operand)
  bool align_y = false;       // y_cstride and y_coff as well (weight gradient, 16-bit scatter)
  bool scatter = false;       // stride 1 only, and Ho / Wo are taken as given (rows past the input's edge read zeros)
  int acts = 2;               // activation ids the entry applies: 2, 1 (stem), 0 (identity epilogue: scatter, weight gradient)
  bool any_taps = false;      // fp8: no 64-bit tap mask in the kernel, so no limit of 64 taps
  bool misaligned_is_unsupported = false;   // fp8: YV4_E_UNSUPPORTED for a misaligned view, elsewhere YV4_E_INVALID
};

#define YV4_DESC_REQUIRE(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return YV4_E_INVALID; } } while (0)

// YV4_OK, or YV4_E_INVALID / YV4_E_UNSUPPORTED with the message set ("<who>: ...").  d is not null.
inline int check_conv_desc(const yv4_conv_desc* d, const char* who, const ConvDescRules& r) {
  YV4_DESC_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "%s: empty shape", who);
  YV4_DESC_REQUIRE(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->pad >= 0, "%s: bad kernel/stride/pad", who);
  YV4_DESC_REQUIRE(!r.scatter || d->stride == 1, "%s: stride-1 kernels only", who);
  YV4_DESC_REQUIRE(r.any_taps || (long long)d->KH * d->KW <= 64, "%s: kernels above 64 taps are not supported", who);
  const int al = r.align;
  if (d->Cin % al || d->x_cstride % al || d->x_coff % al || (r.align_cout && d->Cout % al) ||
      (r.align_y && (d->y_cstride % al || d->y_coff % al))) {
    set_error("%s: Cin = %d, x_cstride = %d, x_coff = %d%s must be multiples of %d", who, d->Cin, d->x_cstride, d->x_coff,
              r.align_cout ? ", Cout and the y view" : r.align_y ? " and the y view" : "", al);
    return r.misaligned_is_unsupported ? YV4_E_UNSUPPORTED : YV4_E_INVALID;
  }
  YV4_DESC_REQUIRE(d->x_coff >= 0 && (long long)d->x_coff + d->Cin <= d->x_cstride, "%s: input view exceeds its pixel stride", who);
  YV4_DESC_REQUIRE(d->y_coff >= 0 && (long long)d->y_coff + d->Cout <= d->y_cstride, "%s: output view exceeds its pixel stride", who);
  YV4_DESC_REQUIRE(!r.residual || (d->r_coff >= 0 && (long long)d->r_coff + d->Cout <= d->r_cstride),
                   "%s: residual view exceeds its pixel stride", who);
  const long long Ho = r.scatter ? d->Ho : ((long long)d->H + 2LL * d->pad - d->KH) / d->stride + 1;
  const long long Wo = r.scatter ? d->Wo : ((long long)d->W + 2LL * d->pad - d->KW) / d->stride + 1;
  YV4_DESC_REQUIRE(Ho == d->Ho && Wo == d->Wo && Ho > 0 && Wo > 0, "%s: Ho/Wo (%d,%d) do not match the geometry (%lld,%lld)",
                   who, d->Ho, d->Wo, Ho, Wo);
  YV4_DESC_REQUIRE((r.acts < 1 || (d->act1 >= 0 && d->act1 <= YV4_ACT_SWISH)) &&
                   (r.acts < 2 || (d->act2 >= 0 && d->act2 <= YV4_ACT_SWISH)), "%s: unknown activation id", who);
  // (all factors are positive here; two at a time, so that the 64-bit product cannot overflow either)
  auto fits31 = [](long long n, int h, int w) { return n * h < (1LL << 31) && n * h * w < (1LL << 31); };
  YV4_DESC_REQUIRE(fits31(d->N, d->Ho, d->Wo) && fits31(d->N, d->H, d->W), "%s: N*Ho*Wo or N*H*W does not fit 31 bits", who);
  return YV4_OK;
}

#undef YV4_DESC_REQUIRE

}  // namespace yv4
