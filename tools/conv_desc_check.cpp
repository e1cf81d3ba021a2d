// Stand-alone driver for the convolution entry points' shared descriptor check (mmdet-yolov4_amd/csrc/conv_desc.h).
//
// Build and run on the CPU, never loaded into Python and never on a GPU machine:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/conv_desc_check.cpp -o /tmp/conv_desc_check
//   /tmp/conv_desc_check tests/golden/conv_desc_rejects.json
//
// Runs every record of the table of malformed descriptors (tests/golden/make_golden_conv_desc.py) through
// check_conv_desc with the rule set of the record's entry -- the sets the entry points pass, restated below; the weight
// gradient and the stem are covered here only, because tests/test_conv_desc_host.py cannot call them with fake pointers.
// A record's "by" says what to expect: "desc" -- the check returns the record's rc; "none" -- YV4_OK; "entry" -- YV4_OK or
// the record's rc (a rule the entry keeps for itself rejected it before the shared check existed).  Every message starts
// with the entry's prefix.  Then the descriptors are perturbed field by field with extreme values: the check must
// answer without an overflow or a division by zero (the sanitizers see those).  Exit status 0: all as expected.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <regex>
#include <string>

#include "../mmdet-yolov4_amd/csrc/conv_desc.h"

namespace yv4 {
static char g_err[512];
void set_error(const char* fmt, ...) {      // the library's is in api.hip
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace yv4
using namespace yv4;

struct Entry { const char* who; ConvDescRules rules; };
// {align, residual, align_cout, align_y, scatter, acts, any_taps, misaligned_is_unsupported}: the test table passes a
// residual wherever the entry takes one
static const Entry kEntries[] = {
    {"conv", {4, true}},
    {"conv h16", {8, true}},
    {"conv splitk", {4, true}},
    {"conv h16 splitk", {8, true}},
    {"conv scatter", {4, false, false, false, true, 0}},
    {"conv scatter h16", {8, false, false, true, true, 0}},
    {"conv f8", {16, true, false, false, false, 2, true, true}},
    {"wgrad", {4, false, true, true, false, 0}},
    {"wgrad h16", {8, false, true, true, false, 0}},
    {"conv stem", {1, false, false, false, false, 1}},
};

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s tests/golden/conv_desc_rejects.json\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const std::regex rec("\"entry\": \"([^\"]+)\", \"case\": \"([^\"]+)\", \"desc\": \\[([-0-9, ]+)\\], \"rc\": (-?[0-9]+|null), "
                       "\"by\": \"([a-z]+)\", \"tightened\": (true|false)");
  int n = 0, bad = 0, tightened = 0, n_by[3] = {0, 0, 0};
  long perturbed = 0;
  for (std::sregex_iterator it(text.begin(), text.end(), rec), end; it != end; ++it, ++n) {
    const std::string who = (*it)[1], name = (*it)[2], by = (*it)[5];
    const Entry* e = nullptr;
    for (const Entry& k : kEntries)
      if (who == k.who) e = &k;
    yv4_conv_desc d;
    memset(&d, 0, sizeof(d));
    int32_t* f = &d.N;      // N .. act2: 19 consecutive int32 fields
    int nf = 0;
    const std::string list = (*it)[3];
    for (const char* p = list.c_str(); *p && nf < 19;) {
      char* q = nullptr;
      f[nf++] = (int32_t)strtol(p, &q, 10);
      p = *q == ',' ? q + 1 : q;
    }
    if (!e || nf != 19) {
      printf("BAD RECORD %s / %s\n", who.c_str(), name.c_str());
      ++bad;
      continue;
    }
    const int want = (*it)[4] == "null" ? 0 : atoi((*it)[4].str().c_str());
    g_err[0] = 0;
    const int rc = check_conv_desc(&d, e->who, e->rules);
    const bool ok = by == "desc" ? rc == want && rc != YV4_OK : by == "none" ? rc == YV4_OK : rc == YV4_OK || rc == want;
    const bool prefix = rc == YV4_OK || (strncmp(g_err, e->who, strlen(e->who)) == 0 && g_err[strlen(e->who)] == ':');
    n_by[by == "desc" ? 0 : by == "entry" ? 1 : 2]++;
    tightened += (*it)[6] == "true";
    if (!ok || !prefix) {
      printf("MISMATCH %s / %s (%s): rc %d, expected %d: %s\n", who.c_str(), name.c_str(), by.c_str(), rc, want, g_err);
      ++bad;
    }
    // every field at the edges of int32: an answer, no trap
    static const int32_t kEdge[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 63, 64, 65, 1 << 16, 1 << 30, INT32_MAX - 1, INT32_MAX};
    for (int i = 0; i < 19; ++i)
      for (int j = 0; j < 19; ++j)
        for (int32_t a : kEdge) {
          yv4_conv_desc t = d;
          int32_t* g = &t.N;
          g[i] = a;
          if (j != i) g[j] = kEdge[(i + j) % 12];
          const int r = check_conv_desc(&t, e->who, e->rules);
          if (r != YV4_OK && r != YV4_E_INVALID && r != YV4_E_UNSUPPORTED) ++bad;
          ++perturbed;
        }
  }
  printf("%d records (%d by the descriptor check, %d by an entry's own rule, %d accepted; %d tightenings), %ld perturbed "
         "descriptors, %d mismatches\n", n, n_by[0], n_by[1], n_by[2], tightened, perturbed, bad);
  return bad || n == 0 ? 1 : 0;
}
