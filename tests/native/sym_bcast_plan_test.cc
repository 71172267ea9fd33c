// sym_bcast_plan_test.cc — CPU sweep of the cut the zero-copy Broadcast kernel walks (device_abi.h symBcastOwner /
// symBcastDirect / symBcastCut with blockLenOf / symA2APart, the SAME host-callable functions symBcastKernel and
// enqueue.cc planSymBcast call, so nothing of the arithmetic is restated here). Stand-alone: no library, no GPU.
//
//   sym_bcast_plan_test      n = 2..8 x every root x minChannelBytes {16, 4096, 16384} x channel caps {1, 3, 32, 256} x
//                            minCTAs {1, 2} x byte counts around 0, 16, the variant switch, block edges and
//                            channel-part edges, 8202, 300 001 and 64 MiB: the owner indices are a bijection of the
//                            non-roots; the variant is direct exactly when n == 2 or bytes < (n - 1) * minChannelBytes;
//                            blocks and channel parts, in (block, channel) order, tile [0, bytes) exactly once; every
//                            part starts at a multiple of 16 within its block; a channel past the launch owns nothing.
//                            Prints "OK cases=<n> direct=<n> twophase=<n> empty=<empty parts>".
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "../../nccl_amd/csrc/device_abi.h"

using namespace ncclamd;

static int gFail = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      printf("FAIL: " __VA_ARGS__); \
      printf("\n");                 \
      gFail++;                      \
    }                               \
  } while (0)

int main() {
  const int caps[] = {1, 3, 32, 256};
  const int minCTAs[] = {1, 2};
  const uint64_t minBytes[] = {16, 4096, 16384};
  long cases = 0, nDirect = 0, nTwoPhase = 0, empty = 0;
  for (int n = 2; n <= 8; n++) {
    for (int root = 0; root < n; root++) {  // owner indices: the non-roots onto [0, n - 1), the root onto n - 1
      std::vector<int> seen(n, 0);
      for (int r = 0; r < n; r++) {
        const int q = symBcastOwner(r, root, n);
        CHECK(q >= 0 && q < n && (q == n - 1) == (r == root), "n=%d root=%d: rank %d owns %d", n, root, r, q);
        if (q >= 0 && q < n) seen[q]++;
      }
      for (int q = 0; q < n; q++) CHECK(seen[q] == 1, "n=%d root=%d: owner index %d taken %d times", n, root, q, seen[q]);
    }
    for (uint64_t mb : minBytes) {
      const uint64_t sw = (uint64_t)(n - 1) * mb;  // the variant switch
      std::vector<uint64_t> sizes = {0, 1, 15, 16, 17, 8202, 300001, (uint64_t)64 << 20, sw - 1, sw, sw + 1};
      for (uint64_t k : {(uint64_t)1, (uint64_t)2, (uint64_t)37})  // block edges: n - 1 full blocks of 16 k bytes
        for (int d = -1; d <= 1; d++) sizes.push_back((uint64_t)(n - 1) * 16 * k + d);
      for (int d = -1; d <= 1; d++) sizes.push_back(3 * sw + d);  // channel-part edges: blocks of 3 minimum parts
      for (uint64_t bytes : sizes)
        for (int cap : caps)
          for (int mc : minCTAs) {
            cases++;
            const bool direct = symBcastDirect(bytes, n, mb);
            CHECK(direct == (n == 2 || bytes < sw), "n=%d bytes=%lu min=%lu: direct %d", n, (unsigned long)bytes,
                  (unsigned long)mb, (int)direct);
            (direct ? nDirect : nTwoPhase)++;
            const SymBcastCut cut = symBcastCut(bytes, n, direct, mb, mc, cap);
            const uint64_t perOwner = (bytes + n - 2) / (n - 1);
            CHECK(cut.blocks == (direct ? 1 : n - 1) && cut.block == (direct ? bytes : (perOwner + 15) / 16 * 16),
                  "n=%d bytes=%lu: %d blocks of %lu", n, (unsigned long)bytes, cut.blocks, (unsigned long)cut.block);
            CHECK(cut.nch >= (mc < cap ? mc : cap) && cut.nch <= cap && cut.nch <= NCCL_AMD_MAX_CHANNELS,
                  "n=%d bytes=%lu cap=%d minCTAs=%d: nch %d", n, (unsigned long)bytes, cap, mc, cut.nch);
            CHECK(cut.part % 16 == 0, "n=%d bytes=%lu: part %lu", n, (unsigned long)bytes, (unsigned long)cut.part);
            // blocks in order, and within each block the channel parts in order, tile [0, bytes) exactly once
            uint64_t at = 0;
            for (int q = 0; q < cut.blocks; q++) {
              const uint64_t len = blockLenOf(bytes, cut.block, q);
              for (int c = 0; c <= cut.nch; c++) {  // c == nch: a channel past the launch owns nothing
                uint64_t lo, hi;
                symA2APart(cut.part, c, len, lo, hi);
                CHECK(lo <= hi && hi <= len, "n=%d bytes=%lu q=%d c=%d: [%lu, %lu) of %lu", n, (unsigned long)bytes, q, c,
                      (unsigned long)lo, (unsigned long)hi, (unsigned long)len);
                if (hi == lo) {
                  empty += c < cut.nch;
                  continue;
                }
                CHECK(c < cut.nch, "n=%d bytes=%lu q=%d: channel nch owns bytes", n, (unsigned long)bytes, q);
                CHECK((uint64_t)q * cut.block + lo == at, "n=%d bytes=%lu q=%d c=%d: starts at %lu, the previous part "
                      "ended at %lu", n, (unsigned long)bytes, q, c, (unsigned long)((uint64_t)q * cut.block + lo),
                      (unsigned long)at);
                CHECK(lo % 16 == 0, "n=%d bytes=%lu q=%d c=%d: start %lu is no multiple of 16", n, (unsigned long)bytes,
                      q, c, (unsigned long)lo);
                at = (uint64_t)q * cut.block + hi;
              }
            }
            CHECK(at == bytes, "n=%d bytes=%lu cap=%d minCTAs=%d min=%lu: parts end at %lu", n, (unsigned long)bytes, cap,
                  mc, (unsigned long)mb, (unsigned long)at);
          }
    }
  }
  if (gFail) {
    printf("FAILED checks=%d\n", gFail);
    return 1;
  }
  printf("OK cases=%ld direct=%ld twophase=%ld empty=%ld\n", cases, nDirect, nTwoPhase, empty);
  return 0;
}
