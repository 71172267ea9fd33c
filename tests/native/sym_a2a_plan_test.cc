// sym_a2a_plan_test.cc — CPU sweep of the cut the zero-copy AlltoAll / Gather kernel walks (device_abi.h symA2ACut /
// symA2APart, the SAME host-callable functions symA2AKernel and enqueue.cc planSymA2A call, so nothing of the
// arithmetic is restated here). Stand-alone: no library, no GPU.
//
//   sym_a2a_plan_test        B in {1, 15, 16, 17, 8202, 16384, 16385, 280004, 64 MiB} x channel caps {1, 3, 32, 256} x
//                            minCTAs {1, 2} x minChannelBytes {16, 4096, 16384}: the channel parts are disjoint and cover
//                            [0, B) exactly, in order; every part starts at a multiple of 16; nch lies within
//                            [min(max(minCTAs, 1), cap), cap] and is ceil(B / minChannelBytes) where that lies inside; and
//                            the cut is the same on every "rank" (the function is not given the rank: it is evaluated
//                            once per rank of a 16-rank communicator and compared). Prints "OK cases=<n> maxnch=<n>
//                            empty=<channels with an empty part>".
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
  const uint64_t sizes[] = {1, 15, 16, 17, 8202, 16384, 16385, 280004, (uint64_t)64 << 20};
  const int caps[] = {1, 3, 32, 256};
  const int minCTAs[] = {1, 2};
  const uint64_t minBytes[] = {16, 4096, 16384};
  int cases = 0, maxNch = 0;
  long empty = 0;
  for (uint64_t B : sizes)
    for (int cap : caps)
      for (int mc : minCTAs)
        for (uint64_t mb : minBytes) {
          cases++;
          const SymA2ACut cut = symA2ACut(B, mb, mc, cap);
          const int floorCh = mc < cap ? mc : cap;
          CHECK(cut.nch >= floorCh && cut.nch <= cap, "B=%lu cap=%d minCTAs=%d min=%lu: nch %d out of [%d, %d]",
                (unsigned long)B, cap, mc, (unsigned long)mb, cut.nch, floorCh, cap);
          const uint64_t want = (B + mb - 1) / mb;
          if (want >= (uint64_t)floorCh && want <= (uint64_t)cap)
            CHECK((uint64_t)cut.nch == want, "B=%lu min=%lu: nch %d, want %lu", (unsigned long)B, (unsigned long)mb,
                  cut.nch, (unsigned long)want);
          CHECK(cut.part % 16 == 0 && cut.part >= 16, "B=%lu: part %lu", (unsigned long)B, (unsigned long)cut.part);
          CHECK(cut.nch <= NCCL_AMD_MAX_CHANNELS, "nch %d beyond the channel arrays", cut.nch);
          maxNch = cut.nch > maxNch ? cut.nch : maxNch;
          // every rank of a 16-rank communicator cuts alike
          for (int rank = 0; rank < NCCL_AMD_MAX_RANKS; rank++) {
            const SymA2ACut other = symA2ACut(B, mb, mc, cap);
            CHECK(other.nch == cut.nch && other.part == cut.part, "rank %d cuts B=%lu differently", rank, (unsigned long)B);
          }
          // the parts, in channel order, tile [0, B) exactly once
          uint64_t at = 0;
          for (int c = 0; c < cut.nch; c++) {
            uint64_t lo, hi;
            symA2APart(cut.part, c, B, lo, hi);
            CHECK(lo <= hi && hi <= B, "B=%lu c=%d: [%lu, %lu)", (unsigned long)B, c, (unsigned long)lo, (unsigned long)hi);
            if (hi == lo) {
              empty++;
              continue;
            }
            CHECK(lo == at, "B=%lu c=%d: starts at %lu, the previous part ended at %lu", (unsigned long)B, c,
                  (unsigned long)lo, (unsigned long)at);
            CHECK(lo % 16 == 0, "B=%lu c=%d: start %lu is no multiple of 16", (unsigned long)B, c, (unsigned long)lo);
            CHECK(hi - lo <= cut.part, "B=%lu c=%d: %lu bytes in a part of %lu", (unsigned long)B, c,
                  (unsigned long)(hi - lo), (unsigned long)cut.part);
            at = hi;
          }
          CHECK(at == B, "B=%lu cap=%d minCTAs=%d min=%lu: parts end at %lu", (unsigned long)B, cap, mc, (unsigned long)mb,
                (unsigned long)at);
          // a channel past the launch owns nothing (the kernel's bound for any c)
          uint64_t lo, hi;
          symA2APart(cut.part, cut.nch, B, lo, hi);
          CHECK(lo == B && hi == B, "B=%lu: channel nch owns [%lu, %lu)", (unsigned long)B, (unsigned long)lo, (unsigned long)hi);
        }
  if (gFail) {
    printf("FAILED checks=%d\n", gFail);
    return 1;
  }
  printf("OK cases=%d maxnch=%d empty=%ld\n", cases, maxNch, empty);
  return 0;
}
