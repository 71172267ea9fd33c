// CPU sweep of the host-visible half of the device API's reduce-copy addition (include/nccl_device.h ncclSymPtr,
// include/nccl_device_reduce_copy.h ncclReduceCopyPlan / ncclReduceCopyRoundElts): a stand-alone host program, plain
// C++17, built under ASan+UBSan. Prints OK at the end; the first failed check prints its line and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "nccl.h"
#include "nccl_device.h"

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

template <typename T, typename Int>
static void stepsOf(ncclWindow_t w) {
  const size_t base = 4096;
  ncclSymPtr<T> p(w, base);
  p += (Int)5;
  CHECK(p.window == w && p.offset == base + 5 * sizeof(T));
  p -= (Int)3;
  CHECK(p.offset == base + 2 * sizeof(T));
  ncclSymPtr<T> q = p + (Int)7;
  CHECK(q.offset == base + 9 * sizeof(T) && p.offset == base + 2 * sizeof(T));
  q = q - (Int)9;
  CHECK(q.offset == base && q.window == w);
  CHECK(q - p == -2 && p - q == 2);
  if (std::is_signed<Int>::value) {  // negative steps
    ncclSymPtr<T> r(w, base);
    r += (Int)-4;
    CHECK(r.offset == base - 4 * sizeof(T));
    r -= (Int)-6;
    CHECK(r.offset == base + 2 * sizeof(T));
    CHECK((r + (Int)-2).offset == base && (r - (Int)-1).offset == base + 3 * sizeof(T));
    CHECK((r + (Int)-2) - r == -2);
  }
}

template <typename T>
static void symPtrOf(ncclWindow_t w, ncclWindow_t other) {
  stepsOf<T, int>(w);
  stepsOf<T, unsigned int>(w);
  stepsOf<T, long>(w);
  stepsOf<T, unsigned long>(w);
  stepsOf<T, long long>(w);
  stepsOf<T, unsigned long long>(w);
  constexpr ncclSymPtr<T> null;
  static_assert(null.window == nullptr && null.offset == 0, "the default ncclSymPtr is (nullptr, 0)");
  const ncclSymPtr<T> a(w, 64), b(w, 64), c(w, 64 + sizeof(T)), d(other, 64);
  CHECK(a == b && !(a != b));
  CHECK(a != c && !(a == c));
  CHECK(a != d && !(a == d));  // the same offset in another window
  CHECK(c - a == 1 && a - c == -1);
  const ncclSymPtr<unsigned char> bytes = c;  // conversion keeps window and byte offset
  CHECK(bytes.window == w && bytes.offset == 64 + sizeof(T));
  const ncclSymPtr<T> back = bytes;
  CHECK(back == c);
  static_assert(std::is_same<typename ncclSymPtr<T>::ElementType, T>::value, "ElementType");
  static_assert(std::is_same<decltype(a == b), bool>::value && std::is_same<decltype(a != b), bool>::value, "bool");
  static_assert(std::is_same<decltype(a - b), ptrdiff_t>::value, "ptrdiff_t");
}

struct Wide {
  char bytes[24];
};

// One plan against its definition, for pointers with the low address bits lows[0..n).
static void checkPlan(const unsigned* lows, int n, unsigned eltSize, size_t count) {
  uintptr_t orBits = 0, andBits = ~(uintptr_t)0;
  for (int i = 0; i < n; i++) {
    orBits |= 0x1000u + lows[i];
    andBits &= 0x1000u + lows[i];
  }
  const ncclReduceCopySegments s = ncclReduceCopyPlan(lows[0], ncclReduceCopyRelBits(orBits, andBits), eltSize, count);
  CHECK(s.prefix + s.elts16 + s.elts4 + s.tail == count);  // the four tile [0, count) in order
  CHECK(s.elts16 % (16 / eltSize) == 0);
  CHECK(eltSize >= 4 ? s.elts4 == 0 : s.elts4 % (4 / eltSize) == 0);
  const size_t at16 = s.prefix * eltSize, at4 = (s.prefix + s.elts16) * eltSize;
  bool all16 = true, all4 = true;
  for (int i = 0; i < n; i++) {
    if (s.elts16) CHECK((lows[i] + at16) % 16 == 0);
    if (s.elts4) CHECK((lows[i] + at4) % 4 == 0);
    all16 = all16 && lows[i] == lows[0];
    all4 = all4 && lows[i] % 4 == lows[0] % 4;
  }
  // the prefix is shorter than one pack of the widest path taken, and no wider path was possible from it on
  if (all16) {
    CHECK(s.prefix * eltSize < 16);
    CHECK(s.prefix == count || (lows[0] + at16) % 16 == 0);
    CHECK(s.elts16 == (count - s.prefix) / (16 / eltSize) * (16 / eltSize));
    const size_t rest = count - s.prefix - s.elts16;
    if (eltSize < 4) CHECK(s.elts4 == rest / (4 / eltSize) * (4 / eltSize) && s.tail * eltSize < 4);
    else CHECK(s.tail * eltSize < 16);
  } else if (all4 && eltSize < 4) {
    CHECK(s.elts16 == 0 && s.prefix * eltSize < 4 && s.tail * eltSize < 4);
    CHECK(s.prefix == count || (lows[0] + at4) % 4 == 0);
  } else {
    CHECK(s.prefix == 0 && s.elts16 == 0 && s.elts4 == 0 && s.tail == count);
  }
}

int main() {
  static ncclWindow_vidmem tables[2];
  for (int t = 0; t < 2; t++) {
    tables[t].nRanks = 4;
    tables[t].rank = 1;
    for (int r = 0; r < 4; r++) {
      tables[t].peerPtr[r] = (char*)(uintptr_t)(0x100000u * (unsigned)(4 * t + r + 1));
      tables[t].peerSize[r] = 1 << 16;
    }
  }
  symPtrOf<signed char>(&tables[0], &tables[1]);
  symPtrOf<unsigned short>(&tables[0], &tables[1]);
  symPtrOf<float>(&tables[0], &tables[1]);
  symPtrOf<double>(&tables[0], &tables[1]);
  symPtrOf<Wide>(&tables[0], &tables[1]);

  // the plan: every element size, every pair of low-address patterns (source, destination) and every triple of them
  // in steps of the element size, every count 0..200 and a few large ones
  const size_t large[] = {4095, 4096, 4097, ((size_t)1 << 31) - 1, ((size_t)1 << 31) + 5, ((size_t)1 << 40) + 3};
  size_t plans = 0;
  for (unsigned eltSize = 1; eltSize <= 8; eltSize *= 2)
    for (unsigned a = 0; a < 16; a += eltSize)
      for (unsigned b = 0; b < 16; b += eltSize) {
        const unsigned two[2] = {a, b};
        for (size_t count = 0; count <= 200; count++, plans++) checkPlan(two, 2, eltSize, count);
        for (size_t count : large) checkPlan(two, 2, eltSize, count);
        for (unsigned c = 0; c < 16; c += eltSize) {
          const unsigned three[3] = {a, b, c};
          for (size_t count = 0; count <= 200; count += 7, plans++) checkPlan(three, 3, eltSize, count);
        }
      }
  const unsigned one[1] = {6};
  checkPlan(one, 1, 2, 100);

  // P, the elements of one round: coop size x packs per thread x elements per 16-byte pack
  static_assert(ncclReduceCopyRoundElts(4, 256, 16) == 256 * 4 * 4, "float, CTA of 256, default UNROLL");
  static_assert(ncclReduceCopyRoundElts(2, 64, 32) == 64 * 4 * 8, "2-byte, one wave, default UNROLL");
  static_assert(ncclReduceCopyRoundElts(1, 1, 64) == 16, "a thread coop takes one pack per round");
  static_assert(ncclReduceCopyPacksPerThread(4, 64, 4) == 1 && ncclReduceCopyPacksPerThread(4, 64, 1) == 1 &&
                    ncclReduceCopyPacksPerThread(4, 64, 8) == 2 && ncclReduceCopyPacksPerThread(8, 64, 1000) == 4,
                "UNROLL is clamped to 1..4 packs");

  printf("plans=%zu sizeof(ncclSymPtr<float>)=%zu\nOK\n", plans, sizeof(ncclSymPtr<float>));
  return 0;
}
