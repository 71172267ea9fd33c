/*
 * nccl_device_reduce_copy.h — the data-movement half of the device API: reduce N sources into M destinations between
 * two barriers of the caller's own kernel. Names, template-parameter order and argument order are the reference's
 * (src/include/nccl_device/reduce_copy.h), so a kernel written against it compiles unchanged; the implementation is
 * this project's own, written for gfx950 (DESIGN.md §2.7 "Reduce-copy"). Included by nccl_device.h.
 *
 * Semantics. For every element index e < count, every destination gets
 *     cast<T>( fold_{i = 0 .. nSrc-1} cast<Acc>(src_i[e]) )
 * folded in source-index order in the accumulate type Acc with one rounding at the end: Acc = float for __half and
 * __hip_bfloat16 under OpSum (round-to-nearest-even when packing), Acc = T otherwise and for every user RedOp.
 * Integer sums wrap. nSrc == 1 is a bit-preserving copy. count == 0, nSrc == 0 or nDst == 0 do nothing.
 * Types: int8, uint8, int32, uint32, int64, uint64, float, double, __half, __hip_bfloat16 (any trivially copyable T
 * of 1, 2, 4 or 8 bytes works with a user RedOp). fp8 is refused at compile time: the reference accumulates it in half.
 *
 * Contract. Every thread of the coop calls with the same arguments, converged. Sources and destinations are global
 * memory (windows, device or mapped host allocations; not LDS). Pointers need alignof(T) only. A
 * destination may be exactly one of the sources (the in-place AllReduce: a thread reads all sources of an element
 * before it writes the element anywhere); any other overlap is undefined. The functions are plain loads and stores:
 * no fence, no flag, no spin. Visibility is the job of the caller's barriers — acquire before, release after.
 *
 * Shape of the loop. All source and destination pointers are resolved once, before the loop (one window-table read per
 * peer for the window and ncclSymPtr forms), into registers: at most NCCL_DEVICE_REDUCE_COPY_MAX_PTRS of each; a call
 * with more sources or destinations takes an element-at-a-time loop that asks the lambdas again. ncclReduceCopyPlan
 * cuts [0, count) into a scalar prefix, 16-byte packs, 4-byte packs and a scalar tail from the pointers' low bits. In
 * a round of the 16-byte path, thread t of a coop of S threads takes packs t, t + S, ..., t + (U-1)·S: consecutive
 * lanes take consecutive packs, so one wave's access covers 64 consecutive packs (1 KiB). All U loads of a source are
 * issued before the first is consumed, and the sources are loaded four at a time. Whole rounds run unchecked; what is
 * left of the segment, the 4-byte packs and the scalar elements run one access per thread.
 *
 * UNROLL (elements per thread and round) stays in every signature. It is clamped: U = UNROLL·sizeof(T)/16 16-byte
 * packs per thread, at least 1 and at most NCCL_DEVICE_REDUCE_COPY_MAX_PACKS (the default, 4·16/sizeof(T), gives 4);
 * a thread coop, which coalesces nothing, takes 1. ncclReduceCopyRoundElts is the resulting element count of a round.
 *
 * Registers: 4 packs of 4 sources in flight plus the accumulators are 100-150 VGPRs in the compiler's report for the
 * test kernels. Give the kernel __launch_bounds__(512) or less; under the default bound of 1024 threads the compiler
 * has 128 registers per lane.
 */
#ifndef NCCL_DEVICE_REDUCE_COPY_H_
#define NCCL_DEVICE_REDUCE_COPY_H_

#ifndef NCCL_DEVICE_H_
#error "include nccl_device.h, not this header"
#endif

#include <stdint.h>

/* Pointers of each kind (sources, destinations) kept in registers. */
#define NCCL_DEVICE_REDUCE_COPY_MAX_PTRS 16
/* 16-byte packs per thread and round, the clamp of UNROLL. */
#define NCCL_DEVICE_REDUCE_COPY_MAX_PACKS 4

/* --------------------------------------------------------------------------------------------- the plan */

/* [0, count) in elements, in this order: a scalar prefix, elts16 elements in 16-byte packs, elts4 elements in 4-byte
 * packs, a scalar tail. */
struct ncclReduceCopySegments {
  size_t prefix, elts16, elts4, tail;
};

/* Pure. lowBits: the first pointer's address mod 16 (a multiple of eltSize). relBits: the bits of the addresses mod 16
 * in which the source and destination pointers are not all alike — zero when all pointers are congruent mod 16, a
 * multiple of 4 when they are congruent mod 4 (ncclReduceCopyRelBits makes it). eltSize: 1, 2, 4 or 8.
 *   congruent mod 16: prefix up to the first 16-byte boundary (fewer than 16/eltSize elements), 16-byte packs, then —
 *                     eltSize < 4 — 4-byte packs, then the tail;
 *   congruent mod 4 only, eltSize < 4: prefix up to the first 4-byte boundary, 4-byte packs, the tail;
 *   otherwise: everything is tail. A 4-byte pack of a 4- or 8-byte type would be one element or none, which is what
 *   the scalar loop moves: elts4 is 0 for them. */
NCCL_HOST_DEVICE_INLINE ncclReduceCopySegments ncclReduceCopyPlan(unsigned lowBits, unsigned relBits, unsigned eltSize,
                                                                  size_t count) {
  ncclReduceCopySegments s;
  s.prefix = s.elts16 = s.elts4 = 0;
  lowBits &= 15u;
  relBits &= 15u;
  size_t rest = count;
  if (relBits == 0) {
    size_t pre = ((16u - lowBits) & 15u) / eltSize;
    if (pre > rest) pre = rest;
    s.prefix = pre;
    rest -= pre;
    const size_t per16 = 16u / eltSize;
    s.elts16 = rest / per16 * per16;
    rest -= s.elts16;
    if (eltSize < 4) {
      const size_t per4 = 4u / eltSize;
      s.elts4 = rest / per4 * per4;
      rest -= s.elts4;
    }
  } else if (eltSize < 4 && relBits % 4u == 0) {
    size_t pre = ((4u - lowBits % 4u) & 3u) / eltSize;
    if (pre > rest) pre = rest;
    s.prefix = pre;
    rest -= pre;
    const size_t per4 = 4u / eltSize;
    s.elts4 = rest / per4 * per4;
    rest -= s.elts4;
  }
  s.tail = rest;
  return s;
}

/* relBits from the OR and the AND of all pointers' addresses: the low bits in which they are not all alike. */
NCCL_HOST_DEVICE_INLINE unsigned ncclReduceCopyRelBits(uintptr_t orOfAddrs, uintptr_t andOfAddrs) {
  return (unsigned)((orOfAddrs ^ andOfAddrs) & 15u);
}

/* 16-byte packs per thread and round for elements of eltSize bytes, a coop of coopSize threads and the signature's
 * UNROLL. A coop of one thread (ncclCoopThread) coalesces nothing and takes one pack per round. */
NCCL_HOST_DEVICE_INLINE constexpr int ncclReduceCopyPacksPerThread(size_t eltSize, int coopSize, int unroll) {
  return coopSize == 1 || (size_t)unroll * eltSize / 16 < 1
             ? 1
             : ((size_t)unroll * eltSize / 16 > NCCL_DEVICE_REDUCE_COPY_MAX_PACKS ? NCCL_DEVICE_REDUCE_COPY_MAX_PACKS
                                                                                   : (int)((size_t)unroll * eltSize / 16));
}

/* P: the elements one round of the 16-byte path moves, for a coop of coopSize threads. */
NCCL_HOST_DEVICE_INLINE constexpr size_t ncclReduceCopyRoundElts(size_t eltSize, int coopSize, int unroll) {
  return (size_t)coopSize * (size_t)ncclReduceCopyPacksPerThread(eltSize, coopSize, unroll) * (16 / eltSize);
}

/* ------------------------------------------------------------------------------------- device functions */
#if defined(__HIPCC__)

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

struct __hip_fp8_e4m3;
struct __hip_fp8_e5m2;
struct __hip_fp8_e4m3_fnuz;
struct __hip_fp8_e5m2_fnuz;

namespace nccl {
namespace utility {

/* The sum a RedOp-taking function is given by the ncclLsaReduceSum* forms. */
template <typename T>
struct OpSum {
  using EltType = T;
  __host__ __device__ __forceinline__ T operator()(T const& a, T const& b) const {
    if constexpr (std::is_integral<T>::value) {
      using U = typename std::make_unsigned<T>::type;
      return (T)(U)((U)a + (U)b); /* wraps */
    } else {
      return a + b;
    }
  }
};

namespace rc {

template <typename T>
struct IsFp8 : std::false_type {};
template <>
struct IsFp8<__hip_fp8_e4m3> : std::true_type {};
template <>
struct IsFp8<__hip_fp8_e5m2> : std::true_type {};
template <>
struct IsFp8<__hip_fp8_e4m3_fnuz> : std::true_type {};
template <>
struct IsFp8<__hip_fp8_e5m2_fnuz> : std::true_type {};

/* How a RedOp folds: the accumulate type, the casts into and out of it, one step. */
template <typename RedOp>
struct Fold {
  using Elt = typename RedOp::EltType;
  using Acc = Elt;
  static NCCL_DEVICE_INLINE Acc up(Elt const& x) { return x; }
  static NCCL_DEVICE_INLINE Elt down(Acc const& a) { return a; }
  static NCCL_DEVICE_INLINE Acc step(RedOp const& op, Acc const& a, Acc const& b) { return op(a, b); }
};
template <>
struct Fold<OpSum<__half>> {
  using Elt = __half;
  using Acc = float;
  static NCCL_DEVICE_INLINE Acc up(Elt const& x) { return __half2float(x); }
  static NCCL_DEVICE_INLINE Elt down(Acc const& a) { return __float2half(a); } /* v_cvt_f16_f32: nearest even */
  static NCCL_DEVICE_INLINE Acc step(OpSum<__half> const&, Acc const& a, Acc const& b) { return a + b; }
};
template <>
struct Fold<OpSum<__hip_bfloat16>> {
  using Elt = __hip_bfloat16;
  using Acc = float;
  static NCCL_DEVICE_INLINE Acc up(Elt const& x) {
    unsigned short b;
    __builtin_memcpy(&b, &x, 2);
    return __uint_as_float((unsigned)b << 16);
  }
  static NCCL_DEVICE_INLINE Elt down(Acc const& a) {
    unsigned u = __float_as_uint(a);
    unsigned short b;
    if ((u & 0x7fffffffu) > 0x7f800000u) b = (unsigned short)((u >> 16) | 0x0040u); /* a quiet NaN */
    else b = (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);              /* nearest even */
    Elt x;
    __builtin_memcpy(&x, &b, 2);
    return x;
  }
  static NCCL_DEVICE_INLINE Acc step(OpSum<__hip_bfloat16> const&, Acc const& a, Acc const& b) { return a + b; }
};

/* What one access moves. may_alias: the memory is the caller's array of T. */
template <int BYTES>
struct Word;
template <>
struct Word<16> {
  typedef unsigned int type __attribute__((ext_vector_type(4), may_alias));
};
template <>
struct Word<8> {
  typedef unsigned long long type __attribute__((may_alias));
};
template <>
struct Word<4> {
  typedef unsigned int type __attribute__((may_alias));
};
template <>
struct Word<2> {
  typedef unsigned short type __attribute__((may_alias));
};
template <>
struct Word<1> {
  typedef unsigned char type;
};

/* Where the resolved pointers live. A wave coop (warp, CTA) keeps pointer i in lane i of two VGPRs and reads it back
 * with v_readlane, which takes a wave-uniform index and ignores EXEC: 4 VGPRs hold all 32 pointers, and a pointer
 * comes back as an SGPR pair. Lanes 0..15 of the wave must be active to take their pointers. A wave without them (the
 * partial last wave of a CTA whose size mod 64 is 1..15) and a thread coop, where nothing is uniform, keep all 16 in a
 * register vector per lane (indexed registers, not an array, which a dynamic index would put into scratch). */
template <typename T, bool PER_THREAD>
struct Table {
  int lo = 0, hi = 0;
  template <typename Lambda>
  NCCL_DEVICE_INLINE void fill(Lambda lambda, int n, uintptr_t& orBits, uintptr_t& andBits) {
    const int lane = (int)__lane_id();
    for (int i = 0; i < n; i++) {
      const uintptr_t a = (uintptr_t)lambda(i);
      if (lane == i) {
        lo = (int)(unsigned)a;
        hi = (int)(unsigned)(a >> 32);
      }
      orBits |= a;
      andBits &= a;
    }
  }
  NCCL_DEVICE_INLINE char* get(int i) const {
    return (char*)(((uintptr_t)(unsigned)__builtin_amdgcn_readlane(hi, i) << 32) |
                   (uintptr_t)(unsigned)__builtin_amdgcn_readlane(lo, i));
  }
};
template <typename T>
struct Table<T, true> {
  /* a vector, not an array: a dynamic index into it is register indexing, never memory */
  typedef unsigned long long Vec __attribute__((ext_vector_type(NCCL_DEVICE_REDUCE_COPY_MAX_PTRS)));
  Vec p;
  template <typename Lambda>
  NCCL_DEVICE_INLINE void fill(Lambda lambda, int n, uintptr_t& orBits, uintptr_t& andBits) {
#pragma unroll
    for (int i = 0; i < NCCL_DEVICE_REDUCE_COPY_MAX_PTRS; i++) {
      uintptr_t a = 0;
      if (i < n) {
        a = (uintptr_t)lambda(i);
        orBits |= a;
        andBits &= a;
      }
      /* Through VGPRs even where the caller's arguments happen to be uniform: 32 uniform pointers would be kept in
       * 64 of the wave's ~100 SGPRs and push everything else out of them. */
      unsigned lo = (unsigned)a, hi = (unsigned)(a >> 32);
      asm volatile("" : "+v"(lo), "+v"(hi));
      p[i] = ((unsigned long long)hi << 32) | lo;
    }
  }
  NCCL_DEVICE_INLINE char* get(int i) const { return (char*)(uintptr_t)p[i]; }
};

/* U accesses of BYTES bytes per thread, `stride` bytes apart from byte `at` on, through all sources and destinations:
 * source 0, then the other sources four at a time (their 4·U loads are issued before the first is folded), then every
 * destination. */
template <typename T, typename RedOp, int BYTES, int U, typename Tbl>
NCCL_DEVICE_INLINE void move(Tbl const& src, int nSrc, Tbl const& dst, int nDst, RedOp const& op, size_t at,
                             size_t stride) {
  using W = typename Word<BYTES>::type;
  typedef W GW __attribute__((address_space(1))); /* global memory: global_load / global_store, not flat */
  using F = Fold<RedOp>;
  using Acc = typename F::Acc;
  constexpr int N = BYTES / (int)sizeof(T);
  constexpr int G = 4;
  W raw[U];
  {
    const char* p = src.get(0) + at;
#pragma unroll
    for (int u = 0; u < U; u++) raw[u] = *(const GW*)(uintptr_t)(p + u * stride);
  }
  if (nSrc > 1) {
    Acc acc[U][N];
#pragma unroll
    for (int u = 0; u < U; u++) {
      T e[N];
      __builtin_memcpy(e, &raw[u], BYTES);
#pragma unroll
      for (int j = 0; j < N; j++) acc[u][j] = F::up(e[j]);
    }
    for (int g = 1; g < nSrc; g += G) {
      const int m = nSrc - g; /* sources left, this group takes min(m, G) */
      W in[G][U];
#pragma unroll
      for (int k = 0; k < G; k++) {
        if (k < m) {
          const char* p = src.get(g + k) + at;
#pragma unroll
          for (int u = 0; u < U; u++) in[k][u] = *(const GW*)(uintptr_t)(p + u * stride);
        }
      }
#pragma unroll
      for (int k = 0; k < G; k++) {
        if (k < m) {
#pragma unroll
          for (int u = 0; u < U; u++) {
            T e[N];
            __builtin_memcpy(e, &in[k][u], BYTES);
#pragma unroll
            for (int j = 0; j < N; j++) acc[u][j] = F::step(op, acc[u][j], F::up(e[j]));
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      T e[N];
#pragma unroll
      for (int j = 0; j < N; j++) e[j] = F::down(acc[u][j]);
      __builtin_memcpy(&raw[u], e, BYTES);
    }
  }
  for (int d = 0; d < nDst; d++) {
    char* p = dst.get(d) + at;
#pragma unroll
    for (int u = 0; u < U; u++) *(GW*)(uintptr_t)(p + u * stride) = raw[u];
  }
}

/* nPacks accesses of BYTES bytes from byte `base` on: whole rounds of U per thread, then one per thread. */
template <typename T, typename RedOp, int BYTES, int U, typename Tbl>
NCCL_DEVICE_INLINE void segment(Tbl const& src, int nSrc, Tbl const& dst, int nDst, RedOp const& op, size_t base,
                                size_t nPacks, size_t tr, size_t coopSize) {
  size_t b = 0;
  if constexpr (U > 1) {
    const size_t round = coopSize * U;
    for (; b + round <= nPacks; b += round)
      move<T, RedOp, BYTES, U>(src, nSrc, dst, nDst, op, base + (b + tr) * BYTES, coopSize * BYTES);
  }
  for (size_t i = b + tr; i < nPacks; i += coopSize)
    move<T, RedOp, BYTES, 1>(src, nSrc, dst, nDst, op, base + i * BYTES, 0);
}

/* The resolved-pointer path: fill the tables, plan, walk the four segments. */
template <typename T, typename RedOp, int U, typename Tbl, typename SrcLambda, typename DstLambda>
NCCL_DEVICE_INLINE void run(SrcLambda srcLambda, int nSrc, DstLambda dstLambda, int nDst, RedOp const& op, size_t count,
                            size_t tr, size_t coopSize) {
  Tbl src, dst;
  uintptr_t orBits = 0, andBits = ~(uintptr_t)0;
  src.fill(srcLambda, nSrc, orBits, andBits);
  dst.fill(dstLambda, nDst, orBits, andBits);
  const ncclReduceCopySegments plan = ncclReduceCopyPlan((unsigned)((uintptr_t)src.get(0) & 15u),
                                                         ncclReduceCopyRelBits(orBits, andBits),
                                                         (unsigned)sizeof(T), count);

  size_t at = plan.prefix * sizeof(T);
  if (plan.elts16)
    segment<T, RedOp, 16, U>(src, nSrc, dst, nDst, op, at, plan.elts16 * sizeof(T) / 16, tr, coopSize);
  at += plan.elts16 * sizeof(T);
  if constexpr (sizeof(T) < 4) {
    if (plan.elts4)
      segment<T, RedOp, 4, 1>(src, nSrc, dst, nDst, op, at, plan.elts4 * sizeof(T) / 4, tr, coopSize);
  }
  /* prefix and tail, one element per thread */
  const size_t nScalar = plan.prefix + plan.tail, tailAt = count - plan.tail;
  for (size_t i = tr; i < nScalar; i += coopSize) {
    const size_t e = i < plan.prefix ? i : i - plan.prefix + tailAt;
    move<T, RedOp, (int)sizeof(T), 1>(src, nSrc, dst, nDst, op, e * sizeof(T), 0);
  }
}

template <typename T, typename RedOp, int UNROLL, typename Coop, typename SrcLambda, typename DstLambda>
NCCL_DEVICE_INLINE void reduceCopy(Coop coop, SrcLambda srcLambda, int nSrc, DstLambda dstLambda, int nDst,
                                   RedOp const& op, size_t count) {
  static_assert(!IsFp8<T>::value,
                "reduce-copy of fp8 is not provided: the reference accumulates it in half, which needs its own parity");
  static_assert(sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8,
                "reduce-copy moves elements of 1, 2, 4 or 8 bytes");
  static_assert(std::is_same<typename RedOp::EltType, T>::value, "RedOp::EltType must be T");
  using F = Fold<RedOp>;
  if (count == 0 || nSrc <= 0 || nDst <= 0) return;
  const size_t tr = (size_t)coop.thread_rank(), coopSize = (size_t)coop.size();

  if (nSrc > NCCL_DEVICE_REDUCE_COPY_MAX_PTRS || nDst > NCCL_DEVICE_REDUCE_COPY_MAX_PTRS) {
    for (size_t e = tr; e < count; e += coopSize) {
      T v = srcLambda(0)[e];
      if (nSrc > 1) {
        typename F::Acc acc = F::up(v);
        for (int s = 1; s < nSrc; s++) acc = F::step(op, acc, F::up(srcLambda(s)[e]));
        v = F::down(acc);
      }
      for (int d = 0; d < nDst; d++) dstLambda(d)[e] = v;
    }
    return;
  }

  if constexpr (std::is_same<Coop, ncclCoopThread>::value) {
    run<T, RedOp, 1, Table<T, true>>(srcLambda, nSrc, dstLambda, nDst, op, count, tr, coopSize);
  } else {
    constexpr int U = ncclReduceCopyPacksPerThread(sizeof(T), 64, UNROLL);
    if constexpr (!std::is_same<Coop, ncclCoopWarp>::value) {
      /* A CTA's partial last wave of fewer than 16 threads has no lanes to keep the pointers in: it walks the same
       * plan with the per-lane table. */
      if ((__builtin_amdgcn_read_exec() & 0xffffull) != 0xffffull) {
        run<T, RedOp, U, Table<T, true>>(srcLambda, nSrc, dstLambda, nDst, op, count, tr, coopSize);
        return;
      }
    }
    run<T, RedOp, U, Table<T, false>>(srcLambda, nSrc, dstLambda, nDst, op, count, tr, coopSize);
  }
}

}  // namespace rc
}  // namespace utility
}  // namespace nccl

#define NCCL_RC_UNROLL(T) (4 * 16 / (int)sizeof(T))
#define NCCL_RC_INTEGRAL(Int) typename = std::enable_if_t<std::is_integral<Int>::value>

/* ---- series 1: any RedOp { using EltType = T; T operator()(T const&, T const&) const; }, lambdas i -> T* ---- */
template <typename T, typename Coop, typename SrcLambda, typename DstLambda, typename RedOp, typename IntCount,
          int UNROLL = NCCL_RC_UNROLL(T), NCCL_RC_INTEGRAL(IntCount)>
NCCL_DEVICE_INLINE void ncclLsaReduceLsaCopy(Coop coop, SrcLambda srcLambda, int nSrc, DstLambda dstLambda, int nDst,
                                             RedOp const& redOp, IntCount count) {
  if (count <= 0) return;
  nccl::utility::rc::reduceCopy<T, RedOp, UNROLL>(coop, srcLambda, nSrc, dstLambda, nDst, redOp, (size_t)count);
}

/* ---- series 2: the sum ---- */
template <typename T, typename Coop, typename SrcLambda, typename DstLambda, typename IntCount,
          int UNROLL = NCCL_RC_UNROLL(T), NCCL_RC_INTEGRAL(IntCount)>
NCCL_DEVICE_INLINE void ncclLsaReduceSumLsaCopy(Coop coop, SrcLambda srcLambda, int nSrc, DstLambda dstLambda, int nDst,
                                                IntCount count) {
  ncclLsaReduceLsaCopy<T, Coop, SrcLambda, DstLambda, nccl::utility::OpSum<T>, IntCount, UNROLL>(
      coop, srcLambda, nSrc, dstLambda, nDst, nccl::utility::OpSum<T>{}, count);
}

/* ---- series 3: N sources -> one local destination ---- */
template <typename T, typename Coop, typename SrcLambda, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T),
          NCCL_RC_INTEGRAL(IntCount)>
NCCL_DEVICE_INLINE void ncclLsaReduceSum(Coop coop, SrcLambda srcLambda, int nSrc, T* dstPtr, IntCount count) {
  auto dstLambda = [=](int) -> T* { return dstPtr; };
  ncclLsaReduceSumLsaCopy<T, Coop, SrcLambda, decltype(dstLambda), IntCount, UNROLL>(coop, srcLambda, nSrc, dstLambda,
                                                                                     1, count);
}
/* the team's members' windows, in team order */
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSum(Coop coop, ncclSymPtr<T> src, T* dstPtr, IntCount count, ncclTeam team) {
  auto srcLambda = [=](int i) -> T* { return src.peerPtr(team, i); };
  ncclLsaReduceSum<T, Coop, decltype(srcLambda), IntCount, UNROLL>(coop, srcLambda, team.nRanks, dstPtr, count);
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSum(Coop coop, ncclSymPtr<T> src, T* dstPtr, IntCount count,
                                         ncclDevComm const& devComm) {
  ncclLsaReduceSum<T, Coop, IntCount, UNROLL>(coop, src, dstPtr, count, ncclTeamLsa(devComm));
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSum(Coop coop, ncclWindow_t window, size_t offset, T* dstPtr, IntCount count,
                                         ncclTeam team) {
  ncclLsaReduceSum<T, Coop, IntCount, UNROLL>(coop, ncclSymPtr<T>(window, offset), dstPtr, count, team);
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSum(Coop coop, ncclWindow_t window, size_t offset, T* dstPtr, IntCount count,
                                         ncclDevComm const& devComm) {
  ncclLsaReduceSum<T, Coop, IntCount, UNROLL>(coop, ncclSymPtr<T>(window, offset), dstPtr, count,
                                              ncclTeamLsa(devComm));
}
template <typename T, typename Coop, typename SrcLambda, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T),
          NCCL_RC_INTEGRAL(IntCount)>
NCCL_DEVICE_INLINE void ncclLocalReduceSum(Coop coop, SrcLambda srcLambda, int nSrc, T* dstPtr, IntCount count) {
  ncclLsaReduceSum<T, Coop, SrcLambda, IntCount, UNROLL>(coop, srcLambda, nSrc, dstPtr, count);
}
/* source i is basePtr + i·displ (displ in elements) */
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLocalReduceSum(Coop coop, int nSrc, T* basePtr, size_t displ, T* dstPtr, IntCount count) {
  auto srcLambda = [=](int i) -> T* { return basePtr + (size_t)i * displ; };
  ncclLsaReduceSum<T, Coop, decltype(srcLambda), IntCount, UNROLL>(coop, srcLambda, nSrc, dstPtr, count);
}

/* ---- series 4: one local source -> N destinations ---- */
template <typename T, typename Coop, typename DstLambda, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T),
          NCCL_RC_INTEGRAL(IntCount)>
NCCL_DEVICE_INLINE void ncclLsaCopy(Coop coop, T* srcPtr, DstLambda dstLambda, int nDst, IntCount count) {
  auto srcLambda = [=](int) -> T* { return srcPtr; };
  ncclLsaReduceSumLsaCopy<T, Coop, decltype(srcLambda), DstLambda, IntCount, UNROLL>(coop, srcLambda, 1, dstLambda,
                                                                                     nDst, count);
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaCopy(Coop coop, T* srcPtr, ncclSymPtr<T> dst, IntCount count, ncclTeam team) {
  auto dstLambda = [=](int i) -> T* { return dst.peerPtr(team, i); };
  ncclLsaCopy<T, Coop, decltype(dstLambda), IntCount, UNROLL>(coop, srcPtr, dstLambda, team.nRanks, count);
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaCopy(Coop coop, T* srcPtr, ncclSymPtr<T> dst, IntCount count,
                                    ncclDevComm const& devComm) {
  ncclLsaCopy<T, Coop, IntCount, UNROLL>(coop, srcPtr, dst, count, ncclTeamLsa(devComm));
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaCopy(Coop coop, T* srcPtr, ncclWindow_t window, size_t offset, IntCount count,
                                    ncclTeam team) {
  ncclLsaCopy<T, Coop, IntCount, UNROLL>(coop, srcPtr, ncclSymPtr<T>(window, offset), count, team);
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaCopy(Coop coop, T* srcPtr, ncclWindow_t window, size_t offset, IntCount count,
                                    ncclDevComm const& devComm) {
  ncclLsaCopy<T, Coop, IntCount, UNROLL>(coop, srcPtr, ncclSymPtr<T>(window, offset), count, ncclTeamLsa(devComm));
}
template <typename T, typename Coop, typename DstLambda, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T),
          NCCL_RC_INTEGRAL(IntCount)>
NCCL_DEVICE_INLINE void ncclLocalCopy(Coop coop, T* srcPtr, DstLambda dstLambda, int nDst, IntCount count) {
  ncclLsaCopy<T, Coop, DstLambda, IntCount, UNROLL>(coop, srcPtr, dstLambda, nDst, count);
}
/* destination i is basePtr + i·displ (displ in elements) */
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLocalCopy(Coop coop, T* srcPtr, int nDst, T* basePtr, size_t displ, IntCount count) {
  auto dstLambda = [=](int i) -> T* { return basePtr + (size_t)i * displ; };
  ncclLsaCopy<T, Coop, decltype(dstLambda), IntCount, UNROLL>(coop, srcPtr, dstLambda, nDst, count);
}

/* ---- series 5: N sources -> M destinations ---- */
/* every member of srcTeam's window at src -> every member of dstTeam's window at dst */
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSumCopy(Coop coop, ncclSymPtr<T> src, ncclTeam srcTeam, ncclSymPtr<T> dst,
                                             ncclTeam dstTeam, IntCount count) {
  auto srcLambda = [=](int i) -> T* { return src.peerPtr(srcTeam, i); };
  auto dstLambda = [=](int i) -> T* { return dst.peerPtr(dstTeam, i); };
  ncclLsaReduceSumLsaCopy<T, Coop, decltype(srcLambda), decltype(dstLambda), IntCount, UNROLL>(
      coop, srcLambda, srcTeam.nRanks, dstLambda, dstTeam.nRanks, count);
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSumCopy(Coop coop, ncclSymPtr<T> src, ncclSymPtr<T> dst, IntCount count,
                                             ncclTeam team) {
  ncclLsaReduceSumCopy<T, Coop, IntCount, UNROLL>(coop, src, team, dst, team, count);
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSumCopy(Coop coop, ncclSymPtr<T> src, ncclSymPtr<T> dst, IntCount count,
                                             ncclDevComm const& devComm) {
  ncclLsaReduceSumCopy<T, Coop, IntCount, UNROLL>(coop, src, dst, count, ncclTeamLsa(devComm));
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSumCopy(Coop coop, ncclWindow_t srcWindow, size_t srcOffset,
                                             ncclWindow_t dstWindow, size_t dstOffset, IntCount count, ncclTeam team) {
  ncclLsaReduceSumCopy<T, Coop, IntCount, UNROLL>(coop, ncclSymPtr<T>(srcWindow, srcOffset),
                                                  ncclSymPtr<T>(dstWindow, dstOffset), count, team);
}
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLsaReduceSumCopy(Coop coop, ncclWindow_t srcWindow, size_t srcOffset,
                                             ncclWindow_t dstWindow, size_t dstOffset, IntCount count,
                                             ncclDevComm const& devComm) {
  ncclLsaReduceSumCopy<T, Coop, IntCount, UNROLL>(coop, ncclSymPtr<T>(srcWindow, srcOffset),
                                                  ncclSymPtr<T>(dstWindow, dstOffset), count, ncclTeamLsa(devComm));
}
/* source i is srcBasePtr + i·srcDispl, destination i is dstBasePtr + i·dstDispl (displacements in elements) */
template <typename T, typename Coop, typename IntCount, int UNROLL = NCCL_RC_UNROLL(T)>
NCCL_DEVICE_INLINE void ncclLocalReduceSumCopy(Coop coop, int nSrc, T* srcBasePtr, size_t srcDispl, int nDst,
                                               T* dstBasePtr, size_t dstDispl, IntCount count) {
  auto srcLambda = [=](int i) -> T* { return srcBasePtr + (size_t)i * srcDispl; };
  auto dstLambda = [=](int i) -> T* { return dstBasePtr + (size_t)i * dstDispl; };
  ncclLsaReduceSumLsaCopy<T, Coop, decltype(srcLambda), decltype(dstLambda), IntCount, UNROLL>(
      coop, srcLambda, nSrc, dstLambda, nDst, count);
}

#undef NCCL_RC_UNROLL
#undef NCCL_RC_INTEGRAL

#endif /* __HIPCC__ */

#endif /* NCCL_DEVICE_REDUCE_COPY_H_ */
