/*
 * nccl_device_ll_a2a.h — ncclLLA2ASession, the low-latency all-to-all of the device API: a running kernel hands small
 * values to its peers' kernels without a barrier round and without a fence on either side. Names, members and
 * argument order are the reference's (src/include/nccl_device/ll_a2a.h), so a kernel written against it compiles
 * unchanged; the implementation is this project's own, written for gfx950 (DESIGN.md §2.7 "LLA2A"). Included by
 * nccl_device.h.
 *
 * Mechanism. Every 8 bytes of a value travel as a 16-byte line {data32, flag32, data32, flag32} whose flag is the
 * session's epoch. A send is ONE system-scope write-through 16-byte store into the peer's line; a receive polls the
 * line with 16-byte system-scope loads until both flags show the epoch. The lines live in a resource buffer of the
 * DevComm: uncached, zero-filled, symmetric. Each aligned 8-byte half {data32, flag32} is single-copy atomic, so a
 * half whose flag matches carries its data whatever the other half shows; 16-byte atomicity is not assumed. The
 * payload is in the line, so nothing else has to become visible: no release fence, no acquire fence. The session
 * publishes nothing but the values it carries — ordering data in user windows still takes the LSA barrier.
 *
 * Memory. Per block (a session's private set of lines, e.g. one per CTA), in 16-byte lines of the resource buffer:
 *     line 0               the block's stored epoch in .x (read and written by the owner only)
 *     lines 1 .. nSlots    the slots of even epochs
 *     then nSlots lines    the slots of odd epochs
 * A value of sizeof(T) bytes takes divUp(sizeof(T), 8) lines: piece u of slot s lies at line s + u * maxElts, so
 * nSlots = ncclLLA2ACalcSlots(maxElts, maxEltSize) lines hold maxElts values of up to maxEltSize bytes.
 *
 * Host side. ncclLLA2ACreateRequirement fills a ncclDevResourceRequirements for the caller to chain into
 * ncclDevCommRequirements::resourceRequirementsList; ncclDevCommCreate places the buffer and fills the handle. The
 * lsaLLA2ABlockCount / lsaLLA2ASlotCount fields of ncclDevCommRequirements stay refused: the requirement list is the
 * supported route. Both host functions are inline here and not exported from libnccl.so: the library exports exactly
 * the ncclResult_t / const char* functions include/nccl.h declares, and ncclLLA2ACalcSlots returns an int. What is kept
 * is source compatibility with a caller written against the reference.
 *
 * Epochs. The constructor loads the block's stored epoch and starts at stored + 2; the destructor stores epoch - 2, so
 * consecutive kernels and replays of a captured graph continue the sequence. Zero-filled memory must never look
 * flagged: the epochs 0 and 1 occur only before the first wrap (a fresh buffer starts at 2), and the wrap steps from
 * 0xFFFFFFFF to 2. Epoch e uses the slots of parity e & 1.
 *
 * The caller's contract, in the reference's words: before endEpoch, for every peer in the team, this coop must have
 * done both of the following, each of which can be accomplished using any thread of the coop:
 *   1. targeted that peer with at least one send();
 *   2. received from a slot targeted by that peer.
 * That is what makes two parities enough: a peer stores lines of epoch e + 2 only after it has received this rank's
 * line of epoch e + 1, which this rank sends only after it has read every line of epoch e it wanted.
 *
 * Every thread of the coop constructs, ends epochs and destroys together, converged. Every thread loads the stored
 * epoch in the constructor without a sync of its own and thread 0 alone stores it in the destructor: the sync that
 * closes every endEpoch and the one that closes the destructor keep a later session on the same block (in this kernel
 * or the next) from loading the word before it is stored. send / bcast / recv* may be called
 * by any thread of the coop on its own. Every spin is bounded as the LSA barrier's untimed wait is (ncclDevSpinGiveUp):
 * a receive that gives up returns unspecified values and ncclCommGetAsyncError reports why; tear the DevComm down.
 *
 * Not here: the reference's trailing `bool multimem, ncclMultimemHandle` constructor parameters (no multimem on this
 * hardware; passing them fails at compile time).
 */
#ifndef NCCL_DEVICE_LL_A2A_H_
#define NCCL_DEVICE_LL_A2A_H_

#ifndef NCCL_DEVICE_H_
#error "include nccl_device.h, not this header"
#endif

#include <stdint.h>
#include <string.h>

/* The lines one poll round of recvUnrolled may load: MaxEltCount * divUp(sizeof(T), 8) (4 VGPRs each). */
#define NCCL_LLA2A_MAX_LINES_PER_ROUND 32

struct ncclLLA2AHandle {
  ncclDevResourceHandle_t bufHandle; /* the line area in the resource window */
  uint32_t nSlots;                   /* lines per parity and block */
};
typedef struct ncclLLA2AHandle ncclLLA2AHandle_t;

/* Lines (slots) that maxElts values of up to maxEltSize bytes take: one per 8 bytes of a value. */
NCCL_HOST_DEVICE_INLINE int ncclLLA2ACalcSlots(int maxElts, int maxEltSize) { return maxElts * ((maxEltSize + 7) / 8); }

/* The first slot line of `block` for `epoch`, in lines from the buffer's start. Pure. */
NCCL_HOST_DEVICE_INLINE uint32_t ncclLLA2ASlotOffset(uint32_t block, uint32_t nSlots, uint32_t epoch) {
  return block * (1 + 2 * nSlots) + 1 + (epoch & 1) * nSlots;
}

/* The epoch after `epoch`: +1, and from 0xFFFFFFFF to 2, so that the parity alternates across the wrap and the epochs
 * 0 and 1 — what zero-filled lines would match, and the parity they would break — never follow. Pure. */
NCCL_HOST_DEVICE_INLINE uint32_t ncclLLA2ANextEpoch(uint32_t epoch) { return epoch + (epoch == 0xFFFFFFFFu ? 3u : 1u); }

/* The resource buffer of nBlocks blocks of nSlots slots: chain *outReq into resourceRequirementsList before
 * ncclDevCommCreate, which fills outHandle->bufHandle. *outHandle must live until then. */
inline ncclResult_t ncclLLA2ACreateRequirement(int nBlocks, int nSlots, ncclLLA2AHandle_t* outHandle,
                                               ncclDevResourceRequirements_t* outReq) {
  memset(outReq, 0, sizeof(*outReq));
  outReq->bufferSize = (size_t)nBlocks * (1 + 2 * (size_t)nSlots) * 16;
  outReq->bufferAlign = 16;
  outReq->outBufferHandle = &outHandle->bufHandle;
  outHandle->nSlots = (uint32_t)nSlots;
  return ncclSuccess;
}

/* ------------------------------------------------------------------------------------- device functions */
#if defined(__HIPCC__)

namespace nccl {
namespace lla2a {

typedef unsigned int Line __attribute__((ext_vector_type(4))); /* {data32, flag32, data32, flag32} */

template <typename T>
struct Pieces {
  static_assert(std::is_trivially_copyable<T>::value, "ncclLLA2ASession moves trivially copyable values");
  static constexpr int value = (int)((sizeof(T) + 7) / 8);
};

/* One line, one store: system-scope write-through. The compiler has no builtin for it and cannot see the store, so it
 * carries its own wait states against a write to its data registers right behind it (as kernels.h's LL stores do). */
NCCL_DEVICE_INLINE void storeLine(Line* p, Line v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

/* The polling load, issued and NOT waited for: the caller issues all loads of a round back to back and then calls
 * landed() on every destination, so a round costs one memory latency, not one per line. (A volatile C++ load gets
 * the same cache policy but a wait of its own behind every load.) */
NCCL_DEVICE_INLINE void issueLoad(Line& v, const Line* p) {
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=&v"(v) : "v"(p) : "memory");
}
/* Waits for every load in flight. The lines pass through the statement as read-write operands: whatever reads them
 * is ordered behind the wait. Between issueLoad and this statement the compiler believes the registers already hold
 * the lines; that it neither copies nor spills them there is a property of its register allocation, not of the
 * language. It holds where it was looked at in the gfx950 assembly (hipcc of ROCm 7.2, -O3): 1 to 12 lines in one round
 * (recv of 4- to 24-byte values, recvReduce<4> of float and double), no copy between the loads and the wait and no
 * scratch; recvUnrolled bounds a round at NCCL_LLA2A_MAX_LINES_PER_ROUND lines, far below the register file, so that
 * nothing has to spill. A kernel built at -O0, or one that already spills, is outside what was checked. */
template <int N>
NCCL_DEVICE_INLINE void landed(Line* v) {
  if constexpr (N == 1) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0])::"memory");
  } else if constexpr (N == 2) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1])::"memory");
  } else if constexpr (N == 3) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2])::"memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])::"memory");
    /* more lines than one statement takes: the first statement waited, the others pass their lines through */
    if constexpr (N > 4) landed<N - 4>(v + 4);
  }
}

/* std::declval for a device function's return type */
template <typename T>
__host__ __device__ T&& declval() noexcept;

NCCL_DEVICE_INLINE void drainStores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

/* The 8-byte pieces of a value as lines of `epoch`; a tail shorter than 8 bytes is zero-padded. */
template <typename T>
NCCL_DEVICE_INLINE void pack(T const& data, uint32_t epoch, Line (&lines)[Pieces<T>::value]) {
  uint32_t w[2 * Pieces<T>::value] = {};
  __builtin_memcpy(w, &data, sizeof(T));
#pragma unroll
  for (int u = 0; u < Pieces<T>::value; u++) lines[u] = Line{w[2 * u], epoch, w[2 * u + 1], epoch};
}

}  // namespace lla2a
}  // namespace nccl

template <typename Coop>
struct ncclLLA2ASession {
  NCCL_DEVICE_INLINE ncclLLA2ASession(Coop coop, ncclDevComm const& comm, ncclTeam team, ncclLLA2AHandle handle,
                                      uint32_t block, int maxElts)
      : coop_(coop), comm_(comm), team_(team), handle_(handle), block_(block), pitch_(maxElts) {
    mine_ = (nccl::lla2a::Line*)ncclGetResourceBufferLocalPointer(comm, handle.bufHandle);
    epoch_ = __hip_atomic_load(epochWord(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 2;
    slotsOffset_ = ncclLLA2ASlotOffset(block_, handle_.nSlots, epoch_);
  }

  NCCL_DEVICE_INLINE ~ncclLLA2ASession() {
    if (coop_.thread_rank() == 0) __hip_atomic_store(epochWord(), epoch_ - 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    coop_.sync();
  }

  ncclLLA2ASession(ncclLLA2ASession const&) = delete;
  ncclLLA2ASession& operator=(ncclLLA2ASession const&) = delete;

  /* `data` into slot `slot` of team member `peer` (this rank included: the same path). */
  template <typename T>
  NCCL_DEVICE_INLINE void send(int peer, int slot, T data) {
    constexpr int P = nccl::lla2a::Pieces<T>::value;
    nccl::lla2a::Line lines[P];
    nccl::lla2a::pack(data, epoch_, lines);
    nccl::lla2a::Line* to = peerSlot(peer, slot);
#pragma unroll
    for (int u = 0; u < P; u++) nccl::lla2a::storeLine(to + u * pitch_, lines[u]);
  }

  /* `data` into slot `slot` of every team member, this rank first and on round the team, so that the ranks' first
   * stores go to different targets. Each member's line area is looked up once, outside the loop over the pieces. */
  template <typename T>
  NCCL_DEVICE_INLINE void bcast(int slot, T data) {
    constexpr int P = nccl::lla2a::Pieces<T>::value;
    nccl::lla2a::Line lines[P];
    nccl::lla2a::pack(data, epoch_, lines);
    int peer = team_.rank;
    for (int k = 0; k < team_.nRanks; k++) {
      nccl::lla2a::Line* to = peerSlot(peer, slot);
#pragma unroll
      for (int u = 0; u < P; u++) nccl::lla2a::storeLine(to + u * pitch_, lines[u]);
      if (++peer == team_.nRanks) peer = 0;
    }
  }

  template <typename T>
  NCCL_DEVICE_INLINE T recv(int slot) {
    T got[1];
    recvUnrolled<1, 1>(slot, 1, 0, got);
    return got[0];
  }

  /* vals[u] = the value in slot eltStart + u * eltStride, for u < max(MinEltCount, eltCount) (<= MaxEltCount). A poll
   * round issues the loads of all wanted lines back to back, waits once and tests every line; it repeats until all
   * carry this epoch. An element past eltCount polls element 0's lines again, so a round has no branch. */
  template <int MinEltCount, int MaxEltCount, typename T>
  NCCL_DEVICE_INLINE void recvUnrolled(int eltStart, int eltCount, int eltStride, T (&vals)[MaxEltCount]) {
    static_assert(1 <= MinEltCount && MinEltCount <= MaxEltCount, "1 <= MinEltCount <= MaxEltCount");
    constexpr int P = nccl::lla2a::Pieces<T>::value;
    static_assert(MaxEltCount * P <= NCCL_LLA2A_MAX_LINES_PER_ROUND, "too many lines in one poll round: lower Unroll");
    const nccl::lla2a::Line* from = mine_ + slotsOffset_ + eltStart;
    int step[MaxEltCount]; /* the element's distance from eltStart in lines */
#pragma unroll
    for (int u = 0; u < MaxEltCount; u++) step[u] = (u < MinEltCount || u < eltCount) ? u * eltStride : 0;
    nccl::lla2a::Line got[MaxEltCount * P];
    uint64_t t0 = 0;
    uint32_t polls = 0;
    for (;;) {
#pragma unroll
      for (int u = 0; u < MaxEltCount; u++) {
#pragma unroll
        for (int v = 0; v < P; v++) nccl::lla2a::issueLoad(got[u * P + v], from + step[u] + v * pitch_);
      }
      nccl::lla2a::landed<MaxEltCount * P>(got);
      bool all = true;
#pragma unroll
      for (int i = 0; i < MaxEltCount * P; i++) all &= got[i].y == epoch_ && got[i].w == epoch_;
      if (__builtin_expect(all, 1)) break;
      if (polls == 0) t0 = __builtin_amdgcn_s_memrealtime();
      __builtin_amdgcn_s_sleep(1);
      if ((++polls & 255) == 0 && ncclDevSpinGiveUp(comm_, t0, false, 0)) break; /* vals are unspecified then */
    }
#pragma unroll
    for (int u = 0; u < MaxEltCount; u++) {
      if (u >= MinEltCount && u >= eltCount) break;
      uint32_t w[2 * P];
#pragma unroll
      for (int v = 0; v < P; v++) {
        w[2 * v] = got[u * P + v].x;
        w[2 * v + 1] = got[u * P + v].z;
      }
      __builtin_memcpy(&vals[u], w, sizeof(T));
    }
  }

  /* reduce(... reduce(eltToAcc(e_0), eltToAcc(e_1)) ..., eltToAcc(e_{eltCount-1})) over the values e_i in slots
   * eltStart + i * eltStride: folded in that order, seeded from the first, received Unroll at a time. */
  template <int Unroll, typename Elt, typename EltToAcc, typename Reduce>
  NCCL_DEVICE_INLINE auto recvReduce(int eltStart, int eltCount, int eltStride, EltToAcc eltToAcc, Reduce reduce)
      -> decltype(eltToAcc(nccl::lla2a::declval<Elt>())) {
    using Acc = decltype(eltToAcc(nccl::lla2a::declval<Elt>()));
    static_assert(Unroll >= 1, "Unroll >= 1");
    Acc acc{};
    int i = 0;
#pragma unroll 1
    for (; i + Unroll <= eltCount; i += Unroll) {
      Elt got[Unroll];
      recvUnrolled<Unroll, Unroll>(eltStart + i * eltStride, Unroll, eltStride, got);
      const Acc first = eltToAcc(got[0]);
      acc = i == 0 ? first : reduce(acc, first);
#pragma unroll
      for (int j = 1; j < Unroll; j++) acc = reduce(acc, eltToAcc(got[j]));
    }
    if (i < eltCount) { /* 1 .. Unroll-1 elements are left */
      const int left = eltCount - i;
      Elt got[Unroll];
      recvUnrolled<1, Unroll>(eltStart + i * eltStride, left, eltStride, got);
      const Acc first = eltToAcc(got[0]);
      acc = i == 0 ? first : reduce(acc, first);
#pragma unroll
      for (int j = 1; j < Unroll; j++)
        if (j < left) acc = reduce(acc, eltToAcc(got[j]));
    }
    return acc;
  }

  /* Ends the all-to-all region (see the contract above) and moves to the next epoch and the other parity. Leaving
   * one of the last two epochs before the wrap also zeroes the lines just used: two epochs on, their parity is used by
   * epoch 2 or 3, whose flags lines from 2^32 epochs ago may still carry. The first sync says every thread has read
   * what it wanted; every wave waits for its clearing stores before the closing sync, because a store to this rank's
   * memory and a later store to a peer's are not otherwise ordered — the peer's answer to that later store, a line of
   * the epoch two ahead in the same slot, must not be overtaken by the clearing. */
  NCCL_DEVICE_INLINE void endEpoch(Coop) {
    if (__builtin_expect(epoch_ >= 0xFFFFFFFEu, 0)) {
      coop_.sync();
      nccl::lla2a::Line* used = mine_ + slotsOffset_;
      for (uint32_t i = (uint32_t)coop_.thread_rank(); i < handle_.nSlots; i += (uint32_t)coop_.size())
        nccl::lla2a::storeLine(used + i, nccl::lla2a::Line{0u, 0u, 0u, 0u});
      nccl::lla2a::drainStores();
    }
    coop_.sync();
    epoch_ = ncclLLA2ANextEpoch(epoch_);
    slotsOffset_ = ncclLLA2ASlotOffset(block_, handle_.nSlots, epoch_);
  }

 private:
  Coop coop_;
  ncclDevComm const& comm_;
  ncclTeam team_;
  ncclLLA2AHandle handle_;
  uint32_t block_;
  int pitch_; /* lines between two pieces of one value: maxElts */
  uint32_t epoch_;
  uint32_t slotsOffset_;     /* this epoch's first slot line of this block, in lines */
  nccl::lla2a::Line* mine_;  /* this rank's line area */

  NCCL_DEVICE_INLINE uint32_t* epochWord() const {
    return (uint32_t*)(mine_ + (size_t)block_ * (1 + 2 * (size_t)handle_.nSlots));
  }
  NCCL_DEVICE_INLINE nccl::lla2a::Line* peerSlot(int peer, int slot) const {
    return (nccl::lla2a::Line*)ncclGetResourceBufferPeerPointer(comm_, handle_.bufHandle, team_, peer) + slotsOffset_ +
           slot;
  }
};

#endif /* __HIPCC__ */

#endif /* NCCL_DEVICE_LL_A2A_H_ */
