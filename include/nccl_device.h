/*
 * nccl_device.h — the device API of libnccl.so (nccl_amd) in its LSA ("load/store accessible") form.
 *
 * A kernel of the caller's own reads and writes its peers' memory through registered windows and synchronises with
 * the other ranks from inside the kernel. This header restates the public names, struct roles and signatures of the
 * reference's device API (src/include/nccl_device/core.h, coop.h, ptr.h, lsa_barrier.h, reduce_copy.h) for the subset that has a
 * hardware counterpart on a full-mesh xGMI node: every rank is load/store accessible from every other, so the world
 * team and the LSA team are the same team and the LSA subset is the whole intra-node device API. The implementation
 * is this project's own.
 *
 * Porting a kernel written against the reference:
 *   - memory orders are std::memory_order from <atomic> (HIP has no cuda::memory_order);
 *   - ncclCoopWarp is one 64-lane wavefront on gfx950, not 32 threads;
 *   - kernels are launched with hipLaunchKernelGGL / <<<>>> on a hipStream_t.
 * Nothing else changes: ncclDevComm is passed to kernels by value, ncclWindow_t by value.
 *
 * ncclSymPtr<T> (ptr.h) is here; the reduce-copy family (reduce_copy.h: ncclLsaReduceSum, ncclLsaCopy,
 * ncclLsaReduceSumCopy, their lambda and ncclLocal* forms) is in nccl_device_reduce_copy.h, which this header includes
 * for hipcc.
 *
 * Not provided (no counterpart here): GIN, multimem (ncclSymPtr has no multimemPtr / lsaMultimemPtr member and the
 * ncclMultimem* / *MultimemCopy functions are not declared, so their use fails at compile time), ncclLLA2A, the hybrid
 * ncclBarrierSession, rail teams, fp8 reduce-copy.
 *
 * Time: every bounded wait counts ticks of __builtin_amdgcn_s_memrealtime(), a constant 100 MHz clock
 * (1 tick = 10 ns; 20 ms = 2,000,000 ticks). `timeoutCycles` arguments are in these ticks.
 *
 * Host-only translation units (plain C++17) may include this header: they see the types, ncclSymPtr's fields and
 * arithmetic, the team functions and the layout function; the device functions need hipcc.
 */
#ifndef NCCL_DEVICE_H_
#define NCCL_DEVICE_H_

#include "nccl.h"

#ifndef __cplusplus
#error "nccl_device.h is a C++ header (include/nccl.h is the C header)"
#endif

#include <atomic>
#include <cstddef>
#include <type_traits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NCCL_DEVICE_INLINE __device__ __forceinline__
#endif
#define NCCL_HOST_DEVICE_INLINE __host__ __device__ inline

/* Ranks of one communicator (nccl_amd/csrc/device_abi.h NCCL_AMD_MAX_RANKS). */
#define NCCL_DEVICE_MAX_RANKS 16
/* The cap on ncclDevCommRequirements::lsaBarrierCount (ncclInvalidArgument above it). */
#define NCCL_DEVICE_MAX_LSA_BARRIERS 4096
/* Resource buffers are placed at multiples of this many bytes; a ncclDevResourceHandle counts them. */
#define NCCL_DEVICE_RESOURCE_GRANULE 128
/* The largest ncclDevResourceRequirements::bufferAlign (a power of two; the allocation's own alignment). */
#define NCCL_DEVICE_MAX_BUFFER_ALIGN 4096

/* ---------------------------------------------------------------------------------------------- types */

struct ncclTeam {
  int nRanks, rank, stride;
};
typedef struct ncclTeam ncclTeam_t;

struct ncclTeamTagWorld {};
struct ncclTeamTagLsa {};

typedef uint32_t ncclDevResourceHandle;
typedef ncclDevResourceHandle ncclDevResourceHandle_t;
typedef uint32_t ncclGinSignal_t;
typedef uint32_t ncclGinCounter_t;
struct ncclTeamRequirements;
typedef struct ncclTeamRequirements ncclTeamRequirements_t;
struct ncclDevResourceRequirements;
typedef struct ncclDevResourceRequirements ncclDevResourceRequirements_t;

typedef enum {
  NCCL_GIN_CONNECTION_NONE,
  NCCL_GIN_CONNECTION_FULL,
  NCCL_GIN_CONNECTION_RAIL,
} ncclGinConnectionType_t;

typedef enum {
  NCCL_GIN_TYPE_NONE = 0,
  NCCL_GIN_TYPE_PROXY = 2,
  NCCL_GIN_TYPE_GDAKI = 3,
  NCCL_GIN_TYPE_GPI = 4,
} ncclGinType_t;

/* One resource buffer asked of ncclDevCommCreate (a list through `next`): bufferSize bytes at a multiple of
 * bufferAlign in every rank's resource window; *outBufferHandle names it afterwards. The gin counts must be 0. */
struct ncclDevResourceRequirements {
  ncclDevResourceRequirements_t* next;
  size_t bufferSize, bufferAlign;
  ncclDevResourceHandle_t* outBufferHandle;
  int ginSignalCount;
  int ginCounterCount;
  ncclGinSignal_t* outGinSignalStart;
  ncclGinCounter_t* outGinCounterStart;
};

/* Same field order and types as the reference's, so a caller's initialised struct is read correctly. Honoured:
 * resourceRequirementsList, lsaBarrierCount. Refused with ncclInvalidUsage when set: teamRequirementsList,
 * lsaMultimem, barrierCount, railGinBarrierCount, lsaLLA2ABlockCount / lsaLLA2ASlotCount, ginForceEnable,
 * ginSignalCount, ginCounterCount, a ginConnectionType other than NONE, worldGinBarrierCount. The remaining gin
 * fields are hints without a meaning here and are ignored. */
struct ncclDevCommRequirements {
  size_t size;
  unsigned int magic;
  unsigned int version;

  ncclDevResourceRequirements_t* resourceRequirementsList;
  ncclTeamRequirements_t* teamRequirementsList;

  bool lsaMultimem;

  int barrierCount;
  int lsaBarrierCount;
  int railGinBarrierCount;

  int lsaLLA2ABlockCount, lsaLLA2ASlotCount;

  bool ginForceEnable;

  int ginContextCount;
  int ginSignalCount;
  int ginCounterCount;
  ncclGinConnectionType_t ginConnectionType;
  bool ginExclusiveContexts;
  int ginQueueDepth;
  int ginTrafficClass;

  int worldGinBarrierCount;

  bool ginStrongSignalsRequired;
  bool ginVaSignalsRequired;
};

#define NCCL_DEV_COMM_REQUIREMENTS_INITIALIZER                                                                     \
  {                                                                                                                \
    sizeof(ncclDevCommRequirements_t), NCCL_API_MAGIC, NCCL_VERSION_CODE, NULL, NULL, false, 0, 0, 0, 0, 0, false, \
        4, 0, 0, NCCL_GIN_CONNECTION_NONE, false, 0, NCCL_CONFIG_UNDEF_INT, 0, true, true                          \
  }

struct ncclCommProperties {
  size_t size;
  unsigned int magic;
  unsigned int version;

  int rank;
  int nRanks;
  int cudaDev; /* the HIP device */
  int nvmlDev; /* -1: no such index here */
  bool deviceApiSupport;
  bool multimemSupport;
  ncclGinType_t ginType;
  int nLsaTeams;
  bool hostRmaSupport;
  ncclGinType_t railedGinType;
};

#define NCCL_COMM_PROPERTIES_INITIALIZER \
  { sizeof(ncclCommProperties_t), NCCL_API_MAGIC, NCCL_VERSION_CODE }

struct ncclLsaBarrierHandle {
  ncclDevResourceHandle_t bufHandle; /* the barrier region in the resource window */
  int nBarriers;
};
typedef struct ncclLsaBarrierHandle ncclLsaBarrierHandle_t;

/* A registered window as the device reads it. The object lives in pinned, mapped, portable host memory, so a kernel
 * dereferences the very ncclWindow_t the host holds. The table is immutable after registration. The device reads the
 * fields above the line only. */
struct ncclWindow_vidmem {
  char* peerPtr[NCCL_DEVICE_MAX_RANKS];   /* every rank's window base as mapped in this process */
  size_t peerSize[NCCL_DEVICE_MAX_RANKS]; /* the bytes each rank registered (equal when symmetric) */
  int nRanks;
  int rank;
  /* ---- host side ---- */
  struct ncclComm* comm;
  void* userPtr;
  size_t size;
  int flags;
  uint64_t peerBase[NCCL_DEVICE_MAX_RANKS]; /* allocation bases of IPC-mapped peers (0: direct pointer) */
};
typedef struct ncclWindow_vidmem ncclWindow_vidmem_t;

/* The resource window's table, copied into ncclDevComm so that barriers and resource buffers never go through the
 * pinned-host indirection. */
typedef struct ncclResourceWindow_vidmem {
  char* peerPtr[NCCL_DEVICE_MAX_RANKS];
} ncclResourceWindow_vidmem_t;

/* Passed to kernels by value. Read-only for its users. */
struct ncclDevComm {
  unsigned int magic;
  unsigned int version;

  int rank, nRanks;
  int lsaRank, lsaSize; /* == rank, nRanks: one node, full mesh */

  ncclWindow_t resourceWindow;
  ncclResourceWindow_vidmem_t resourceWindow_inlined;

  ncclLsaBarrierHandle_t lsaBarrier; /* the lsaBarrierCount barriers of ncclDevCommCreate */

  uint32_t* abortFlag;   /* the communicator's abort word (pinned host memory; nonzero = abort) */
  uint32_t* errorWord;   /* its device error word: the first error a kernel recorded (ncclCommGetAsyncError) */
  uint64_t timeoutTicks; /* its spin timeout (NCCL_AMD_SPIN_TIMEOUT_MS) in 100 MHz ticks */

  void* hostState; /* ncclDevCommDestroy's key; never read on the device */
};

/* What an untimed wait records in ncclDevComm::errorWord when it gives up (device_abi.h DevError). */
#define NCCL_DEVICE_ERR_TIMEOUT 1u
#define NCCL_DEVICE_ERR_ABORT 2u

/* --------------------------------------------------------------------------------------- resource layout */

/* One rank's resource allocation of a DevComm (uncached device memory, zero-filled, the same layout on every rank):
 *
 *   [0, ...)            uint32 epoch[lsaBarrierCount]          this rank's epoch of barrier b (local use only)
 *   [inboxOffset, ...)  uint32 inbox[lsaBarrierCount][nRanks]  inbox[b][from]: the epoch rank `from` has arrived at
 *   buffer k            at offsets[k], a multiple of max(aligns[k], NCCL_DEVICE_RESOURCE_GRANULE)
 *
 * Every region starts at a multiple of NCCL_DEVICE_RESOURCE_GRANULE; totalBytes is a multiple of 4096. aligns[k]
 * must be a power of two (0 counts as 1). Pure: called by ncclDevCommCreate, by the barrier and by CPU tests. */
struct ncclDevResourceLayout {
  size_t epochOffset;
  size_t inboxOffset;
  size_t buffersOffset; /* where the first buffer may start */
  size_t totalBytes;
};

NCCL_HOST_DEVICE_INLINE size_t ncclDevAlignUp(size_t x, size_t a) { return (x + a - 1) / a * a; }

NCCL_HOST_DEVICE_INLINE size_t ncclLsaBarrierInboxOffset(int nBarriers) {
  return ncclDevAlignUp((size_t)nBarriers * sizeof(uint32_t), NCCL_DEVICE_RESOURCE_GRANULE);
}

NCCL_HOST_DEVICE_INLINE ncclDevResourceLayout ncclDevCommResourceLayout(int nRanks, int lsaBarrierCount, int nBuffers,
                                                                        const size_t* sizes, const size_t* aligns,
                                                                        size_t* offsets) {
  ncclDevResourceLayout l;
  l.epochOffset = 0;
  l.inboxOffset = ncclLsaBarrierInboxOffset(lsaBarrierCount);
  l.buffersOffset = l.inboxOffset + ncclDevAlignUp((size_t)lsaBarrierCount * (size_t)nRanks * sizeof(uint32_t),
                                                   NCCL_DEVICE_RESOURCE_GRANULE);
  size_t at = l.buffersOffset;
  for (int k = 0; k < nBuffers; k++) {
    size_t a = aligns[k] > NCCL_DEVICE_RESOURCE_GRANULE ? aligns[k] : NCCL_DEVICE_RESOURCE_GRANULE;
    at = ncclDevAlignUp(at, a);
    offsets[k] = at;
    at += sizes[k];
  }
  l.totalBytes = ncclDevAlignUp(at > 0 ? at : 1, 4096);
  return l;
}

NCCL_HOST_DEVICE_INLINE size_t ncclGetResourceBufferOffset(ncclDevResourceHandle_t h) {
  return (size_t)h * NCCL_DEVICE_RESOURCE_GRANULE;
}

/* Barrier epochs are uint32 and wrap: "has `seen` reached `want`?" holds while the two are less than 2^31 apart,
 * and a peer is never more than one epoch ahead of or behind this rank. */
NCCL_HOST_DEVICE_INLINE bool ncclLsaEpochReached(uint32_t seen, uint32_t want) { return (int32_t)(seen - want) >= 0; }

/* ------------------------------------------------------------------------------------------------ teams */

/* A team is an arithmetic progression of world ranks as seen from this rank: its member i is the world rank
 * myWorldRank + (i - team.rank) * team.stride, for 0 <= i < team.nRanks. */
NCCL_HOST_DEVICE_INLINE ncclTeam ncclTeamWorld(ncclDevComm const& comm) {
  ncclTeam t;
  t.nRanks = comm.nRanks;
  t.rank = comm.rank;
  t.stride = 1;
  return t;
}

NCCL_HOST_DEVICE_INLINE ncclTeam ncclTeamLsa(ncclDevComm const& comm) {
  ncclTeam t;
  t.nRanks = comm.lsaSize;
  t.rank = comm.lsaRank;
  t.stride = 1;
  return t;
}

NCCL_HOST_DEVICE_INLINE int ncclTeamRankToWorld(ncclDevComm const& comm, ncclTeam team, int rank) {
  return comm.rank + (rank - team.rank) * team.stride;
}

NCCL_HOST_DEVICE_INLINE int ncclTeamRankToLsa(ncclDevComm const& comm, ncclTeam team, int rank) {
  return comm.lsaRank + (rank - team.rank) * team.stride;
}

/* Is member bRank of team b a member of team a? (Both teams are this rank's.) */
NCCL_HOST_DEVICE_INLINE bool ncclTeamRankIsMember(ncclTeam_t a, ncclTeam_t b, int bRank) {
  const int delta = (bRank - b.rank) * b.stride; /* world distance from this rank */
  if (delta % a.stride != 0) return false;
  const int aRank = a.rank + delta / a.stride;
  return aRank >= 0 && aRank < a.nRanks;
}

/* Member bRank of team b as a rank of team a (it must be a member of a). */
NCCL_HOST_DEVICE_INLINE int ncclTeamRankToTeam(ncclTeam_t a, ncclTeam_t b, int bRank) {
  return a.rank + (bRank - b.rank) * b.stride / a.stride;
}

/* parent = outer x inner: the inner factor is this rank's run of innerSize consecutive parent ranks, the outer
 * factor the parent ranks at this rank's position of every run. innerSize divides parent.nRanks. */
NCCL_HOST_DEVICE_INLINE ncclTeam_t ncclTeamInnerFactor(ncclTeam_t parent, int innerSize) {
  ncclTeam_t t;
  t.nRanks = innerSize;
  t.rank = parent.rank % innerSize;
  t.stride = parent.stride;
  return t;
}

NCCL_HOST_DEVICE_INLINE ncclTeam_t ncclTeamOuterFactor(ncclTeam_t parent, int innerSize) {
  ncclTeam_t t;
  t.nRanks = parent.nRanks / innerSize;
  t.rank = parent.rank / innerSize;
  t.stride = parent.stride * innerSize;
  return t;
}

/* `subset` is a subset of `parent`: the index'th member (ascending) of parent minus subset, as a parent rank,
 * for 0 <= index < parent.nRanks - subset.nRanks. */
NCCL_HOST_DEVICE_INLINE int ncclTeamRankInDifference(ncclTeam_t parent, ncclTeam_t subset, int index) {
  const int step = subset.stride / parent.stride;        /* parent ranks between two subset members */
  const int first = parent.rank - subset.rank * step;    /* the subset's member 0 as a parent rank */
  if (index < first) return index;                       /* below the subset */
  const int rest = index - first;
  const int perGap = step - 1;                           /* non-members between two neighbours of the subset */
  const int inGaps = (subset.nRanks - 1) * perGap;
  if (rest < inGaps) return first + (rest / perGap) * step + 1 + rest % perGap;
  return first + (subset.nRanks - 1) * step + 1 + (rest - inGaps); /* above the subset */
}

/* ------------------------------------------------------------------------------------------- ncclSymPtr */

/* A typed pointer into a symmetric window: the window and a byte offset, the same on every rank. Arithmetic counts
 * elements of T (negative steps included); a - b is the distance in elements; conversion to ncclSymPtr<U> keeps window
 * and byte offset. Host and device. The device members are the window getters below cast to T*. There is no
 * multimemPtr / lsaMultimemPtr: multimem has no counterpart here, and leaving them undeclared makes a use fail at
 * compile time. */
template <typename T>
struct ncclSymPtr {
  using ElementType = T;
  ncclWindow_t window;
  size_t offset;

  NCCL_HOST_DEVICE_INLINE constexpr ncclSymPtr(ncclWindow_t window = nullptr, size_t offset = 0)
      : window(window), offset(offset) {}

  template <typename U>
  NCCL_HOST_DEVICE_INLINE operator ncclSymPtr<U>() const {
    return ncclSymPtr<U>(window, offset);
  }

#define NCCL_SYMPTR_STEP(Int)                                     \
  NCCL_HOST_DEVICE_INLINE ncclSymPtr<T>& operator+=(Int d) {      \
    offset += (size_t)d * sizeof(T); /* modular: d may be < 0 */  \
    return *this;                                                 \
  }                                                               \
  NCCL_HOST_DEVICE_INLINE ncclSymPtr<T>& operator-=(Int d) {      \
    offset -= (size_t)d * sizeof(T);                              \
    return *this;                                                 \
  }
  NCCL_SYMPTR_STEP(int)
  NCCL_SYMPTR_STEP(unsigned int)
  NCCL_SYMPTR_STEP(long)
  NCCL_SYMPTR_STEP(unsigned long)
  NCCL_SYMPTR_STEP(long long)
  NCCL_SYMPTR_STEP(unsigned long long)
#undef NCCL_SYMPTR_STEP

#if defined(__HIPCC__)
  __device__ __forceinline__ T* localPtr() const;
  __device__ __forceinline__ T* lsaPtr(int peer) const;
  __device__ __forceinline__ T* peerPtr(int peer) const;
  __device__ __forceinline__ T* peerPtr(ncclTeam team, int peer) const;
#endif
};

template <typename T, typename Int, typename = std::enable_if_t<std::is_integral<Int>::value>>
NCCL_HOST_DEVICE_INLINE ncclSymPtr<T> operator+(ncclSymPtr<T> p, Int d) {
  return p += d;
}
template <typename T, typename Int, typename = std::enable_if_t<std::is_integral<Int>::value>>
NCCL_HOST_DEVICE_INLINE ncclSymPtr<T> operator-(ncclSymPtr<T> p, Int d) {
  return p -= d;
}
template <typename T>
NCCL_HOST_DEVICE_INLINE ptrdiff_t operator-(ncclSymPtr<T> a, ncclSymPtr<T> b) {
  return ((ptrdiff_t)a.offset - (ptrdiff_t)b.offset) / (ptrdiff_t)sizeof(T);
}
/* (the reference declares these two with a ncclSymPtr return type, a slip: they compare) */
template <typename T>
NCCL_HOST_DEVICE_INLINE bool operator==(ncclSymPtr<T> a, ncclSymPtr<T> b) {
  return a.window == b.window && a.offset == b.offset;
}
template <typename T>
NCCL_HOST_DEVICE_INLINE bool operator!=(ncclSymPtr<T> a, ncclSymPtr<T> b) {
  return !(a == b);
}

/* ------------------------------------------------------------------------------------- device functions */
#if defined(__HIPCC__)

/* Cooperative groups: the set of threads that calls a barrier together. Every thread of the group calls with the
 * same arguments, converged. */
struct ncclCoopThread {
  NCCL_DEVICE_INLINE int thread_rank() const { return 0; }
  NCCL_DEVICE_INLINE constexpr int size() const { return 1; }
  NCCL_DEVICE_INLINE constexpr int num_threads() const { return 1; }
  NCCL_DEVICE_INLINE void sync() {}
};

/* One wavefront: 64 lanes on gfx950 (the reference's warp has 32). All 64 lanes must be active. */
struct ncclCoopWarp {
  NCCL_DEVICE_INLINE int thread_rank() const { return (int)__lane_id(); }
  NCCL_DEVICE_INLINE constexpr int size() const { return 64; }
  NCCL_DEVICE_INLINE constexpr int num_threads() const { return 64; }
  NCCL_DEVICE_INLINE void sync() { __builtin_amdgcn_wave_barrier(); }
};

/* The whole workgroup. */
struct ncclCoopCta {
  NCCL_DEVICE_INLINE int thread_rank() const {
    return (int)(threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z));
  }
  NCCL_DEVICE_INLINE int size() const { return (int)(blockDim.x * blockDim.y * blockDim.z); }
  NCCL_DEVICE_INLINE int num_threads() const { return size(); }
  NCCL_DEVICE_INLINE void sync() { __syncthreads(); }
};

/* sync() that also tells every thread of the group whether any of them passed true */
NCCL_DEVICE_INLINE bool ncclCoopSyncAny(ncclCoopThread, bool p) { return p; }
NCCL_DEVICE_INLINE bool ncclCoopSyncAny(ncclCoopWarp, bool p) { return __any(p) != 0; }
NCCL_DEVICE_INLINE bool ncclCoopSyncAny(ncclCoopCta, bool p) { return __syncthreads_or(p) != 0; }

/* ---- window pointers ---- */
NCCL_DEVICE_INLINE void* ncclGetLsaPointer(ncclWindow_t w, size_t offset, int peer) {
  return w->peerPtr[peer] + offset;
}
NCCL_DEVICE_INLINE void* ncclGetLocalPointer(ncclWindow_t w, size_t offset) {
  return w->peerPtr[w->rank] + offset;
}
/* `peer` is a world rank; world and LSA ranks coincide */
NCCL_DEVICE_INLINE void* ncclGetPeerPointer(ncclWindow_t w, size_t offset, int peer) {
  return w->peerPtr[peer] + offset;
}
NCCL_DEVICE_INLINE void* ncclGetPeerPointer(ncclWindow_t w, size_t offset, ncclTeam team, int peer) {
  return w->peerPtr[w->rank + (peer - team.rank) * team.stride] + offset;
}

template <typename T>
NCCL_DEVICE_INLINE T* ncclSymPtr<T>::localPtr() const {
  return (T*)ncclGetLocalPointer(window, offset);
}
template <typename T>
NCCL_DEVICE_INLINE T* ncclSymPtr<T>::lsaPtr(int peer) const {
  return (T*)ncclGetLsaPointer(window, offset, peer);
}
template <typename T>
NCCL_DEVICE_INLINE T* ncclSymPtr<T>::peerPtr(int peer) const {
  return (T*)ncclGetPeerPointer(window, offset, peer);
}
template <typename T>
NCCL_DEVICE_INLINE T* ncclSymPtr<T>::peerPtr(ncclTeam team, int peer) const {
  return (T*)ncclGetPeerPointer(window, offset, team, peer);
}

/* ---- resource buffers (in ncclDevComm::resourceWindow, through its inlined table) ---- */
NCCL_DEVICE_INLINE void* ncclGetResourceBufferLsaPointer(ncclDevComm const& comm, ncclDevResourceHandle h, int peer) {
  return comm.resourceWindow_inlined.peerPtr[peer] + ncclGetResourceBufferOffset(h);
}
NCCL_DEVICE_INLINE void* ncclGetResourceBufferLocalPointer(ncclDevComm const& comm, ncclDevResourceHandle h) {
  return ncclGetResourceBufferLsaPointer(comm, h, comm.lsaRank);
}
NCCL_DEVICE_INLINE void* ncclGetResourceBufferPeerPointer(ncclDevComm const& comm, ncclDevResourceHandle h,
                                                          ncclTeam team, int peer) {
  return ncclGetResourceBufferLsaPointer(comm, h, ncclTeamRankToLsa(comm, team, peer));
}

/* ---- the LSA barrier ----
 *
 * Barrier `index` of a team: every member keeps an epoch (in its own resource memory, so consecutive kernels and
 * replays of a captured graph continue the sequence) and an inbox word per other member.
 *   arrive  each wave waits for its own stores, the group syncs, then (unless `order` is relaxed) one system-scope
 *           release fence writes this XCD's L2 back — user windows are ordinary cached memory — and the next epoch is
 *           stored into this rank's word of every other member's inbox;
 *   wait    polls this rank's inbox until every other member's word has reached the next epoch (wrap-safe compare),
 *           then (unless relaxed) one system-scope acquire invalidates this CU's caches, then the group syncs.
 * Inbox words live in uncached exported memory and are written and polled with system-scope relaxed atomics.
 * A relaxed order emits no fence.
 *
 * Every spin is bounded. The timed forms return ncclTimeout once timeoutCycles ticks (100 MHz) have passed without
 * every peer arriving, or when the communicator's abort word is set meanwhile; they record nothing. The untimed
 * forms give up as the library's own kernels do: on the abort word (recording NCCL_DEVICE_ERR_ABORT), on an error
 * already recorded, and after the communicator's spin timeout (recording NCCL_DEVICE_ERR_TIMEOUT);
 * ncclCommGetAsyncError then reports it. After a wait that gave up the barrier is out of step: tear down.
 *
 * The fences are system scope because peers may sit on other devices; no cross-device run of this code exists yet
 * (DESIGN.md §2.7). */
template <typename Coop>
struct ncclLsaBarrierSession {
  NCCL_DEVICE_INLINE ncclLsaBarrierSession(Coop coop, ncclDevComm const& comm, ncclTeam team,
                                           ncclLsaBarrierHandle handle, uint32_t index)
      : coop_(coop), comm_(comm), team_(team), handle_(handle), index_(index) {
    char* mine = (char*)ncclGetResourceBufferLocalPointer(comm, handle.bufHandle);
    epochPtr_ = (uint32_t*)mine + index;
    inbox_ = (uint32_t*)(mine + ncclLsaBarrierInboxOffset(handle.nBarriers)) + (size_t)index * team.nRanks;
    epoch_ = __hip_atomic_load(epochPtr_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

  NCCL_DEVICE_INLINE ncclLsaBarrierSession(Coop coop, ncclDevComm const& comm, ncclTeamTagLsa, uint32_t index)
      : ncclLsaBarrierSession(coop, comm, ncclTeamLsa(comm), comm.lsaBarrier, index) {}

  NCCL_DEVICE_INLINE ~ncclLsaBarrierSession() {
    coop_.sync();
    if (coop_.thread_rank() == 0) __hip_atomic_store(epochPtr_, epoch_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    coop_.sync();
  }

  ncclLsaBarrierSession(ncclLsaBarrierSession const&) = delete;
  ncclLsaBarrierSession& operator=(ncclLsaBarrierSession const&) = delete;

  NCCL_DEVICE_INLINE void arrive(Coop, std::memory_order order) {
    const int nPeers = team_.nRanks - 1;
    drain();  // each wave: its own stores have left the CU
    coop_.sync();
    const int tr = coop_.thread_rank();
    if (order != std::memory_order_relaxed && order != std::memory_order_acquire && order != std::memory_order_consume &&
        tr < (nPeers > 0 ? nPeers : 1)) {
      __atomic_thread_fence(__ATOMIC_RELEASE);  // system scope: buffer_wbl2 sc0 sc1
      drain();  // kept explicit: the compiler may drop the fence's own wait (MI355X_MICROARCH "Compiler hazard")
    }
    for (int i = tr; i < nPeers; i += coop_.size()) {
      const int peer = i < team_.rank ? i : i + 1;
      char* theirs = (char*)ncclGetResourceBufferPeerPointer(comm_, handle_.bufHandle, team_, peer);
      uint32_t* word = (uint32_t*)(theirs + ncclLsaBarrierInboxOffset(handle_.nBarriers)) +
                       (size_t)index_ * team_.nRanks + team_.rank;
      __hip_atomic_store(word, epoch_ + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }

  NCCL_DEVICE_INLINE void wait(Coop, std::memory_order order) { (void)waitFor(order, false, 0); }
  NCCL_DEVICE_INLINE void sync(Coop c, std::memory_order order) {
    arrive(c, order);
    wait(c, order);
  }
  /* The timed forms. After ncclTimeout this barrier index is out of step with its peers, as after an untimed give-up:
   * this rank's arrival is already in their inboxes and its epoch has advanced (the destructor stores it). Do not
   * retry on the same index: a retry would pair different epochs. Tear the DevComm down. */
  NCCL_DEVICE_INLINE ncclResult_t wait(Coop, std::memory_order order, uint64_t timeoutCycles) {
    return waitFor(order, true, timeoutCycles);
  }
  NCCL_DEVICE_INLINE ncclResult_t sync(Coop c, std::memory_order order, uint64_t timeoutCycles) {
    arrive(c, order);
    return wait(c, order, timeoutCycles);
  }

 private:
  Coop coop_;
  ncclDevComm const& comm_;
  ncclTeam team_;
  ncclLsaBarrierHandle handle_;
  uint32_t index_;
  uint32_t epoch_;
  uint32_t* epochPtr_;
  uint32_t* inbox_;

  static NCCL_DEVICE_INLINE void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

  NCCL_DEVICE_INLINE void recordError(uint32_t code) const {
    uint32_t expected = 0;
    __hip_atomic_compare_exchange_strong(comm_.errorWord, &expected, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_SYSTEM);
  }

  // the slow path of a spin, every 256 polls
  NCCL_DEVICE_INLINE bool giveUp(uint64_t t0, bool timed, uint64_t timeoutCycles) const {
    const uint64_t waited = __builtin_amdgcn_s_memrealtime() - t0;
    const bool aborted = __hip_atomic_load(comm_.abortFlag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
    if (timed) return aborted || waited > timeoutCycles;
    if (aborted) {
      recordError(NCCL_DEVICE_ERR_ABORT);
      return true;
    }
    if (__hip_atomic_load(comm_.errorWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) return true;
    if (waited > comm_.timeoutTicks) {
      recordError(NCCL_DEVICE_ERR_TIMEOUT);
      return true;
    }
    return false;
  }

  NCCL_DEVICE_INLINE ncclResult_t waitFor(std::memory_order order, bool timed, uint64_t timeoutCycles) {
    const int nPeers = team_.nRanks - 1;
    const uint32_t want = epoch_ + 1;
    const int tr = coop_.thread_rank();
    bool gaveUp = false;
    for (int i = tr; i < nPeers && !gaveUp; i += coop_.size()) {
      const uint32_t* word = inbox_ + (i < team_.rank ? i : i + 1);
      uint64_t t0 = 0;
      uint32_t polls = 0;
      while (!ncclLsaEpochReached(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), want)) {
        if (polls == 0) t0 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_sleep(1);
        if ((++polls & 255) == 0 && giveUp(t0, timed, timeoutCycles)) {
          gaveUp = true;
          break;
        }
      }
    }
    if (order != std::memory_order_relaxed && order != std::memory_order_release && tr < (nPeers > 0 ? nPeers : 1))
      __atomic_thread_fence(__ATOMIC_ACQUIRE);  // system scope: buffer_inv sc0 sc1
    gaveUp = ncclCoopSyncAny(coop_, gaveUp);
    epoch_ = want;
    return gaveUp ? ncclTimeout : ncclSuccess;
  }
};

#endif /* __HIPCC__ */

/* The reduce-copy family. Its plan function is host and device; the rest needs hipcc. */
#include "nccl_device_reduce_copy.h"

#endif /* NCCL_DEVICE_H_ */
