// device_abi.h — data layout shared by the host runtime and the gfx950 kernels.
//
// HBM layout per rank (all offsets in bytes, every region 16-byte aligned):
//
//   staging  (hipExtMallocWithFlags(..., hipDeviceMallocUncached), exported by HIP IPC)
//     [channel c < maxChannels][kind k < 2 (RS, AG)][slot s < nSlots][from < nRanks][slotBytes]
//     Written ONLY by peer `from` over xGMI (remote write-through stores); read ONLY by the owner.
//
//   flags    (uncached, exported by HIP IPC)
//     uint64 [channel][flag kind < 4][from < NCCL_AMD_MAX_RANKS]
//       RS_READY[c][from]  = number of RS slices `from` has written into my staging (monotonic)
//       RS_ACK[c][from]    = number of my RS slices `from` has consumed from ITS staging
//       AG_READY / AG_ACK  = the same for the all-gather direction
//       SYM_ENTER / SYM_MID / SYM_DONE[c][from] = epoch of the last symmetric (window) collective in
//                          which `from` entered / published its reduced block / finished reading peers
//       REG_SEND / REG_RECV[c][from] = `from`'s registered send / recv buffer as mapped in MY address space,
//                          stored before its SYM_ENTER (zero-copy collectives on ncclCommRegister buffers)
//       SIGNAL[0][from]    = number of signals `from` has raised for me (ncclPutSignal / ncclSignal; monotonic,
//                          channel 0's row only)
//     A word is written by exactly one remote rank and polled only by its owner.
//
//   LL lines (same uncached allocation as the flags, at DevComm::llOffset; reference prims_ll.h:108-158)
//     [channel < llChannels][parity < 2][from < nRanks][llBytes]: 16-byte lines {data32, flag32, data32,
//     flag32} written by `from` with one write-through store; the flag is the channel's LL epoch, so the
//     reader needs neither a flag word nor a fence. Parity = epoch & 1 (double buffering).
//
//   LL64 lines (the LL128-class protocol, at DevComm::ll64Offset; reference prims_ll128.h): same geometry,
//     64-byte lines = 4 lanes x 16 bytes = 56 bytes of payload + the 64-bit epoch flag in the last 8 bytes.
//     64 bytes, not the reference's 128: on MI355X a 128-byte line written by one wave-instruction is
//     observed torn, 64-byte segments are not (tests/native/store_atomicity_probe).
//     A separate area, so stale LL64 payload can never alias an LL flag position and vice versa.
//
//   counters (plain device memory, local)
//     uint64 [channel][ctr kind < CTR_KINDS (sendRS, recvRS, sendAG, recvAG, sym, ...)][peer < NCCL_AMD_MAX_RANKS]
//     Per-connection step counters (reference: conn->step, src/device/prims_simple.h:100-173),
//     kept in device memory so a captured hipGraph replays correctly.
#pragma once
#include <stdint.h>

#define NCCL_AMD_MAX_RANKS 16
#define NCCL_AMD_MAX_CHANNELS 256

namespace ncclamd {

enum StagingKind { STG_RS = 0, STG_AG = 1, STG_KINDS = 2 };
// FLG_PULL_READY / FLG_PULL_ACK and CTR_PULL_PUB / CTR_PULL_GOT: the AG-pull gather (kernels.h
// Channel::agPull) publishes ONE copy per step that every peer reads, so it keeps its own sequence (the
// per-pair AG counters diverge once a Reduce has pushed to its root only).
// FLG_REG_SEND / FLG_REG_RECV: the device-side pointer exchange of registered (ncclCommRegister) buffers —
// before its ENTER signal, rank `from` stores its send / recv buffer AS MAPPED IN THIS PROCESS into these
// words of the same channel (reference: the ptrExchange slots of prims_simple.h:748-846).
// FLG_SIGNAL and CTR_SIG_SENT / CTR_SIG_SEEN / CTR_SIG_ARRIVE: the one-sided operations (kernels.h rmaPutKernel /
// rmaWaitKernel), channel 0's rows only: the signal word per sender; signals this rank raised per
// peer, signals it consumed per peer, and the workgroups of a put launch that finished a message for a peer. Only the
// one-sided kernels touch these rows: the channel kernels load and store rows below CTR_CHAN_KINDS.
enum FlagKind {
  FLG_RS_READY = 0, FLG_RS_ACK = 1, FLG_AG_READY = 2, FLG_AG_ACK = 3,
  FLG_SYM_ENTER = 4, FLG_SYM_MID = 5, FLG_SYM_DONE = 6, FLG_PULL_READY = 7, FLG_PULL_ACK = 8,
  FLG_REG_SEND = 9, FLG_REG_RECV = 10, FLG_SIGNAL = 11, FLG_KINDS = 12
};
enum CtrKind {
  CTR_SEND_RS = 0, CTR_RECV_RS = 1, CTR_SEND_AG = 2, CTR_RECV_AG = 3, CTR_SYM = 4, CTR_LL = 5,
  CTR_PULL_PUB = 6, CTR_PULL_GOT = 7, CTR_CHAN_KINDS = 8,  // the rows a channel kernel keeps in LDS (ChanState)
  CTR_SIG_SENT = 8, CTR_SIG_SEEN = 9, CTR_SIG_ARRIVE = 10, CTR_KINDS = 11
};

// Ring / chain kernels (pipe.h; NCCL_ALGO=RING / TREE)
enum PipeKind { PIPE_RING_AR = 0, PIPE_RING_RS = 1, PIPE_RING_AG = 2, PIPE_CHAIN_AR = 3, PIPE_CHAIN_REDUCE = 4 };

// Device reduction kinds (reference ncclDevRedOp_t subset, src/include/device.h)
enum DevRedOp { DEV_SUM = 0, DEV_PROD = 1, DEV_MINMAX = 2, DEV_PREMULSUM = 3, DEV_SUMPOSTDIV = 4, DEV_NUMOPS = 5 };

// Error codes written by a kernel into the host-visible error word.
// DERR_MISMATCH: a peer ran another kernel kind for the same collective (registered zero-copy vs staged; the
// wait probe in kernels.h waitAll), reported instead of waiting for the spin timeout.
enum DevError { DERR_NONE = 0, DERR_TIMEOUT = 1, DERR_ABORT = 2, DERR_MISMATCH = 3 };

struct DevComm {
  int rank;
  int nRanks;
  int nSlots;
  int maxChannels;
  uint64_t slotBytes;
  uint64_t timeoutTicks;  // s_memrealtime ticks (100 MHz) before a spin gives up
  char* staging[NCCL_AMD_MAX_RANKS];     // every rank's staging base as mapped here
  uint64_t* flags[NCCL_AMD_MAX_RANKS];   // every rank's flag block as mapped here
  uint64_t* counters;                    // local step counters
  uint64_t llOffset;                     // LL line area inside every rank's flag allocation
  uint64_t llBytes;                      // line bytes per (channel, parity, sender)
  uint64_t ll64Offset;                   // LL64 line area (same geometry as the LL area)
  int llChannels;
  uint32_t* abortFlag;                   // host-pinned; nonzero = abort
  uint32_t* errorWord;                   // host-pinned; first DevError recorded
};

// Kernel argument block (passed by value, < 4 KiB like the reference's ncclDevKernelArgs4K,
// src/device/common.h:435-449).
struct CollArgs {
  const void* sendbuff;
  void* recvbuff;
  const DevComm* comm;
  uint64_t count;      // AR/Reduce: elements; RS: recvcount; AG: sendcount (bytes for AG)
  uint64_t chunk;      // elements per rank block (AR: alignUp(divUp(count,n),EPP); RS/AG: count)
  uint64_t part;       // elements per channel within a rank block
  uint64_t slice;      // elements per pipeline step (per peer)
  uint64_t redArg;     // scalar / xormask / divisor bits
  const void* redArgPtr;  // device scalar (PreMulSum with ncclScalarDevice), else nullptr
  int nSteps;
  int root;
  int aligned;         // send/recv base pointers are 16-byte aligned
  int protoFlags;      // NCCL_AMD_PROTO_FLAGS diagnostics (kernels.h collKernel)
  // Ring AllReduce (PIPE_RING_AR) and the reference-order direct AllReduce (COLL_ARREF) in the reference's
  // partition: channel parts lo / mid (= part) / hi (ncclCollCbdPart, reference src/include/device.h:337-361),
  // each walked in loops of n chunks of `chunk` elements (all_reduce.h:21-38). Unused by every other kernel.
  uint64_t cbdLo, cbdHi;
  // ... and refSub workgroups per reference channel part: workgroup c serves part c / refSub and, inside every
  // chunk of that part, the sub-chunk c % refSub (an element's fold order depends only on its loop and chunk,
  // never on which workgroup moves it), so the reference's channel count and this launch's parallelism are
  // independent.
  uint32_t refSub;
  uint32_t refPad;
};

// Staged batch: up to kMaxCollBatch ops of one group with the same collective, type and op (and the same
// one-shot / direct choice) in ONE collBatchKernel launch; op k runs on channels chOff[k] .. + nch[k] - 1.
constexpr int kMaxCollBatch = 8;
struct CollBatchArgs {
  CollArgs op[kMaxCollBatch];
  int chOff[kMaxCollBatch];
  int nch[kMaxCollBatch];
  int nOps;
};

// LL batch: up to kMaxLLBatch small ops of one group (same comm, stream, type and op; any of AllReduce,
// ReduceScatter, AllGather, Reduce) run by ONE launch (reference: ops of a group aggregated into one kernel
// plan, enqueue.cc:405-470).
constexpr int kMaxLLBatch = 32;
enum LLColl { LL_AR = 0, LL_RS = 1, LL_AG = 2, LL_REDUCE = 3, LL_BCAST = 4 };
enum LLProto { LLP_LL = 0, LLP_LL64 = 1 };
constexpr int kLL64Payload = 56;  // payload bytes per 64-byte LL64 line
struct LLOp {
  const void* send;
  void* recv;
  uint64_t count;  // elements (AllReduce: of the buffer; ReduceScatter / AllGather: of one rank block)
  uint64_t chunk;  // elements per rank block (fold order of each element's owner)
  uint64_t part;   // 8-byte payloads per channel
  int nch;         // channels this op uses
  int chOff;       // first channel (batches spread their ops over the LL channels)
  int coll;        // LLColl
  int root;        // LL_REDUCE: the rank that folds and stores (the others send and poll only); LL_BCAST: the sender
  int proto;       // LLProto: LL (part = 8-byte payloads) or LL64 (part = 64-byte lines of 56 payload bytes)
};
// The kernel arguments hold room for K ops: a lone op launches with K = 1 (88 bytes of kernel arguments
// instead of 1.8 KiB; the host issue cost of a launch grows with its argument bytes, about 3 us at 64 B
// vs 6.5 us at 2 KiB on the MI355X box, scripts/launch_probe.hip).
// A batch (K > 1) also carries, per LL channel (at most 32), the bit mask of the ops that run on it: a work-group
// reads ONE word of the argument block to find its ops, instead of every op's channel range (each op descriptor
// its own line of the argument block, and every work-group of the launch reading them all).
constexpr int kMaxLLChannels = 32;
template <int K>
struct LLArgs {
  const DevComm* comm;
  uint64_t* counters;  // comm->counters (device): the channels' LL epochs load beside the DevComm, not after it
  uint64_t redArg;
  const void* redArgPtr;
  int nOps;
  uint32_t chMask[K > 1 ? kMaxLLChannels : 1];  // bit k: op k runs on this channel (K > 1 only)
  LLOp ops[K];
};
static_assert(kMaxLLBatch <= 32, "LLArgs::chMask holds one bit per op");
using LLBatchArgs = LLArgs<kMaxLLBatch>;

// Symmetric (window) collective arguments: every rank's buffers as mapped in this process (reference
// ncclSymPtr::peerPtr, src/device/symmetric/kernel.cuh), so peers are read and written directly.
// regMode (buffers registered with ncclCommRegister, reference src/register/coll_reg.cc:326-395): the host
// knows only where ITS OWN buffers are mapped in every peer, so send[r] / recv[r] (r != rank) hold MY buffers
// as mapped in rank r; the kernel hands them to rank r through r's FLG_REG_SEND / FLG_REG_RECV words and reads
// the peers' buffers from its own words after the ENTER handshake (the reference's ptrExchange,
// prims_simple.h:748-846). `aligned` then carries only the count condition: pointer alignment of every
// rank's buffers is decided in the kernel, from the exchanged pointers, identically on every rank.
struct SymArgs {
  const DevComm* comm;
  const char* send[NCCL_AMD_MAX_RANKS];  // rank r's sendbuff (regMode: my sendbuff as mapped in rank r)
  char* recv[NCCL_AMD_MAX_RANKS];        // rank r's recvbuff (regMode: my recvbuff as mapped in rank r)
  uint64_t count;      // AR: elements; RS: recvcount; AG: sendcount
  uint64_t chunk;      // elements per rank block
  uint64_t part;       // elements per channel (AR two-shot / RS / AG: within a block; one-shot: of the buffer)
  uint64_t redArg;
  const void* redArgPtr;
  int aligned;
  int wtPublish;       // bytes peers read (AR fold result, AG own block) stored write-through: no L2 write-back
  int regMode;         // buffers registered with ncclCommRegister: device-side pointer exchange (above)
  int relFence;        // publish with a system release fence even after write-through stores (across devices)
};

// Mapping check at communicator init (mapcheck.cc, kernels.hip mapCheckKernel): the words this rank stores into
// peer p's staging slab (w[p][0]) and flag block (w[p][1]) through its mappings of them.
struct MapCheckArgs {
  uint64_t w[NCCL_AMD_MAX_RANKS][2][2];
  uint64_t probeOff;  // the check area inside every rank's flag allocation (same offset everywhere)
  int skip;           // tests (NCCL_AMD_MAPCHECK_FAULT): no stores, as a mapping that drops them
};

__host__ __device__ inline uint64_t stagingOffset(const DevComm& dc, int c, int kind, int slot, int from) {
  return ((((uint64_t)c * STG_KINDS + kind) * dc.nSlots + slot) * dc.nRanks + from) * dc.slotBytes;
}
__host__ __device__ inline uint64_t llLineOffset(const DevComm& dc, int c, int parity, int from) {
  return dc.llOffset + (((uint64_t)c * 2 + parity) * dc.nRanks + from) * dc.llBytes;
}
__host__ __device__ inline uint64_t ll64LineOffset(const DevComm& dc, int c, int parity, int from) {
  return dc.ll64Offset + (((uint64_t)c * 2 + parity) * dc.nRanks + from) * dc.llBytes;
}
__host__ __device__ inline uint64_t flagIndex(int c, int kind, int from) {
  return ((uint64_t)c * FLG_KINDS + kind) * NCCL_AMD_MAX_RANKS + from;
}
__host__ __device__ inline uint64_t ctrIndex(int c, int kind, int peer) {
  return ((uint64_t)c * CTR_KINDS + kind) * NCCL_AMD_MAX_RANKS + peer;
}
// How a Broadcast's buffer of `count` bytes is cut (kernels.h Channel<.., COLL_BCAST> and llBcastOp; host-callable so
// that tests/native/bcast_plan_test walks exactly what those kernels walk; the same arithmetic as sliceRange /
// Channel::blockLen of the other collectives): rank block q holds blockLenOf elements; channel c
// moves elements [lo, hi) of a block of blockLen elements at pipeline step s; LL channel part j holds payload units
// [lo, hi) of `units`.
__host__ __device__ inline uint64_t minU64(uint64_t a, uint64_t b) { return b < a ? b : a; }
__host__ __device__ inline uint64_t blockLenOf(uint64_t count, uint64_t chunk, int q) {
  const uint64_t b = (uint64_t)q * chunk;
  return b >= count ? 0 : minU64(chunk, count - b);
}
__host__ __device__ inline void sliceBounds(uint64_t part, uint64_t slice, int c, int s, uint64_t blockLen, uint64_t& lo,
                                            uint64_t& hi) {
  const uint64_t pEnd = minU64((uint64_t)(c + 1) * part, blockLen);
  lo = minU64((uint64_t)c * part + (uint64_t)s * slice, pEnd);
  hi = minU64(lo + slice, pEnd);
}
__host__ __device__ inline void llPartBounds(uint64_t part, int j, uint64_t units, uint64_t& lo, uint64_t& hi) {
  lo = minU64((uint64_t)j * part, units);
  hi = minU64(lo + part, units);
}

// ---- point-to-point (kernels.h p2pKernel, p2p.cc) ----
// A send or a recv of `bytes` is cut the same way on both sides, from the byte count and per-communicator constants
// alone: nch = clamp(ceil(bytes / chunk), minCh, maxCh) channel parts of alignUp(ceil(bytes / nch), 16) bytes (then
// nch = ceil(bytes / part), so that no channel below nch is empty), part j on physical channel j, walked in slices of
// p2pSliceBytes(slotBytes) through the pair's RS slots. An empty message has no channels: neither side handshakes.
// Host-callable so that tests/native/p2p_plan_test walks exactly what the kernel walks.
struct P2pCut {
  int nch;
  uint64_t part;
};
__host__ __device__ inline uint64_t p2pSliceBytes(uint64_t slotBytes) { return slotBytes & ~(uint64_t)15; }
__host__ __device__ inline P2pCut p2pCut(uint64_t bytes, uint64_t chunk, int minCh, int maxCh) {
  P2pCut c = {0, 0};
  if (bytes == 0) return c;
  if (chunk < 16) chunk = 16;
  uint64_t nch = (bytes + chunk - 1) / chunk;
  if (nch < (uint64_t)minCh) nch = (uint64_t)minCh;
  if (nch > (uint64_t)maxCh) nch = (uint64_t)maxCh;
  if (nch < 1) nch = 1;
  c.part = ((bytes + nch - 1) / nch + 15) / 16 * 16;
  c.nch = (int)((bytes + c.part - 1) / c.part);
  return c;
}
// slices of channel part j: steps, and bytes [lo, hi) of the message at step s (sliceBounds over the whole message)
__host__ __device__ inline int p2pSteps(uint64_t bytes, uint64_t part, uint64_t slice, int j) {
  uint64_t lo, hi;
  sliceBounds(part, part, j, 0, bytes, lo, hi);
  return (int)((hi - lo + slice - 1) / slice);
}

// ---- zero-copy AlltoAll / Gather on symmetric windows (kernels.h symA2AKernel, enqueue.cc) ----
// Every rank block of B bytes is cut alike, from B and rank-uniform constants alone (the function is not given the
// rank, so every rank launches the same grid): nch = clamp(ceil(B / minChannelBytes), max(minCTAs, 1), cap) channels
// of alignUp(ceil(B / nch), 16) bytes; channel c owns bytes [min(c * part, B), min((c + 1) * part, B)) of EVERY
// block. A channel whose range is empty still runs the handshake (the channels' epochs stay in step).
// Host-callable so that tests/native/sym_a2a_plan_test walks exactly what the kernel walks.
struct SymA2ACut {
  int nch;
  uint64_t part;
};
__host__ __device__ inline SymA2ACut symA2ACut(uint64_t bytes, uint64_t minChannelBytes, int minCTAs, int cap) {
  if (minChannelBytes < 16) minChannelBytes = 16;
  uint64_t nch = (bytes + minChannelBytes - 1) / minChannelBytes;
  if (nch < (uint64_t)(minCTAs > 1 ? minCTAs : 1)) nch = (uint64_t)(minCTAs > 1 ? minCTAs : 1);
  if (nch > (uint64_t)(cap > 1 ? cap : 1)) nch = (uint64_t)(cap > 1 ? cap : 1);
  SymA2ACut c;
  c.nch = (int)nch;
  c.part = ((bytes + nch - 1) / nch + 15) / 16 * 16;
  return c;
}
__host__ __device__ inline void symA2APart(uint64_t part, int c, uint64_t bytes, uint64_t& lo, uint64_t& hi) {
  lo = minU64((uint64_t)c * part, bytes);
  hi = minU64(lo + part, bytes);
}
enum SymA2AMode { SYM_A2A_ALLTOALL = 0, SYM_A2A_GATHER = 1 };
// Kernel arguments: every rank's sendbuff as mapped in this process (the same offset in every rank's window) and
// this rank's recvbuff, which needs no window (only sendbuffs are read remotely; GATHER: used on the root only).
struct SymA2AArgs {
  const DevComm* comm;
  const char* send[NCCL_AMD_MAX_RANKS];
  char* recv;
  uint64_t bytes;   // B: bytes per rank block
  uint64_t part;    // bytes per channel within a block (symA2ACut)
  int mode;         // SymA2AMode
  int root;         // GATHER
  int elementwise;  // NCCL_AMD_FORCE_ELEMENTWISE
  int pad;
};

// One message of a stream, and one stream = the in-order messages of one group to (recv == 0) or from one peer.
// Stream i runs on workgroups wgOff .. wgOff + nch - 1 of its launch, workgroup wgOff + j on physical channel j, which
// walks the stream's messages in order and skips those cut into j or fewer parts.
struct P2pMsg {
  uint64_t ptr;
  uint64_t bytes;
  uint64_t part;
  uint32_t nch;
  uint32_t pad;
};
struct P2pStream {
  uint16_t wgOff, nch, msgOff, nMsgs;
  uint8_t peer, recv;
  uint16_t pad;
};
// Kernel arguments (< 4 KiB): S streams and M messages inline; a lone transfer or a pair exchange launches with the
// small block (the host issue cost of a launch grows with its argument bytes, LLArgs above).
constexpr int kP2pMaxStreams = 2 * (NCCL_AMD_MAX_RANKS - 1);
constexpr int kP2pMaxMsgs = 96;
template <int S, int M>
struct P2pArgs {
  const DevComm* comm;
  int nStreams;
  int protoFlags;    // CollArgs::protoFlags
  int elementwise;   // NCCL_AMD_FORCE_ELEMENTWISE
  int pad;
  P2pStream st[S];
  P2pMsg msg[M];
};
static_assert(sizeof(P2pArgs<kP2pMaxStreams, kP2pMaxMsgs>) < 4096, "kernel arguments stay under 4 KiB");

// ---- one-sided operations (kernels.h rmaPutKernel / rmaWaitKernel, rma.cc) ----
// One put or signal (bytes == 0: a signal, no workgroup copies) and one stream = the in-order messages of one batch to
// one peer. Stream i runs on workgroups wgOff .. wgOff + nch - 1 of its launch; workgroup wgOff + j copies part j
// (p2pCut's) of every message cut into more than j parts, and workgroup wgOff posts the stream's signals in order.
struct RmaMsg {
  uint64_t src;    // localbuff
  uint64_t dst;    // the target inside the peer's window, as mapped in this process
  uint64_t bytes;
  uint64_t part;
  uint32_t nch;
  uint32_t pad;
};
struct RmaStream {
  uint16_t wgOff, nch, msgOff, nMsgs;
  uint8_t peer;
  uint8_t pad[3];
};
constexpr int kRmaMaxStreams = NCCL_AMD_MAX_RANKS;  // one per peer, self included
constexpr int kRmaMaxMsgs = 96;
template <int S, int M>
struct RmaArgs {
  const DevComm* comm;
  int nStreams;
  int protoFlags;    // CollArgs::protoFlags (8: no release fence before a signal)
  int elementwise;   // NCCL_AMD_FORCE_ELEMENTWISE
  int pad;
  RmaStream st[S];
  RmaMsg msg[M];
};
static_assert(sizeof(RmaArgs<kRmaMaxStreams, kRmaMaxMsgs>) < 4096, "kernel arguments stay under 4 KiB");
// ncclWaitSignal: per peer, the signals to consume (descriptors naming one peer added up); lane i serves entry i
struct RmaWaitArgs {
  const DevComm* comm;
  int n;
  int pad;
  struct {
    int peer;
    uint32_t opCnt;
  } d[NCCL_AMD_MAX_RANKS];
};

// The k-th peer (k = 1 .. n-1) that channel c of rank `me` visits in a workgroup-wide multi-peer loop: the
// staged scatter's pushes, the pull gather's reads, the zero-copy kernels' reads. Rotated by channel: with one
// order on every channel, all of a rank's channels would sit on the SAME peer's xGMI link at step position k;
// rotated, any n-1 consecutive channels put position k on all n-1 peers once (a Latin square), and for a fixed
// (c, k) the ranks' choices are a shift, so every peer is also the source / target of exactly one rank.
// Data placement and fold order never depend on it (tests/native/plan_test `peers`).
__host__ __device__ inline int chanPeer(int me, int n, int c, int k) {
  return (me + 1 + (k - 1 + c) % (n - 1)) % n;
}

}  // namespace ncclamd
