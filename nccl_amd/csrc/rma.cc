// rma.cc — the one-sided operations ncclPutSignal / ncclSignal / ncclWaitSignal: entry points, argument checks, the
// per-group host plan and its launches.
//
// Reference: src/nccl.h.in:612-692, src/collectives.cc:315-400 (entry points), src/enqueue.cc:2807-3008 (rmaTaskAppend:
// the argument checks, in this order and with these codes), docs/userguide/source/api/p2p.rst:51-127.
//
// The plan: a put stores straight into the target window as ncclCommWindowRegister mapped it here
// (ncclWindow_vidmem::peerPtr), so there is one copy and nothing to agree on with the peer. The consecutive puts and
// signals of one group on one communicator and stream form a batch; per target peer the batch's messages form a stream
// in issue order, cut with p2pCut and its knobs, on a fixed set of workgroups whose first posts the stream's signals
// one after the other. A batch's streams are packed whole into launches of at most chanCap workgroups; a stream is
// never split between launches. A ncclWaitSignal closes a batch and is a launch of one wave of its own.
#include <string.h>

#include <algorithm>

#include "core.h"

namespace ncclamd {

static P2pCut rmaCutFor(const ncclComm* comm, size_t bytes) {
  const int mx = std::max(1, std::min(comm->tune.p2pMaxCh, comm->chanCap));
  return p2pCut(bytes, (uint64_t)comm->tune.p2pChunkBytes, std::min(comm->tune.p2pMinCh, mx), mx);
}

namespace {
struct Batch {  // the open run of puts and signals: per peer its messages, and the peers in first-use order
  hipStream_t stream = nullptr;
  std::vector<RmaMsg> to[NCCL_AMD_MAX_RANKS];
  std::vector<int> peers;
  bool empty() const { return peers.empty(); }
};
}  // namespace

// Pack the batch's streams whole into launches: a stream that no longer fits (workgroups, message descriptors) opens
// the next launch. Streams of different peers share no word, so their order between launches is free.
static ncclResult_t closeBatch(const ncclComm* comm, Batch& b, RmaPlan* plan) {
  if (b.empty()) return ncclSuccess;
  const int budget = std::max(1, comm->chanCap);
  RmaStep cur;
  cur.wait = false;
  cur.stream = b.stream;
  cur.put.grid = 0;
  memset(&cur.w, 0, sizeof(cur.w));
  auto flush = [&]() {
    if (cur.put.grid > 0) plan->steps.push_back(cur);
    cur.put.grid = 0;
    cur.put.streams.clear();
    cur.put.msgs.clear();
  };
  for (int peer : b.peers) {
    const std::vector<RmaMsg>& msgs = b.to[peer];
    int nch = 1;  // a stream of bare signals still needs its posting workgroup
    size_t bytes = 0;
    for (const RmaMsg& m : msgs) {
      nch = std::max(nch, (int)m.nch);
      bytes += m.bytes;
    }
    plan->maxPeerBytes = std::max(plan->maxPeerBytes, bytes);
    if (nch > budget || msgs.size() > (size_t)kRmaMaxMsgs) {
      WARN("internal: a put stream of %d workgroups and %zu messages fits no launch (at most %d and %d)", nch,
           msgs.size(), budget, kRmaMaxMsgs);
      return ncclInternalError;
    }
    if (cur.put.grid + nch > budget || cur.put.msgs.size() + msgs.size() > (size_t)kRmaMaxMsgs ||
        cur.put.streams.size() + 1 > (size_t)kRmaMaxStreams)
      flush();
    RmaStream s;
    memset(&s, 0, sizeof(s));
    s.wgOff = (uint16_t)cur.put.grid;
    s.nch = (uint16_t)nch;
    s.msgOff = (uint16_t)cur.put.msgs.size();
    s.nMsgs = (uint16_t)msgs.size();
    s.peer = (uint8_t)peer;
    cur.put.streams.push_back(s);
    cur.put.msgs.insert(cur.put.msgs.end(), msgs.begin(), msgs.end());
    cur.put.grid += nch;
    b.to[peer].clear();
  }
  flush();
  b.peers.clear();
  return ncclSuccess;
}

ncclResult_t rmaPlan(ncclComm* comm, const std::vector<RmaOp>& ops, RmaPlan* plan) {
  plan->steps.clear();
  plan->maxPeerBytes = 0;
  Batch b;
  for (const RmaOp& op : ops) {
    if (op.wait) {
      NCCLCHECK(closeBatch(comm, b, plan));
      RmaStep st;
      st.wait = true;
      st.stream = op.stream;
      st.put.grid = 0;
      memset(&st.w, 0, sizeof(st.w));
      for (int r = 0; r < comm->nRanks && r < NCCL_AMD_MAX_RANKS; r++) {
        if (op.waitCnt[r] == 0) continue;
        st.w.d[st.w.n].peer = r;
        st.w.d[st.w.n].opCnt = op.waitCnt[r];
        st.w.n++;
      }
      if (st.w.n == 0) return ncclInternalError;  // (checked at the entry point)
      plan->steps.push_back(st);
      continue;
    }
    if (op.peer < 0 || op.peer >= comm->nRanks) return ncclInternalError;  // (checked at the entry point)
    // another stream closes the batch; so does a message that would overflow its peer's stream (the messages of one
    // stream stay in one launch, so the split falls between batches, in issue order)
    if (!b.empty() && (b.stream != op.stream || b.to[op.peer].size() >= (size_t)kRmaMaxMsgs)) NCCLCHECK(closeBatch(comm, b, plan));
    if (b.empty()) b.stream = op.stream;
    const P2pCut cut = rmaCutFor(comm, op.bytes);  // count == 0: no parts, a signal
    if (b.to[op.peer].empty()) b.peers.push_back(op.peer);
    b.to[op.peer].push_back({(uint64_t)(uintptr_t)op.src, (uint64_t)(uintptr_t)op.dst, (uint64_t)op.bytes, cut.part, (uint32_t)cut.nch, 0});
  }
  return closeBatch(comm, b, plan);
}

// Host-side guard before an rmaPutKernel launches (p2p.cc p2pCheckGrid's rule): the grid within the co-resident cap,
// the workgroup ranges and message ranges of the streams exactly the launch's, every peer a rank, no message cut into
// more parts than its stream has workgroups.
static ncclResult_t rmaCheckGrid(const ncclComm* comm, const RmaLaunch& l) {
  bool good = l.grid >= 1 && l.grid <= std::max(1, comm->chanCap) && !l.streams.empty() &&
              l.streams.size() <= (size_t)kRmaMaxStreams && l.msgs.size() <= (size_t)kRmaMaxMsgs;
  int off = 0;
  size_t moff = 0;
  for (size_t i = 0; good && i < l.streams.size(); i++) {
    const RmaStream& s = l.streams[i];
    good = s.wgOff == off && s.nch >= 1 && s.msgOff == moff && s.nMsgs >= 1 && s.peer < comm->nRanks;
    for (size_t k = 0; good && k < s.nMsgs; k++)
      good = moff + k < l.msgs.size() && l.msgs[moff + k].nch <= s.nch && (l.msgs[moff + k].bytes == 0) == (l.msgs[moff + k].nch == 0);
    off += s.nch;
    moff += s.nMsgs;
  }
  if (good && off == l.grid && moff == l.msgs.size()) return ncclSuccess;
  WARN("internal: a put launch of %d workgroups (cap %d) was refused before launch", l.grid, comm->chanCap);
  return ncclInternalError;
}

ncclResult_t rmaLaunchPlan(ncclComm* comm, const RmaPlan& plan) {
  for (const RmaStep& s : plan.steps)
    if (!s.wait) NCCLCHECK(rmaCheckGrid(comm, s.put));
  for (const RmaStep& s : plan.steps) {
    hipStream_t stream = comm->sharedDevInProcess ? comm->internalStream : s.stream;
    if (s.wait) {
      TRACE("rma wait: rank %d, %d peers", comm->rank, s.w.n);
      NCCLCHECK(launchRmaWaitKernel(comm, s.w, stream));
    } else {
      TRACE("rma launch: rank %d, %zu streams, %zu messages, %d workgroups", comm->rank, s.put.streams.size(),
            s.put.msgs.size(), s.put.grid);
      NCCLCHECK(launchRmaPutKernel(comm, s.put, stream));
    }
    if (comm->fdServer) {  // (enqueue.cc noteLaunch)
      hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(stream, &st) == hipSuccess && st == hipStreamCaptureStatusNone) ipcNoteLaunch(stream, comm->device);
      else (void)hipGetLastError();
    }
  }
  return ncclSuccess;
}

static ncclResult_t rmaFail(ncclResult_t r) {
  groupRecordError(r);
  return r;
}

// The checks every entry point shares (p2p.cc p2pCheck's): the comm first, as ncclAllReduce does; then the datatype
// and the communicator's error state.
static ncclResult_t rmaCheck(const char* opName, ncclComm* comm, ncclDataType_t datatype, int* ts) {
  logInit();
  ncclResult_t ret = commCheck(comm, opName, "comm");
  if (ret == ncclSuccess && ((int)datatype < 0 || datatype >= ncclNumTypes)) {
    WARN("%s : invalid type %d", opName, (int)datatype);
    ret = ncclInvalidArgument;
  }
  if (ret == ncclSuccess) {
    commPollAsync(comm);
    if (comm->asyncResult.load() != ncclSuccess) {
      WARN("%s: communicator is in error state %d", opName, comm->asyncResult.load());
      ret = ncclInvalidUsage;
    }
  }
  if (ret != ncclSuccess) return rmaFail(ret);
  *ts = typeSize(datatype);
  return ret;
}

static ncclResult_t peerCheck(const char* opName, int r, const ncclComm* comm) {
  if (r >= 0 && r < comm->nRanks) return ncclSuccess;
  WARN("%s : invalid peer %d (peer should be in the 0..%d range)", opName, r, comm->nRanks);
  return rmaFail(ncclInvalidArgument);
}

// reference enqueue.cc:2825-2841
static ncclResult_t ctxCheck(int ctx, int sigIdx, unsigned int flags) {
  if (ctx != 0) {
    WARN("Context %d is invalid (must be 0)", ctx);
    return rmaFail(ncclInvalidArgument);
  }
  if (sigIdx != 0) {
    WARN("Signal index %d is invalid (must be 0)", sigIdx);
    return rmaFail(ncclInvalidArgument);
  }
  if (flags != 0) {
    WARN("Flags %u is invalid (must be 0)", flags);
    return rmaFail(ncclInvalidArgument);
  }
  return ncclSuccess;
}

// Record the op: inside a group as it is, outside as a group of its own (launched before the call returns).
static ncclResult_t rmaSubmit(const RmaOp& op) {
  const bool own = !groupActive();
  if (own) groupStartInternal();
  groupDeferRma(op);
  return own ? groupEndInternal() : ncclSuccess;
}

}  // namespace ncclamd

using namespace ncclamd;

#define NCCL_ALIAS(ret, name, ...) extern "C" __attribute__((visibility("default"), alias(#name))) ret p##name(__VA_ARGS__);

NCCL_EXPORT ncclResult_t ncclPutSignal(const void* localbuff, size_t count, ncclDataType_t datatype, int peer,
                                       ncclWindow_t peerWin, size_t peerWinOffset, int sigIdx, int ctx, unsigned int flags,
                                       ncclComm_t comm, hipStream_t stream) {
  ROCTX_RANGE("ncclPutSignal comm=%p count=%zu datatype=%d peer=%d offset=%zu", (void*)comm, count, (int)datatype, peer,
              peerWinOffset);
  int ts = 0;
  NCCLCHECK(rmaCheck("PutSignal", comm, datatype, &ts));
  NCCLCHECK(peerCheck("PutSignal", peer, comm));
  NCCLCHECK(ctxCheck(ctx, sigIdx, flags));
  const size_t bytes = count * (size_t)ts;
  if (peerWin == nullptr) {
    WARN("ncclPutSignal: peerWin is NULL");
    return rmaFail(ncclInvalidArgument);
  }
  if (localbuff == nullptr) {
    WARN("ncclPutSignal: localbuff is NULL");
    return rmaFail(ncclInvalidArgument);
  }
  if (findSymWindow(comm, localbuff, bytes) == nullptr) {
    WARN("ncclPutSignal: localbuff [%p, +%zu) is not inside a NCCL_WIN_COLL_SYMMETRIC window of this communicator",
         localbuff, bytes);
    return rmaFail(ncclInvalidArgument);
  }
  if (std::find(comm->windows.begin(), comm->windows.end(), peerWin) == comm->windows.end() || peerWin->comm != comm) {
    WARN("ncclPutSignal: peerWin %p is not a window of this communicator", (void*)peerWin);
    return rmaFail(ncclInvalidArgument);
  }
  const size_t peerSize = peerWin->peerSize[peer];
  if (peerWinOffset > peerSize || bytes > peerSize - peerWinOffset) {
    WARN("ncclPutSignal: [%zu, +%zu) exceeds the %zu bytes rank %d registered for window %p", peerWinOffset, bytes,
         peerSize, peer, (void*)peerWin);
    return rmaFail(ncclInvalidArgument);
  }
  INFO("PutSignal: opCount %lx localbuff %p count %zu datatype %d peer %d win %p offset %zu comm %p [nranks=%d] stream %p",
       (unsigned long)comm->opCount, localbuff, count, (int)datatype, peer, (void*)peerWin, peerWinOffset, (void*)comm,
       comm->nRanks, (void*)stream);
  RmaOp op;
  memset(&op, 0, sizeof(op));
  op.comm = comm;
  op.stream = stream;
  op.src = localbuff;
  op.dst = peerWin->peerPtr[peer] + peerWinOffset;
  op.bytes = bytes;
  op.peer = peer;
  return rmaSubmit(op);
}
NCCL_ALIAS(ncclResult_t, ncclPutSignal, const void*, size_t, ncclDataType_t, int, ncclWindow_t, size_t, int, int, unsigned int,
           ncclComm_t, hipStream_t)

NCCL_EXPORT ncclResult_t ncclSignal(int peer, int sigIdx, int ctx, unsigned int flags, ncclComm_t comm, hipStream_t stream) {
  ROCTX_RANGE("ncclSignal comm=%p peer=%d", (void*)comm, peer);
  int ts = 0;
  NCCLCHECK(rmaCheck("Signal", comm, ncclInt8, &ts));
  NCCLCHECK(peerCheck("Signal", peer, comm));
  NCCLCHECK(ctxCheck(ctx, sigIdx, flags));
  INFO("Signal: opCount %lx peer %d comm %p [nranks=%d] stream %p", (unsigned long)comm->opCount, peer, (void*)comm,
       comm->nRanks, (void*)stream);
  RmaOp op;
  memset(&op, 0, sizeof(op));
  op.comm = comm;
  op.stream = stream;
  op.peer = peer;
  return rmaSubmit(op);
}
NCCL_ALIAS(ncclResult_t, ncclSignal, int, int, int, unsigned int, ncclComm_t, hipStream_t)

NCCL_EXPORT ncclResult_t ncclWaitSignal(int nDesc, ncclWaitSignalDesc_t* signalDescs, ncclComm_t comm, hipStream_t stream) {
  ROCTX_RANGE("ncclWaitSignal comm=%p nDesc=%d", (void*)comm, nDesc);
  int ts = 0;
  NCCLCHECK(rmaCheck("WaitSignal", comm, ncclInt32, &ts));
  if (signalDescs == nullptr || nDesc <= 0) {
    WARN("ncclWaitSignal: invalid arguments");
    return rmaFail(ncclInvalidArgument);
  }
  RmaOp op;
  memset(&op, 0, sizeof(op));
  op.comm = comm;
  op.stream = stream;
  op.wait = true;
  for (int i = 0; i < nDesc; i++) {  // reference enqueue.cc:2894-2908
    const ncclWaitSignalDesc_t& d = signalDescs[i];
    if (d.opCnt <= 0) {
      WARN("ncclWaitSignal: descriptor %d has invalid opCnt %d", i, d.opCnt);
      return rmaFail(ncclInvalidArgument);
    }
    if (d.sigIdx != 0) {
      WARN("ncclWaitSignal: descriptor %d has invalid sigIdx %d (must be 0)", i, d.sigIdx);
      return rmaFail(ncclInvalidArgument);
    }
    if (d.ctx != 0) {
      WARN("ncclWaitSignal: descriptor %d has invalid context %d (must be 0)", i, d.ctx);
      return rmaFail(ncclInvalidArgument);
    }
    if (d.peer < 0 || d.peer >= comm->nRanks) {
      WARN("ncclWaitSignal: descriptor %d has invalid peer %d (peer should be in the 0..%d range)", i, d.peer, comm->nRanks);
      return rmaFail(ncclInvalidArgument);
    }
    if ((uint64_t)op.waitCnt[d.peer] + (uint64_t)d.opCnt > 0x7fffffffu) {
      WARN("ncclWaitSignal: the descriptors of peer %d add up to more than INT_MAX signals", d.peer);
      return rmaFail(ncclInvalidArgument);
    }
    op.waitCnt[d.peer] += (uint32_t)d.opCnt;  // descriptors naming the same peer add up
  }
  INFO("WaitSignal: opCount %lx nDesc %d comm %p [nranks=%d] stream %p", (unsigned long)comm->opCount, nDesc, (void*)comm,
       comm->nRanks, (void*)stream);
  return rmaSubmit(op);
}
NCCL_ALIAS(ncclResult_t, ncclWaitSignal, int, ncclWaitSignalDesc_t*, ncclComm_t, hipStream_t)
