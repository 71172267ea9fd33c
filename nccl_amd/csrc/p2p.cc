// p2p.cc — ncclSend / ncclRecv and the three collectives the reference builds from them (ncclAlltoAll, ncclGather,
// ncclScatter): entry points, argument checks, the per-group host plan and its launches.
//
// Reference: src/collectives.cc:154-310 (entry points), src/enqueue.cc:3070-3109 (AlltoAll / Gather / Scatter expand
// into sends and recvs at enqueue time), :1158-1166 (a self send needs its recv in the same group), src/group.cc
// (nothing launches before the outermost ncclGroupEnd; an ungrouped call is a group of one).
//
// The plan: per ordered pair and direction, the group's messages form a stream; a message's channel
// count and part size come from its byte count and per-communicator constants alone (device_abi.h p2pCut), so the
// sender and the receiver cut it alike whatever else either does in its group. Part j of every stream runs on
// physical channel j: staging, flags and counters are indexed by (channel, kind, peer), so streams of different peers
// share no word. A launch holds at most chanCap co-resident workgroups; when a group needs more, launches hold
// contiguous runs of the reference's rounds (round r: send to rank + r, recv from rank - r), a round's two streams
// never apart. The unfinished stream of the smallest round anywhere then has every earlier launch of both its ranks
// complete, so both its workgroups are resident: no deadlock, however each rank packs its rounds.
//
// ncclAlltoAll / ncclGather whose sendbuff lies in a symmetric window do not expand: they are planned and launched as
// one collective on the zero-copy kernel (symA2ASubmit below, enqueue.cc planSymA2A).
#include <string.h>

#include <algorithm>

#include "core.h"

namespace ncclamd {

// channels per peer and direction: the knob, the channels allocated, and half the co-resident cap (a round's send and
// recv streams share a launch)
static int p2pMaxChannels(const ncclComm* comm) {
  return std::min(comm->tune.p2pMaxCh, std::min(comm->maxChannels, comm->chanCap / 2));
}

P2pCut p2pCutFor(const ncclComm* comm, size_t bytes) {
  const int mx = std::max(1, p2pMaxChannels(comm));
  return p2pCut(bytes, (uint64_t)comm->tune.p2pChunkBytes, std::min(comm->tune.p2pMinCh, mx), mx);
}

ncclResult_t p2pPlan(ncclComm* comm, const std::vector<P2pOp>& ops, P2pPlan* plan) {
  const int n = comm->nRanks, me = comm->rank;
  plan->self.clear();
  plan->launches.clear();
  plan->maxPeerBytes = 0;
  std::vector<P2pMsg> sendTo[NCCL_AMD_MAX_RANKS], recvFrom[NCCL_AMD_MAX_RANKS];
  bool remote = false;
  for (const P2pOp& op : ops) {
    if (op.peer < 0 || op.peer >= n) return ncclInternalError;  // (checked at the entry point)
    if (op.bytes == 0) continue;  // both sides know: counts match. No handshake, no place in the order
    const P2pCut cut = p2pCutFor(comm, op.bytes);
    (op.recv ? recvFrom : sendTo)[op.peer].push_back({(uint64_t)(uintptr_t)op.buff, (uint64_t)op.bytes, cut.part, (uint32_t)cut.nch, 0});
    remote = remote || op.peer != me;
  }
  // round 0: self sends and recvs pair up in issue order (reference enqueue.cc:1158-1166)
  if (sendTo[me].size() != recvFrom[me].size()) {
    WARN("ncclGroupEnd: rank %d has %zu sends to itself and %zu recvs from itself in one group; a send to self needs "
         "its recv in the same group", me, sendTo[me].size(), recvFrom[me].size());
    return ncclInvalidUsage;
  }
  for (size_t k = 0; k < sendTo[me].size(); k++) {
    if (sendTo[me][k].bytes != recvFrom[me][k].bytes) {
      WARN("ncclGroupEnd: rank %d sends %lu bytes to itself and receives %lu", me, (unsigned long)sendTo[me][k].bytes,
           (unsigned long)recvFrom[me][k].bytes);
      return ncclInvalidUsage;
    }
    plan->self.push_back({(void*)(uintptr_t)recvFrom[me][k].ptr, (const void*)(uintptr_t)sendTo[me][k].ptr, (size_t)sendTo[me][k].bytes});
  }
  if (!remote) return ncclSuccess;
  const int budget = comm->chanCap;
  if (p2pMaxChannels(comm) < 1) {
    WARN("ncclSend / ncclRecv need two co-resident workgroups (one channel for each direction of a round); this "
         "communicator launches at most %d (NCCL_MAX_CTAS, ranks per GPU)", budget);
    return ncclInvalidUsage;
  }
  P2pLaunch cur;
  cur.grid = 0;
  cur.firstRound = cur.lastRound = 0;
  auto close = [&]() {
    if (cur.grid > 0) plan->launches.push_back(cur);
    cur.grid = 0;
    cur.streams.clear();
    cur.msgs.clear();
  };
  for (int r = 1; r < n; r++) {
    const int peers[2] = {(me + r) % n, (me - r + n) % n};
    const std::vector<P2pMsg>* lists[2] = {&sendTo[peers[0]], &recvFrom[peers[1]]};
    int nch[2] = {0, 0};
    size_t bytes[2] = {0, 0};
    for (int d = 0; d < 2; d++)
      for (const P2pMsg& m : *lists[d]) {
        nch[d] = std::max(nch[d], (int)m.nch);
        bytes[d] += m.bytes;
      }
    plan->maxPeerBytes = std::max(plan->maxPeerBytes, std::max(bytes[0], bytes[1]));
    const int need = nch[0] + nch[1];
    const size_t needMsgs = lists[0]->size() + lists[1]->size();
    if (need == 0) continue;
    if (need > budget || needMsgs > (size_t)kP2pMaxMsgs) {
      WARN("ncclGroupEnd: round %d of rank %d (send to %d, recv from %d) needs %d workgroups and %zu message descriptors "
           "in one launch; at most %d and %d fit", r, me, peers[0], peers[1], need, needMsgs, budget, kP2pMaxMsgs);
      return ncclInvalidUsage;
    }
    if (cur.grid + need > budget || cur.msgs.size() + needMsgs > (size_t)kP2pMaxMsgs ||
        cur.streams.size() + 2 > (size_t)kP2pMaxStreams)
      close();
    if (cur.grid == 0) cur.firstRound = r;
    cur.lastRound = r;
    for (int d = 0; d < 2; d++) {
      if (nch[d] == 0) continue;
      P2pStream s;
      memset(&s, 0, sizeof(s));
      s.wgOff = (uint16_t)cur.grid;
      s.nch = (uint16_t)nch[d];
      s.msgOff = (uint16_t)cur.msgs.size();
      s.nMsgs = (uint16_t)lists[d]->size();
      s.peer = (uint8_t)peers[d];
      s.recv = (uint8_t)d;
      cur.streams.push_back(s);
      cur.msgs.insert(cur.msgs.end(), lists[d]->begin(), lists[d]->end());
      cur.grid += nch[d];
    }
  }
  close();
  return ncclSuccess;
}

// Host-side guard before a p2pKernel launches (enqueue.cc checkGrid's rule): the grid within the co-resident cap,
// every channel index within the channels the staging slab, flag block and counters were allocated for, the
// workgroup ranges and message ranges of the streams exactly the launch's.
static ncclResult_t p2pCheckGrid(const ncclComm* comm, const P2pLaunch& l) {
  bool good = l.grid >= 1 && l.grid <= comm->chanCap && !l.streams.empty() && l.streams.size() <= (size_t)kP2pMaxStreams &&
              l.msgs.size() <= (size_t)kP2pMaxMsgs;
  int off = 0;
  size_t moff = 0;
  for (size_t i = 0; good && i < l.streams.size(); i++) {
    const P2pStream& s = l.streams[i];
    good = s.wgOff == off && s.nch >= 1 && s.nch <= comm->maxChannels && s.msgOff == moff && s.peer < comm->nRanks &&
           s.peer != comm->rank;
    for (size_t k = 0; good && k < s.nMsgs; k++) good = moff + k < l.msgs.size() && l.msgs[moff + k].nch <= s.nch;
    off += s.nch;
    moff += s.nMsgs;
  }
  if (good && off == l.grid && moff == l.msgs.size()) return ncclSuccess;
  WARN("internal: a p2p launch of %d workgroups (cap %d, %d channels allocated) was refused before launch", l.grid,
       comm->chanCap, comm->maxChannels);
  return ncclInternalError;
}

ncclResult_t p2pLaunchPlan(ncclComm* comm, const P2pPlan& plan, hipStream_t stream) {
  for (const P2pLaunch& l : plan.launches) NCCLCHECK(p2pCheckGrid(comm, l));
  for (const P2pSelfCopy& c : plan.self)
    if (c.dst != c.src) HIPCHECK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, stream));
  for (const P2pLaunch& l : plan.launches) {
    TRACE("p2p launch: rank %d rounds %d..%d, %zu streams, %zu messages, %d workgroups", comm->rank, l.firstRound,
          l.lastRound, l.streams.size(), l.msgs.size(), l.grid);
    NCCLCHECK(launchP2pKernel(comm, l, stream));
  }
  if (comm->fdServer && !plan.launches.empty()) {  // (enqueue.cc noteLaunch)
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) == hipSuccess && st == hipStreamCaptureStatusNone) ipcNoteLaunch(stream, comm->device);
    else (void)hipGetLastError();
  }
  return ncclSuccess;
}

// The checks every p2p entry point shares (enqueue.cc enqueueCheck's, without a reduction operator): the comm first,
// also for count == 0, as ncclAllReduce does; then the datatype and the communicator's error state.
static ncclResult_t p2pCheck(const char* opName, ncclComm* comm, ncclDataType_t datatype, int* ts) {
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
  if (ret != ncclSuccess) groupRecordError(ret);
  else *ts = typeSize(datatype);
  return ret;
}

static ncclResult_t p2pFail(ncclResult_t r) {
  groupRecordError(r);
  return r;
}

static ncclResult_t rankCheck(const char* opName, const char* what, int r, const ncclComm* comm) {
  if (r >= 0 && r < comm->nRanks) return ncclSuccess;
  WARN("%s : invalid %s %d (%s should be in the 0..%d range)", opName, what, r, what, comm->nRanks);
  return p2pFail(ncclInvalidArgument);
}

static ncclResult_t bufCheck(const char* opName, const char* name, const void* p, size_t count, ncclComm* comm) {
  if (!comm->tune.checkPointers || count == 0) return ncclSuccess;
  const ncclResult_t r = ptrCheck(p, comm, name, opName);
  return r == ncclSuccess ? r : p2pFail(r);
}

// Record the ops: inside a group as they are, outside as a group of their own (launched before the call returns).
static ncclResult_t p2pSubmit(const P2pOp* ops, size_t nOps) {
  const bool own = !groupActive();
  if (own) groupStartInternal();
  for (size_t i = 0; i < nOps; i++) groupDeferP2p(ops[i]);
  return own ? groupEndInternal() : ncclSuccess;
}

// AlltoAll / Gather with the sendbuff in a symmetric window (enqueue.cc symA2AEligible): one collective on the zero-copy
// kernel instead of the send / recv expansion. Inside a group it is deferred with the group's
// collectives and launches in their section, in issue order; outside it launches before the call returns.
static ncclResult_t symA2ASubmit(const CollInfo& info) {
  if (groupActive()) return groupDeferColl(info);
  DeviceRestore restore;
  return launchColl(info);
}

static ncclResult_t sendRecv(const char* opName, bool recv, void* buff, size_t count, ncclDataType_t datatype, int peer,
                             ncclComm* comm, hipStream_t stream) {
  ROCTX_RANGE("nccl%s comm=%p count=%zu datatype=%d peer=%d", opName, (void*)comm, count, (int)datatype, peer);
  int ts = 0;
  NCCLCHECK(p2pCheck(opName, comm, datatype, &ts));
  NCCLCHECK(rankCheck(opName, "peer", peer, comm));
  NCCLCHECK(bufCheck(opName, recv ? "recvbuff" : "sendbuff", buff, count, comm));
  INFO("%s: opCount %lx buff %p count %zu datatype %d peer %d comm %p [nranks=%d] stream %p", opName,
       (unsigned long)comm->opCount, buff, count, (int)datatype, peer, (void*)comm, comm->nRanks, (void*)stream);
  const P2pOp op = {comm, stream, buff, count * (size_t)ts, peer, recv};
  return p2pSubmit(&op, 1);
}

}  // namespace ncclamd

using namespace ncclamd;

#define NCCL_ALIAS(ret, name, ...) extern "C" __attribute__((visibility("default"), alias(#name))) ret p##name(__VA_ARGS__);

NCCL_EXPORT ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                                  hipStream_t stream) {
  return sendRecv("Send", false, (void*)sendbuff, count, datatype, peer, comm, stream);
}
NCCL_ALIAS(ncclResult_t, ncclSend, const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)

NCCL_EXPORT ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                                  hipStream_t stream) {
  return sendRecv("Recv", true, recvbuff, count, datatype, peer, comm, stream);
}
NCCL_ALIAS(ncclResult_t, ncclRecv, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)

// AlltoAll (reference enqueue.cc:3070-3083): a send and a recv of `count` elements to and from every rank r, self
// included, at offset r * count.
NCCL_EXPORT ncclResult_t ncclAlltoAll(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                                      ncclComm_t comm, hipStream_t stream) {
  ROCTX_RANGE("ncclAlltoAll comm=%p count=%zu datatype=%d", (void*)comm, count, (int)datatype);
  int ts = 0;
  NCCLCHECK(p2pCheck("AlltoAll", comm, datatype, &ts));
  NCCLCHECK(bufCheck("AlltoAll", "sendbuff", sendbuff, count, comm));
  NCCLCHECK(bufCheck("AlltoAll", "recvbuff", recvbuff, count, comm));
  INFO("AlltoAll: opCount %lx sendbuff %p recvbuff %p count %zu datatype %d comm %p [nranks=%d] stream %p",
       (unsigned long)comm->opCount, sendbuff, recvbuff, count, (int)datatype, (void*)comm, comm->nRanks, (void*)stream);
  const size_t bytes = count * (size_t)ts;
  if (symA2AEligible(comm, sendbuff, (size_t)comm->nRanks * bytes, count))
    return symA2ASubmit({FUNC_SYM_ALLTOALL, "AlltoAll", sendbuff, recvbuff, count, datatype, ncclSum, 0, comm, stream});
  std::vector<P2pOp> ops;
  for (int r = 0; r < comm->nRanks; r++) {
    ops.push_back({comm, stream, (char*)sendbuff + (size_t)r * bytes, bytes, r, false});
    ops.push_back({comm, stream, (char*)recvbuff + (size_t)r * bytes, bytes, r, true});
  }
  return p2pSubmit(ops.data(), ops.size());
}
NCCL_ALIAS(ncclResult_t, ncclAlltoAll, const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t)

// Gather (reference enqueue.cc:3084-3096): every rank sends to the root, which receives block r from rank r;
// recvbuff is read on the root only.
NCCL_EXPORT ncclResult_t ncclGather(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root,
                                    ncclComm_t comm, hipStream_t stream) {
  ROCTX_RANGE("ncclGather comm=%p count=%zu datatype=%d root=%d", (void*)comm, count, (int)datatype, root);
  int ts = 0;
  NCCLCHECK(p2pCheck("Gather", comm, datatype, &ts));
  NCCLCHECK(rankCheck("Gather", "root", root, comm));
  NCCLCHECK(bufCheck("Gather", "sendbuff", sendbuff, count, comm));
  if (comm->rank == root) NCCLCHECK(bufCheck("Gather", "recvbuff", recvbuff, count, comm));
  INFO("Gather: opCount %lx sendbuff %p recvbuff %p count %zu datatype %d root %d comm %p [nranks=%d] stream %p",
       (unsigned long)comm->opCount, sendbuff, recvbuff, count, (int)datatype, root, (void*)comm, comm->nRanks, (void*)stream);
  const size_t bytes = count * (size_t)ts;
  if (symA2AEligible(comm, sendbuff, bytes, count))
    return symA2ASubmit({FUNC_SYM_GATHER, "Gather", sendbuff, recvbuff, count, datatype, ncclSum, root, comm, stream});
  std::vector<P2pOp> ops;
  ops.push_back({comm, stream, (void*)sendbuff, bytes, root, false});
  if (comm->rank == root)
    for (int r = 0; r < comm->nRanks; r++) ops.push_back({comm, stream, (char*)recvbuff + (size_t)r * bytes, bytes, r, true});
  return p2pSubmit(ops.data(), ops.size());
}
NCCL_ALIAS(ncclResult_t, ncclGather, const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)

// Scatter (reference enqueue.cc:3097-3109): the root sends block r to rank r, every rank receives one; sendbuff is
// read on the root only.
NCCL_EXPORT ncclResult_t ncclScatter(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root,
                                     ncclComm_t comm, hipStream_t stream) {
  ROCTX_RANGE("ncclScatter comm=%p count=%zu datatype=%d root=%d", (void*)comm, count, (int)datatype, root);
  int ts = 0;
  NCCLCHECK(p2pCheck("Scatter", comm, datatype, &ts));
  NCCLCHECK(rankCheck("Scatter", "root", root, comm));
  if (comm->rank == root) NCCLCHECK(bufCheck("Scatter", "sendbuff", sendbuff, count, comm));
  NCCLCHECK(bufCheck("Scatter", "recvbuff", recvbuff, count, comm));
  INFO("Scatter: opCount %lx sendbuff %p recvbuff %p count %zu datatype %d root %d comm %p [nranks=%d] stream %p",
       (unsigned long)comm->opCount, sendbuff, recvbuff, count, (int)datatype, root, (void*)comm, comm->nRanks, (void*)stream);
  const size_t bytes = count * (size_t)ts;
  std::vector<P2pOp> ops;
  if (comm->rank == root)
    for (int r = 0; r < comm->nRanks; r++) ops.push_back({comm, stream, (char*)sendbuff + (size_t)r * bytes, bytes, r, false});
  ops.push_back({comm, stream, recvbuff, bytes, root, true});
  return p2pSubmit(ops.data(), ops.size());
}
NCCL_ALIAS(ncclResult_t, ncclScatter, const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)
