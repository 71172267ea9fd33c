// group.cc — ncclGroupStart / ncclGroupEnd.
//
// Reference: src/include/group.h:81-155 (thread-local group depth), src/group.cc:766-887
// (ncclGroupEndInternal), :598-760 (groupLaunch), :35 (ncclAsyncLaunch of deferred inits).
// Semantics kept: group state is thread-local; calls inside a group are only recorded, and nothing
// is enqueued on any stream until the outermost ncclGroupEnd; communicator inits inside a group run
// concurrently at ncclGroupEnd (required when one thread creates several ranks). Kernel launches here
// never block on peers (all connections are made at init), so one thread may drive every device of
// the node even without a group — the group is still honoured for ordering and error reporting.
// ncclSend / ncclRecv (p2p.cc) are recorded beside the collectives; at the group end each communicator's p2p work is
// planned first (errors before anything launches) and launched after the group's collectives.
// A zero-copy ncclAlltoAll / ncclGather (sendbuff in a symmetric window) is recorded as a collective and
// launches in the collectives' section, in issue order.
// The one-sided operations (rma.cc) likewise: planned first, launched per communicator in issue order after that
// communicator's collectives and p2p launches.
#include <string.h>

#include <algorithm>
#include <functional>
#include <map>
#include <thread>
#include <vector>

#include "core.h"

namespace ncclamd {

struct GroupState {
  int depth = 0;
  ncclResult_t error = ncclSuccess;
  std::vector<CollInfo> colls;
  std::vector<P2pOp> p2ps;  // ncclSend / ncclRecv (p2p.cc), launched after the group's collectives
  std::vector<RmaOp> rmas;  // ncclPutSignal / ncclSignal / ncclWaitSignal (rma.cc), launched after those
  std::vector<std::function<ncclResult_t()>> inits;
};
static thread_local GroupState tGroup;

bool groupActive() { return tGroup.depth > 0; }

ncclResult_t groupStartInternal() {
  tGroup.depth++;
  return ncclSuccess;
}

ncclResult_t groupDeferColl(const CollInfo& info) {
  tGroup.colls.push_back(info);
  return ncclSuccess;
}

ncclResult_t groupDeferP2p(const P2pOp& op) {
  tGroup.p2ps.push_back(op);
  return ncclSuccess;
}

ncclResult_t groupDeferRma(const RmaOp& op) {
  tGroup.rmas.push_back(op);
  return ncclSuccess;
}

// A group's one-sided ops per communicator, in first-use order, each list in issue order
struct CommRma {
  ncclComm* comm;
  std::vector<RmaOp> ops;
  RmaPlan plan;
  std::vector<hipStream_t> streams;  // the distinct streams its ops name (a shared-GPU comm forks from / joins to each)
};
static std::vector<CommRma> rmaByComm(const std::vector<RmaOp>& rmas) {
  std::vector<CommRma> out;
  for (const RmaOp& op : rmas) {
    size_t k = 0;
    while (k < out.size() && out[k].comm != op.comm) k++;
    if (k == out.size()) out.push_back({op.comm, {}, {}, {}});
    out[k].ops.push_back(op);
    if (std::find(out[k].streams.begin(), out[k].streams.end(), op.stream) == out[k].streams.end())
      out[k].streams.push_back(op.stream);
  }
  return out;
}
static CollInfo rmaAt(const CommRma& c, hipStream_t stream) {
  return {FUNC_ALLGATHER, "PutSignal", nullptr, nullptr, 0, ncclInt8, ncclSum, 0, c.comm, stream};
}

// A group's p2p ops per communicator, in first-use order, each list in issue order; `stream` = the first op's, on
// which the communicator's p2p work launches (the others are joined to it by events, p2pStreamJoin).
struct CommP2p {
  ncclComm* comm;
  hipStream_t stream;
  std::vector<P2pOp> ops;
  P2pPlan plan;
};
static std::vector<CommP2p> p2pByComm(const std::vector<P2pOp>& p2ps) {
  std::vector<CommP2p> out;
  for (const P2pOp& op : p2ps) {
    size_t k = 0;
    while (k < out.size() && out[k].comm != op.comm) k++;
    if (k == out.size()) out.push_back({op.comm, op.stream, {}, {}});
    out[k].ops.push_back(op);
  }
  return out;
}
// `to` waits for everything enqueued on `from` so far (capture-safe: an event record and a wait)
static ncclResult_t p2pStreamJoin(hipStream_t from, hipStream_t to) {
  hipEvent_t ev;
  HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, from);
  if (e == hipSuccess) e = hipStreamWaitEvent(to, ev, 0);
  (void)hipEventDestroy(ev);  // released once the record completes
  HIPCHECK(e);
  return ncclSuccess;
}
// fork (before = true): the launch stream waits for the group's other p2p streams of this comm; join: they wait for it
static ncclResult_t p2pOtherStreams(const CommP2p& c, bool before) {
  std::vector<hipStream_t> seen;
  for (const P2pOp& op : c.ops) {
    if (op.stream == c.stream || std::find(seen.begin(), seen.end(), op.stream) != seen.end()) continue;
    seen.push_back(op.stream);
    NCCLCHECK(before ? p2pStreamJoin(op.stream, c.stream) : p2pStreamJoin(c.stream, op.stream));
  }
  return ncclSuccess;
}

ncclResult_t groupDeferInit(std::function<ncclResult_t()> job) {
  tGroup.inits.push_back(std::move(job));
  return ncclSuccess;
}

void groupRecordError(ncclResult_t r) {
  if (tGroup.depth > 0 && tGroup.error == ncclSuccess && r != ncclSuccess) tGroup.error = r;
}

// Model time of one planned op (ncclGroupSimulateEnd): which kernel it planned onto and its tuner-sized bytes.
static ModelCost planCost(const PlannedColl& pc) {
  const ncclComm* comm = pc.info.comm;
  const int n = comm->nRanks;
  size_t bytes = pc.info.count * (size_t)typeSize(pc.info.datatype);
  if (pc.info.func == FUNC_REDUCESCATTER || pc.info.func == FUNC_ALLGATHER) bytes *= (size_t)n;
  // zero-copy AlltoAll / Gather: the symmetric model on the bytes a rank pulls — n blocks in the model's terms, which
  // prices (n-1)/n of them on the links, i.e. (n-1) B (a Gather: its root's share, the launch's longest)
  if (pc.info.func == FUNC_SYM_ALLTOALL || pc.info.func == FUNC_SYM_GATHER) bytes *= (size_t)n;
  ModelAlgo a = MODEL_DIRECT;
  if (pc.kind == PLAN_SYM) a = MODEL_SYM;
  else switch (pc.p.algo) {
    case ALGO_COPY:
    case ALGO_ONERANK: a = MODEL_COPY; break;
    case ALGO_LL: a = pc.p.ll.ops[0].proto == LLP_LL64 ? MODEL_LL128 : MODEL_LL; break;
    case ALGO_ONESHOT: a = MODEL_ONESHOT; break;
    case ALGO_PIPE:
      a = pc.p.pipeKind == PIPE_CHAIN_AR || pc.p.pipeKind == PIPE_CHAIN_REDUCE ? MODEL_CHAIN : MODEL_RING;
      break;
    default: a = MODEL_DIRECT; break;
  }
  return modelCost(a, pc.info.func, n, bytes);
}

// ncclGroupSimulateEnd (reference group.cc:116-123, :766-866 with simInfo): the group's collectives are
// planned exactly as ncclGroupEnd would plan them (same batches) and dropped instead of launched; deferred
// communicator inits still run. estimatedTime = the cost model's µs for the group: per communicator, one
// latency per launch plus every op's transfer time, and the slowest communicator (they run concurrently on
// their own GPUs). The reference reports the model time of the last op it planned; for a one-op group the
// two agree.
static ncclResult_t groupSimulate(std::vector<CollInfo>& colls, const std::vector<P2pOp>& p2ps,
                                  const std::vector<RmaOp>& rmas, float* estimatedUs) {
  std::map<ncclComm*, double> perComm;
  std::map<ncclComm*, std::vector<PlannedColl>> open;
  auto flush = [&](ncclComm* c) {
    std::vector<PlannedColl>& run = open[c];
    if (run.empty()) return;
    double t = 0;
    for (size_t k = 0; k < run.size(); k++) {
      if (run[k].kind == PLAN_NONE) continue;
      ModelCost m = planCost(run[k]);
      t += (k == 0 ? m.latUs : 0.0) + m.xferUs;
    }
    perComm[c] += t;
    run.clear();
  };
  for (size_t i = 0; i < colls.size(); i++) {
    PlannedColl pc;
    pc.info = colls[i];
    const uint64_t opCount = pc.info.comm->opCount;  // nothing is launched: keep the op counter as it was
    tPlanOnly = true;  // and nothing is registered (eager registration, register.cc)
    const ncclResult_t r = planColl(pc.info, pc.p, pc.sp, &pc.kind);
    tPlanOnly = false;
    NCCLCHECK(r);
    pc.info.comm->opCount = opCount;
    std::vector<PlannedColl>& run = open[pc.info.comm];
    if (!batchable(run, pc)) flush(pc.info.comm);
    run.push_back(pc);
  }
  for (auto& kv : open) flush(kv.first);
  // p2p work: planned as the group end would and dropped; one link's worth of the largest per-peer byte total (the
  // links of different peers run side by side), priced as a two-rank direct transfer of those bytes, plus a launch
  // latency per launch. The tuner plugin is not consulted (the reference does not consult it for p2p either).
  for (CommP2p& c : p2pByComm(p2ps)) {
    NCCLCHECK(p2pPlan(c.comm, c.ops, &c.plan));
    const ModelCost m = modelCost(MODEL_DIRECT, FUNC_ALLGATHER, 2, 2 * c.plan.maxPeerBytes);
    perComm[c.comm] += m.latUs * (double)std::max<size_t>(1, c.plan.launches.size()) + m.xferUs;
  }
  // one-sided work: planned and dropped the same way, priced with the p2p model (one link's worth of the largest
  // per-peer byte total, a launch latency per launch, waits included); no tuner, no NCCL_ALGO / NCCL_PROTO
  for (CommRma& c : rmaByComm(rmas)) {
    NCCLCHECK(rmaPlan(c.comm, c.ops, &c.plan));
    const ModelCost m = modelCost(MODEL_DIRECT, FUNC_ALLGATHER, 2, 2 * c.plan.maxPeerBytes);
    perComm[c.comm] += m.latUs * (double)std::max<size_t>(1, c.plan.steps.size()) + m.xferUs;
  }
  double worst = 0;
  for (auto& kv : perComm) worst = kv.second > worst ? kv.second : worst;
  *estimatedUs = (float)worst;
  return ncclSuccess;
}

ncclResult_t groupEndInternal(ncclSimInfo_t* simInfo) {
  if (tGroup.depth == 0) {
    WARN("ncclGroupEnd: not in a group call.");
    return ncclInvalidUsage;
  }
  ncclSimInfo_t sim;
  size_t simSize = 0;
  if (simInfo) {  // reference group.cc:792-800: copy what the caller's (possibly older) struct holds
    memcpy(&simSize, &simInfo->size, sizeof(size_t));
    if (simSize > sizeof(ncclSimInfo_t)) simSize = sizeof(ncclSimInfo_t);
    sim = NCCL_SIM_INFO_INITIALIZER;
    memcpy(&sim, simInfo, simSize);
  }
  if (--tGroup.depth > 0) return ncclSuccess;
  ncclResult_t ret = tGroup.error;
  std::vector<CollInfo> colls;
  std::vector<P2pOp> p2pOps;
  std::vector<RmaOp> rmaOps;
  std::vector<std::function<ncclResult_t()>> inits;
  p2pOps.swap(tGroup.p2ps);
  rmaOps.swap(tGroup.rmas);
  colls.swap(tGroup.colls);
  inits.swap(tGroup.inits);
  tGroup.error = ncclSuccess;
  if (ret != ncclSuccess) return ret;  // a call inside the group failed its checks: launch nothing
  if (simInfo && sim.magic != 0x74685283) {
    WARN("ncclSimInfo_t argument not initialized via NCCL_SIM_INFO_INITIALIZER");
    return ncclInvalidArgument;
  }

  if (!inits.empty()) {
    std::vector<ncclResult_t> rs(inits.size(), ncclSuccess);
    std::vector<std::thread> ts;
    int dev = 0;
    (void)hipGetDevice(&dev);
    for (size_t i = 0; i < inits.size(); i++) ts.emplace_back([&, i]() { rs[i] = inits[i](); });
    for (auto& t : ts) t.join();
    (void)hipSetDevice(dev);
    for (auto r : rs)
      if (r != ncclSuccess) return r;
  }
  if (simInfo) {
    float us = 0;
    NCCLCHECK(groupSimulate(colls, p2pOps, rmaOps, &us));
    sim.estimatedTime = us;
    memcpy(simInfo, &sim, simSize);
    return ncclSuccess;
  }
  // the group's p2p work is planned per communicator before anything launches: a send to self without its recv
  // (ncclInvalidUsage) or a round that fits no launch fails the group with nothing enqueued
  std::vector<CommP2p> p2p = p2pByComm(p2pOps);
  for (CommP2p& c : p2p) NCCLCHECK(p2pPlan(c.comm, c.ops, &c.plan));
  std::vector<CommRma> rma = rmaByComm(rmaOps);  // ... and the one-sided work: every planning failure surfaces here
  for (CommRma& c : rma) NCCLCHECK(rmaPlan(c.comm, c.ops, &c.plan));
  int dev = 0;
  (void)hipGetDevice(&dev);
  // each communicator's upkeep first, before any of the group's kernels is launched (enqueue.cc collProgress; not
  // while any of its streams in this group is being captured)
  for (size_t i = 0; i < colls.size(); i++) {
    bool seen = false;
    for (size_t j = 0; j < i && !seen; j++) seen = colls[j].comm == colls[i].comm;
    if (seen) continue;
    bool capturing = false;
    for (size_t j = i; j < colls.size() && !capturing; j++) {
      if (colls[j].comm != colls[i].comm) continue;
      hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
      capturing = hipStreamIsCapturing(colls[j].stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone;
      (void)hipGetLastError();
    }
    if (capturing) continue;
    (void)hipSetDevice(colls[i].comm->device);
    collProgress(colls[i].comm, colls[i].stream);
  }
  for (const CommP2p& c : p2p) {  // ... also of the communicators that only send and receive in this group
    bool skip = false;
    for (size_t j = 0; j < colls.size() && !skip; j++) skip = colls[j].comm == c.comm;
    for (size_t j = 0; j < c.ops.size() && !skip; j++) {
      hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
      skip = hipStreamIsCapturing(c.ops[j].stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone;
      (void)hipGetLastError();
    }
    if (skip) continue;
    (void)hipSetDevice(c.comm->device);
    collProgress(c.comm, c.stream);
  }
  for (const CommRma& c : rma) {  // ... or only put, signal and wait
    bool skip = false;
    for (size_t j = 0; j < colls.size() && !skip; j++) skip = colls[j].comm == c.comm;
    for (size_t j = 0; j < p2p.size() && !skip; j++) skip = p2p[j].comm == c.comm;
    for (size_t j = 0; j < c.streams.size() && !skip; j++) {
      hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
      skip = hipStreamIsCapturing(c.streams[j], &st) != hipSuccess || st != hipStreamCaptureStatusNone;
      (void)hipGetLastError();
    }
    if (skip) continue;
    (void)hipSetDevice(c.comm->device);
    collProgress(c.comm, c.streams[0]);
  }
  ncclResult_t r = ncclSuccess;
  for (size_t i = 0; i < colls.size() && r == ncclSuccess; i++) r = collFork(colls[i]);
  for (size_t i = 0; i < p2p.size() && r == ncclSuccess; i++) {
    (void)hipSetDevice(p2p[i].comm->device);
    r = p2pOtherStreams(p2p[i], true);
    const CollInfo at = {FUNC_ALLGATHER, "SendRecv", nullptr, nullptr, 0, ncclInt8, ncclSum, 0, p2p[i].comm, p2p[i].stream};
    if (r == ncclSuccess) r = collFork(at);
  }
  for (size_t i = 0; i < rma.size() && r == ncclSuccess; i++)
    for (size_t j = 0; j < rma[i].streams.size() && r == ncclSuccess; j++) r = collFork(rmaAt(rma[i], rma[i].streams[j]));
  // launches in group order per comm; consecutive ops that planned onto the same kernel with the same stream,
  // type and operator become one launch (enqueue.cc batchable / launchBatch). Every rank of a comm issues the
  // same op sequence, so every rank forms the same batches.
  std::map<ncclComm*, std::vector<PlannedColl>> open;
  auto flush = [&](ncclComm* c) -> ncclResult_t {
    std::vector<PlannedColl>& run = open[c];
    ncclResult_t res = run.empty() ? ncclSuccess : launchBatch(run);
    run.clear();
    return res;
  };
  for (size_t i = 0; i < colls.size() && r == ncclSuccess; i++) {
    PlannedColl pc;
    pc.info = colls[i];
    (void)hipSetDevice(pc.info.comm->device);
    r = planColl(pc.info, pc.p, pc.sp, &pc.kind);
    if (r != ncclSuccess) break;
    std::vector<PlannedColl>& run = open[pc.info.comm];
    if (!batchable(run, pc)) r = flush(pc.info.comm);
    if (r == ncclSuccess) run.push_back(pc);
  }
  for (auto& kv : open)
    if (r == ncclSuccess) r = flush(kv.first);
  // then each communicator's p2p work: after its collectives on every rank, because both kinds advance the same
  // per-pair sequences
  for (size_t i = 0; i < p2p.size() && r == ncclSuccess; i++) {
    ncclComm* c = p2p[i].comm;
    (void)hipSetDevice(c->device);
    r = p2pLaunchPlan(c, p2p[i].plan, c->sharedDevInProcess ? c->internalStream : p2p[i].stream);
  }
  // then its one-sided work, in issue order: its signals follow everything the communicator does in this group
  for (size_t i = 0; i < rma.size() && r == ncclSuccess; i++) {
    (void)hipSetDevice(rma[i].comm->device);
    r = rmaLaunchPlan(rma[i].comm, rma[i].plan);
  }
  for (size_t i = 0; i < colls.size() && r == ncclSuccess; i++) r = collJoin(colls[i]);
  for (size_t i = 0; i < p2p.size() && r == ncclSuccess; i++) {
    (void)hipSetDevice(p2p[i].comm->device);
    const CollInfo at = {FUNC_ALLGATHER, "SendRecv", nullptr, nullptr, 0, ncclInt8, ncclSum, 0, p2p[i].comm, p2p[i].stream};
    r = collJoin(at);
    if (r == ncclSuccess) r = p2pOtherStreams(p2p[i], false);
  }
  for (size_t i = 0; i < rma.size() && r == ncclSuccess; i++)
    for (size_t j = 0; j < rma[i].streams.size() && r == ncclSuccess; j++) r = collJoin(rmaAt(rma[i], rma[i].streams[j]));
  (void)hipSetDevice(dev);
  return r;
}

}  // namespace ncclamd

using namespace ncclamd;

NCCL_EXPORT ncclResult_t ncclGroupStart() {
  ROCTX_RANGE("ncclGroupStart");
  return groupStartInternal();
}
extern "C" __attribute__((visibility("default"), alias("ncclGroupStart"))) ncclResult_t pncclGroupStart();

NCCL_EXPORT ncclResult_t ncclGroupEnd() {
  ROCTX_RANGE("ncclGroupEnd");
  return groupEndInternal(nullptr);
}
extern "C" __attribute__((visibility("default"), alias("ncclGroupEnd"))) ncclResult_t pncclGroupEnd();

NCCL_EXPORT ncclResult_t ncclGroupSimulateEnd(ncclSimInfo_t* simInfo) { return groupEndInternal(simInfo); }
extern "C" __attribute__((visibility("default"), alias("ncclGroupSimulateEnd"))) ncclResult_t
pncclGroupSimulateEnd(ncclSimInfo_t*);
