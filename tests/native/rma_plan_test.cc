// rma_plan_test.cc — CPU test driver of the ncclPutSignal / ncclSignal / ncclWaitSignal host side: the entry points'
// argument checks (rma.cc), the batch plan and the group order (rma.cc rmaPlan, group.cc). Compiled with rma.cc,
// group.cc, p2p.cc, enqueue.cc and debug.cc like p2p_plan_test (no GPU: the kernel launches are recorded instead of
// run, the few HIP calls are stubbed), so what it inspects is exactly what the library would launch.
//
//   rma_plan_test args     one line "<call>=<ncclResult_t> launches=<n>" per row of the argument table
//   rma_plan_test batch    the batching rules; prints "OK checks=<n>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "plan_stubs.h"

namespace ncclamd {
struct Recorded {  // one launch, in launch order
  bool wait;
  hipStream_t stream;
  RmaLaunch put;
  RmaWaitArgs w;
};
static std::vector<Recorded> gRec;
ncclResult_t launchRmaPutKernel(const ncclComm*, const RmaLaunch& l, hipStream_t s) {
  gRec.push_back({false, s, l, {}});
  return ncclSuccess;
}
ncclResult_t launchRmaWaitKernel(const ncclComm*, const RmaWaitArgs& w, hipStream_t s) {
  gRec.push_back({true, s, {}, w});
  return ncclSuccess;
}
ncclResult_t launchP2pKernel(const ncclComm*, const P2pLaunch&, hipStream_t) { return ncclInternalError; }
ModelCost modelCost(ModelAlgo, CollFunc, int, size_t bytes) { return {1.0, (double)bytes * 1e-4}; }
thread_local bool tPlanOnly = false;
}  // namespace ncclamd

using namespace ncclamd;

static const uintptr_t kSrcBase = 0x10000000, kSrcSize = 0x4000000;  // this rank's symmetric source window
static const uintptr_t kDstBase = 0x40000000;                        // peer r's target at kDstBase + r * 0x1000000

struct Fixture {
  ncclComm comm;
  ncclWindow_vidmem src, dst;
  Fixture(int n, int rank, int chanCap) {
    // rma.cc launches no collective (a collective launch is an error); buffers count as registered
    gStubs.refuseLaunch = gStubs.refuseSymLaunch = gStubs.regLookupAlways = gStubs.regCoversAnswer = true;
    stubComm(comm, n, rank, 1 << 20, chanCap);
    memset(&src, 0, sizeof(src));
    memset(&dst, 0, sizeof(dst));
    src.comm = dst.comm = &comm;
    src.userPtr = (void*)kSrcBase;
    src.size = kSrcSize;
    src.flags = NCCL_WIN_COLL_SYMMETRIC;
    dst.userPtr = (void*)(kDstBase + (uintptr_t)rank * 0x1000000);
    dst.size = 1000 + 100 * (size_t)rank;
    dst.flags = 0;  // a window with another size on every rank: not symmetric
    for (int r = 0; r < n; r++) {
      src.peerPtr[r] = (char*)kSrcBase;  // (never a target here)
      src.peerSize[r] = kSrcSize;
      dst.peerPtr[r] = (char*)(kDstBase + (uintptr_t)r * 0x1000000);
      dst.peerSize[r] = (size_t)(1 << 24);
    }
    comm.windows = {&src, &dst};
  }
};

#define REQUIRE(cond, ...)          \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, "FAIL: ");    \
      fprintf(stderr, __VA_ARGS__); \
      fputc('\n', stderr);          \
      return false;                 \
    }                               \
    gChecks++;                      \
  } while (0)
static int gChecks = 0;

static ncclResult_t put(Fixture& f, size_t srcOff, size_t bytes, int peer, size_t dstOff, hipStream_t s = nullptr) {
  return ncclPutSignal((const void*)(kSrcBase + srcOff), bytes, ncclUint8, peer, &f.dst, dstOff, 0, 0, 0, &f.comm, s);
}

// invariants of every recorded put launch: within the cap and the argument block, streams contiguous and whole
static bool launchesSound(const Fixture& f) {
  for (const Recorded& r : gRec) {
    if (r.wait) {
      REQUIRE(r.w.n >= 1 && r.w.n <= f.comm.nRanks, "a wait of %d descriptors", r.w.n);
      continue;
    }
    REQUIRE(r.put.grid >= 1 && r.put.grid <= f.comm.chanCap, "a launch of %d workgroups (cap %d)", r.put.grid, f.comm.chanCap);
    REQUIRE(r.put.streams.size() <= (size_t)kRmaMaxStreams && r.put.msgs.size() <= (size_t)kRmaMaxMsgs, "argument block overflow");
    int off = 0;
    size_t moff = 0;
    for (const RmaStream& s : r.put.streams) {
      REQUIRE(s.wgOff == off && s.msgOff == moff && s.nch >= 1 && s.nMsgs >= 1, "stream layout");
      for (int k = 0; k < s.nMsgs; k++) REQUIRE(r.put.msgs[moff + k].nch <= s.nch, "a message wider than its stream");
      off += s.nch;
      moff += s.nMsgs;
    }
    REQUIRE(off == r.put.grid && moff == r.put.msgs.size(), "streams do not cover the launch");
  }
  return true;
}

// per peer, the source pointers of its messages in launch order; fails when a peer appears in two launches of one batch
static std::map<int, std::vector<uint64_t>> perPeer(size_t from, size_t to, bool* wholeStreams) {
  std::map<int, std::vector<uint64_t>> out;
  std::map<int, int> launchesOf;
  for (size_t i = from; i < to && i < gRec.size(); i++) {
    if (gRec[i].wait) continue;
    for (const RmaStream& s : gRec[i].put.streams) {
      launchesOf[s.peer]++;
      for (int k = 0; k < s.nMsgs; k++) out[s.peer].push_back(gRec[i].put.msgs[s.msgOff + k].src);
    }
  }
  *wholeStreams = true;
  for (auto& kv : launchesOf) *wholeStreams = *wholeStreams && kv.second == 1;
  return out;
}

static bool batchChecks() {
  bool whole = false;
  {  // puts to three peers in one group: one launch of three streams
    Fixture f(4, 1, 256);
    gRec.clear();
    ncclGroupStart();
    REQUIRE(put(f, 0, 100, 0, 0) == ncclSuccess && put(f, 256, 100, 2, 0) == ncclSuccess && put(f, 512, 100, 3, 0) == ncclSuccess, "puts refused");
    REQUIRE(gRec.empty(), "a put inside a group launched before the group end");
    REQUIRE(ncclGroupEnd() == ncclSuccess, "group end");
    REQUIRE(gRec.size() == 1 && !gRec[0].wait && gRec[0].put.streams.size() == 3 && gRec[0].put.grid == 3, "three peers: %zu launches", gRec.size());
    REQUIRE(gRec[0].put.msgs[0].dst == kDstBase && gRec[0].put.msgs[1].dst == kDstBase + 2 * 0x1000000, "targets");
    if (!launchesSound(f)) return false;
  }
  {  // a wait splits batches; the order is the issue order
    Fixture f(4, 1, 256);
    gRec.clear();
    ncclWaitSignalDesc_t d[3] = {{2, 0, 0, 0}, {1, 2, 0, 0}, {3, 0, 0, 0}};
    ncclGroupStart();
    put(f, 0, 100, 0, 0);
    put(f, 256, 100, 2, 0);
    REQUIRE(ncclWaitSignal(3, d, &f.comm, nullptr) == ncclSuccess, "wait refused");
    put(f, 512, 100, 0, 16);
    REQUIRE(ncclGroupEnd() == ncclSuccess, "group end");
    REQUIRE(gRec.size() == 3 && !gRec[0].wait && gRec[1].wait && !gRec[2].wait, "put, wait, put: %zu launches", gRec.size());
    REQUIRE(gRec[0].put.streams.size() == 2 && gRec[2].put.streams.size() == 1, "batches around the wait");
    // merged duplicate descriptors: peer 0 twice adds up, in rank order
    REQUIRE(gRec[1].w.n == 2 && gRec[1].w.d[0].peer == 0 && gRec[1].w.d[0].opCnt == 5 && gRec[1].w.d[1].peer == 2 && gRec[1].w.d[1].opCnt == 1,
            "merged descriptors: n %d, (%d, %u), (%d, %u)", gRec[1].w.n, gRec[1].w.d[0].peer, gRec[1].w.d[0].opCnt, gRec[1].w.d[1].peer, gRec[1].w.d[1].opCnt);
    if (!launchesSound(f)) return false;
  }
  {  // two puts to one peer: one stream, issue order, one workgroup set; count == 0 is a signal; ncclSignal moves nothing
    Fixture f(4, 1, 256);
    f.comm.tune.p2pChunkBytes = 4096;
    gRec.clear();
    ncclGroupStart();
    put(f, 0, 3 * 4096 + 1, 2, 0);
    put(f, 0x10000, 100, 2, 64);
    put(f, 0x20000, 0, 2, 7);
    REQUIRE(ncclSignal(2, 0, 0, 0, &f.comm, nullptr) == ncclSuccess, "signal refused");
    REQUIRE(ncclGroupEnd() == ncclSuccess, "group end");
    REQUIRE(gRec.size() == 1 && gRec[0].put.streams.size() == 1, "one peer: %zu launches", gRec.size());
    const RmaStream& s = gRec[0].put.streams[0];
    const std::vector<RmaMsg>& m = gRec[0].put.msgs;
    REQUIRE(s.nMsgs == 4 && s.nch == 4 && s.wgOff == 0 && gRec[0].put.grid == 4, "stream of %d messages on %d workgroups", s.nMsgs, s.nch);
    REQUIRE(m[0].src == kSrcBase && m[1].src == kSrcBase + 0x10000 && m[2].src == kSrcBase + 0x20000 && m[3].src == 0, "issue order");
    REQUIRE(m[0].nch == 4 && m[0].part % 16 == 0 && m[0].part * 4 >= m[0].bytes && m[1].nch == 1, "cut");
    REQUIRE(m[2].bytes == 0 && m[2].nch == 0 && m[3].bytes == 0 && m[3].nch == 0, "count == 0 is a signal");
    if (!launchesSound(f)) return false;
    gRec.clear();  // a lone signal: one workgroup
    REQUIRE(ncclSignal(1, 0, 0, 0, &f.comm, nullptr) == ncclSuccess && gRec.size() == 1 && gRec[0].put.grid == 1 && gRec[0].put.streams[0].peer == 1,
            "a lone self signal");
  }
  {  // beyond chanCap: split between peers, every stream whole
    Fixture f(5, 0, 4);
    f.comm.tune.p2pChunkBytes = 4096;
    gRec.clear();
    ncclGroupStart();
    for (int p = 1; p < 5; p++) put(f, (size_t)p * 0x10000, 3 * 4096, p, 0);
    put(f, 0x80000, 16, 1, 0);
    REQUIRE(ncclGroupEnd() == ncclSuccess, "group end");
    if (!launchesSound(f)) return false;
    std::map<int, std::vector<uint64_t>> got = perPeer(0, gRec.size(), &whole);
    REQUIRE(gRec.size() == 4 && whole && got.size() == 4 && got[1].size() == 2 && got[1][1] == kSrcBase + 0x80000, "chanCap split: %zu launches", gRec.size());
  }
  {  // beyond the argument block: 4 peers x 50 messages split between peers; 100 to one peer split in issue order
    Fixture f(5, 0, 256);
    gRec.clear();
    ncclGroupStart();
    for (int k = 0; k < 200; k++) put(f, (size_t)k * 16, 16, 1 + k % 4, 0);
    REQUIRE(ncclGroupEnd() == ncclSuccess, "group end");
    if (!launchesSound(f)) return false;
    std::map<int, std::vector<uint64_t>> got = perPeer(0, gRec.size(), &whole);
    REQUIRE(gRec.size() == 4 && whole && got.size() == 4, "argument block split: %zu launches", gRec.size());
    for (int p = 1; p <= 4; p++)
      for (int i = 0; i < 50; i++) REQUIRE(got[p].size() == 50 && got[p][i] == kSrcBase + (uint64_t)(4 * i + p - 1) * 16, "peer %d message %d out of order", p, i);
    gRec.clear();
    ncclGroupStart();
    for (int k = 0; k < 100; k++) put(f, (size_t)k * 16, 16, 3, 0);
    REQUIRE(ncclGroupEnd() == ncclSuccess, "group end");
    if (!launchesSound(f)) return false;
    REQUIRE(gRec.size() == 2 && gRec[0].put.msgs.size() == 96 && gRec[1].put.msgs.size() == 4 && gRec[1].put.msgs[0].src == kSrcBase + 96 * 16,
            "one long stream: %zu launches", gRec.size());
  }
  {  // another stream closes the batch; a refused call poisons the group and nothing launches
    Fixture f(4, 1, 256);
    gRec.clear();
    ncclGroupStart();
    put(f, 0, 100, 0, 0, (hipStream_t)0x10);
    put(f, 0, 100, 2, 0, (hipStream_t)0x20);
    REQUIRE(ncclGroupEnd() == ncclSuccess && gRec.size() == 2 && gRec[0].stream == (hipStream_t)0x10 && gRec[1].stream == (hipStream_t)0x20, "two streams");
    gRec.clear();
    ncclGroupStart();
    put(f, 0, 100, 0, 0);
    REQUIRE(put(f, 0, 100, 0, (size_t)1 << 24) == ncclInvalidArgument, "a put past the window was accepted");
    REQUIRE(ncclGroupEnd() == ncclInvalidArgument && gRec.empty(), "a poisoned group launched");
    REQUIRE(put(f, 0, 100, 0, 0) == ncclSuccess && gRec.size() == 1, "the communicator is unusable after a refused call");
    // ncclGroupSimulateEnd plans and drops
    gRec.clear();
    ncclSimInfo_t sim = NCCL_SIM_INFO_INITIALIZER;
    ncclGroupStart();
    put(f, 0, 1 << 20, 0, 0);
    REQUIRE(ncclGroupSimulateEnd(&sim) == ncclSuccess && gRec.empty() && sim.estimatedTime > 1.0f, "simulate: %f us, %zu launches", sim.estimatedTime, gRec.size());
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "args")) {
    Fixture f(4, 1, 256);
    auto report = [&](const char* what, ncclResult_t r) {
      printf("%s=%d launches=%zu\n", what, (int)r, gRec.size());
      gRec.clear();
    };
    const void* src = (const void*)kSrcBase;
    ncclWaitSignalDesc_t ok = {1, 0, 0, 0};
    report("put_nullcomm", ncclPutSignal(src, 0, ncclUint8, 0, &f.dst, 0, 0, 0, 0, nullptr, nullptr));
    report("signal_nullcomm", ncclSignal(0, 0, 0, 0, nullptr, nullptr));
    report("wait_nullcomm", ncclWaitSignal(1, &ok, nullptr, nullptr));
    report("put_type13", ncclPutSignal(src, 4, (ncclDataType_t)13, 0, &f.dst, 0, 0, 0, 0, &f.comm, nullptr));
    report("put_peer4", ncclPutSignal(src, 4, ncclUint8, 4, &f.dst, 0, 0, 0, 0, &f.comm, nullptr));
    report("signal_peer-1", ncclSignal(-1, 0, 0, 0, &f.comm, nullptr));
    report("put_ctx1", ncclPutSignal(src, 4, ncclUint8, 0, &f.dst, 0, 0, 1, 0, &f.comm, nullptr));
    report("put_sigidx1", ncclPutSignal(src, 4, ncclUint8, 0, &f.dst, 0, 1, 0, 0, &f.comm, nullptr));
    report("put_flags1", ncclPutSignal(src, 4, ncclUint8, 0, &f.dst, 0, 0, 0, 1, &f.comm, nullptr));
    report("signal_ctx1", ncclSignal(0, 0, 1, 0, &f.comm, nullptr));
    report("signal_sigidx1", ncclSignal(0, 1, 0, 0, &f.comm, nullptr));
    report("signal_flags1", ncclSignal(0, 0, 0, 1, &f.comm, nullptr));
    report("put_nullwin", ncclPutSignal(src, 4, ncclUint8, 0, nullptr, 0, 0, 0, 0, &f.comm, nullptr));
    report("put_nullbuff", ncclPutSignal(nullptr, 4, ncclUint8, 0, &f.dst, 0, 0, 0, 0, &f.comm, nullptr));
    report("put_nullbuff_count0", ncclPutSignal(nullptr, 0, ncclUint8, 0, &f.dst, 0, 0, 0, 0, &f.comm, nullptr));
    report("put_src_outside", ncclPutSignal((const void*)(kSrcBase + kSrcSize - 3), 4, ncclUint8, 0, &f.dst, 0, 0, 0, 0, &f.comm, nullptr));
    report("put_src_nonsym", ncclPutSignal(f.dst.userPtr, 4, ncclUint8, 0, &f.dst, 0, 0, 0, 0, &f.comm, nullptr));
    ncclWindow_vidmem stranger = f.dst;
    report("put_unknown_win", ncclPutSignal(src, 4, ncclUint8, 0, &stranger, 0, 0, 0, 0, &f.comm, nullptr));
    f.dst.peerSize[0] = 1000;
    f.dst.peerSize[2] = 1200;  // every rank registered another size: the bound is the peer's
    report("put_past_peer0", ncclPutSignal(src, 1, ncclFloat32, 0, &f.dst, 997, 0, 0, 0, &f.comm, nullptr));
    report("put_offset_past_peer0", ncclPutSignal(src, 0, ncclUint8, 0, &f.dst, 1001, 0, 0, 0, &f.comm, nullptr));
    report("put_huge_offset", ncclPutSignal(src, 4, ncclUint8, 0, &f.dst, ~(size_t)0 - 1, 0, 0, 0, &f.comm, nullptr));
    report("put_end_peer0", ncclPutSignal(src, 1, ncclFloat32, 0, &f.dst, 996, 0, 0, 0, &f.comm, nullptr));
    report("put_within_peer2", ncclPutSignal(src, 1, ncclFloat32, 2, &f.dst, 1196, 0, 0, 0, &f.comm, nullptr));
    report("wait_nulldescs", ncclWaitSignal(1, nullptr, &f.comm, nullptr));
    report("wait_ndesc0", ncclWaitSignal(0, &ok, &f.comm, nullptr));
    ncclWaitSignalDesc_t bad[2] = {{1, 0, 0, 0}, {1, 0, 0, 0}};
    bad[1].opCnt = 0;
    report("wait_opcnt0", ncclWaitSignal(2, bad, &f.comm, nullptr));
    bad[1] = {1, 0, 1, 0};
    report("wait_sigidx1", ncclWaitSignal(2, bad, &f.comm, nullptr));
    bad[1] = {1, 0, 0, 1};
    report("wait_ctx1", ncclWaitSignal(2, bad, &f.comm, nullptr));
    bad[1] = {1, 4, 0, 0};
    report("wait_peer4", ncclWaitSignal(2, bad, &f.comm, nullptr));
    bad[1] = {1, -1, 0, 0};
    report("wait_peer-1", ncclWaitSignal(2, bad, &f.comm, nullptr));
    report("put_ok", ncclPutSignal(src, 100, ncclFloat32, 2, &f.dst, 8, 0, 0, 0, &f.comm, nullptr));
    report("put_self_ok", ncclPutSignal(src, 100, ncclUint8, 1, &f.dst, 8, 0, 0, 0, &f.comm, nullptr));
    report("put_count0_ok", ncclPutSignal(src, 0, ncclFloat32, 2, &f.dst, 8, 0, 0, 0, &f.comm, nullptr));
    report("signal_ok", ncclSignal(3, 0, 0, 0, &f.comm, nullptr));
    report("wait_ok", ncclWaitSignal(1, &ok, &f.comm, nullptr));
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "batch")) {
    if (!batchChecks()) return 1;
    printf("OK checks=%d\n", gChecks);
    return 0;
  }
  fprintf(stderr, "usage: rma_plan_test args | batch\n");
  return 2;
}
