// p2p_plan_test.cc — CPU test driver of the ncclSend / ncclRecv host plan (p2p.cc) and of the cut the p2p kernel walks.
// Compiled with p2p.cc, enqueue.cc and debug.cc like bcast_plan_test (no GPU: launches, the group machinery and the
// few HIP calls are stubbed), it slices every message with the SAME host-callable functions the kernel calls
// (device_abi.h p2pCut / p2pSteps / sliceBounds), so nothing of the arithmetic is restated here.
//
//   p2p_plan_test cut        n in 2..16 x byte counts x slot sizes {4096, default}: a message's descriptor is identical
//                            when planned as the sender among arbitrary other ops and as the receiver alone (symmetry),
//                            and its (channel, step) slices tile [0, bytes) exactly once with no empty channel below
//                            nch (coverage). Prints "OK cases=<n> maxnch=<n>".
//   p2p_plan_test pack       n in {2, 5, 8, 16} x grid budgets {2, 4, 16, 32, 512} x random op sets: every launch within
//                            the budget, rounds increasing across launches, a round's send and recv streams in one
//                            launch, every message planned once and in issue order; a budget of 1 is refused.
//                            Prints "OK cases=<n> launches=<n> split=<n>".
//   p2p_plan_test self       self sends and recvs: "matched=<r> copies=<n> sendonly=<r> recvonly=<r> onerank=<r>"
//   p2p_plan_test args       the entry points: "<call>=<ncclResult_t> launches=<n>" per line
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

#include "plan_stubs.h"

namespace ncclamd {
static int gLaunches = 0;
ncclResult_t launchP2pKernel(const ncclComm*, const P2pLaunch&, hipStream_t) {
  gLaunches++;
  return ncclSuccess;
}
// the group machinery, reduced to what an ungrouped p2p call needs: record, then plan and launch at the end
static int gDepth = 0;
static ncclResult_t gGroupError = ncclSuccess;
static std::vector<P2pOp> gOps;
bool groupActive() { return gDepth > 0; }
ncclResult_t groupStartInternal() { gDepth++; return ncclSuccess; }
ncclResult_t groupDeferColl(const CollInfo&) { return ncclSuccess; }
ncclResult_t groupDeferP2p(const P2pOp& op) { gOps.push_back(op); return ncclSuccess; }
void groupRecordError(ncclResult_t r) { if (gDepth > 0 && gGroupError == ncclSuccess) gGroupError = r; }
ncclResult_t groupEndInternal(ncclSimInfo_t*) {
  if (--gDepth > 0) return ncclSuccess;
  std::vector<P2pOp> ops;
  ops.swap(gOps);
  ncclResult_t r = gGroupError;
  gGroupError = ncclSuccess;
  if (r != ncclSuccess || ops.empty()) return r;
  P2pPlan plan;
  r = p2pPlan(ops[0].comm, ops, &plan);
  return r == ncclSuccess ? p2pLaunchPlan(ops[0].comm, plan, ops[0].stream) : r;
}
}  // namespace ncclamd

using namespace ncclamd;

// p2p.cc launches no collective (a collective launch is an error); buffers count as registered
static void initComm(ncclComm& comm, int n, int rank, size_t slotBytes, int chanCap) {
  gStubs.refuseLaunch = gStubs.refuseSymLaunch = gStubs.regLookupAlways = gStubs.regCoversAnswer = true;
  stubComm(comm, n, rank, slotBytes, chanCap);
}

#define REQUIRE(cond, ...)          \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, "FAIL: ");    \
      fprintf(stderr, __VA_ARGS__); \
      fputc('\n', stderr);          \
      return false;                 \
    }                               \
  } while (0)

static uint32_t gRng = 12345;
static uint32_t rnd() { return gRng = gRng * 1664525u + 1013904223u; }

// the message with user pointer `ptr` in a plan, and the stream (direction, peer) that carries it
static const P2pMsg* findMsg(const P2pPlan& plan, uint64_t ptr, const P2pStream** stream) {
  for (const P2pLaunch& l : plan.launches)
    for (const P2pStream& s : l.streams)
      for (int k = 0; k < s.nMsgs; k++)
        if (l.msgs[s.msgOff + k].ptr == ptr) {
          *stream = &s;
          return &l.msgs[s.msgOff + k];
        }
  return nullptr;
}

static bool checkCut(int n, size_t bytes, size_t slotBytes, int* maxNch) {
  ncclComm a, b;
  initComm(a, n, 0, slotBytes, 256);
  initComm(b, n, n - 1, slotBytes, 256);
  // the sender: the message among arbitrary other ops (other peers, the same peer before and after, recvs)
  std::vector<P2pOp> ops;
  const int others = (int)(rnd() % 6);
  for (int k = 0; k < others; k++)
    ops.push_back({&a, nullptr, (void*)(uintptr_t)(0x1000000 + 0x100000 * k), (size_t)(rnd() % 3000000), 1 + (int)(rnd() % (n - 1)), (rnd() & 1) != 0});
  const size_t at = ops.empty() ? 0 : rnd() % (ops.size() + 1);
  ops.insert(ops.begin() + at, {&a, nullptr, (void*)(uintptr_t)0x7f000010, bytes, n - 1, false});
  const std::vector<P2pOp> alone = {{&b, nullptr, (void*)(uintptr_t)0x7e000000, bytes, 0, true}};
  P2pPlan pa, pb;
  REQUIRE(p2pPlan(&a, ops, &pa) == ncclSuccess && p2pPlan(&b, alone, &pb) == ncclSuccess, "n %d bytes %zu: plan failed", n, bytes);
  const P2pStream *sa = nullptr, *sb = nullptr;
  const P2pMsg* ma = findMsg(pa, 0x7f000010, &sa);
  const P2pMsg* mb = findMsg(pb, 0x7e000000, &sb);
  if (bytes == 0) {  // no descriptor, no workgroup, no handshake on either side
    REQUIRE(!ma && !mb && pb.launches.empty(), "n %d: an empty message was planned", n);
    return true;
  }
  REQUIRE(ma && mb, "n %d bytes %zu: message missing from a plan", n, bytes);
  REQUIRE(sa->recv == 0 && sa->peer == n - 1 && sb->recv == 1 && sb->peer == 0, "n %d bytes %zu: wrong stream", n, bytes);
  REQUIRE(ma->bytes == bytes && mb->bytes == bytes && ma->nch == mb->nch && ma->part == mb->part,
          "n %d bytes %zu slot %zu: sender plans nch %u part %lu, receiver nch %u part %lu", n, bytes, slotBytes, ma->nch,
          (unsigned long)ma->part, mb->nch, (unsigned long)mb->part);
  REQUIRE(ma->nch >= 1 && (int)ma->nch <= sa->nch && (int)mb->nch <= sb->nch && sa->nch <= 128 && ma->part % 16 == 0,
          "n %d bytes %zu: nch %u of stream %d, part %lu", n, bytes, ma->nch, sa->nch, (unsigned long)ma->part);
  if ((int)ma->nch > *maxNch) *maxNch = (int)ma->nch;
  const uint64_t slice = p2pSliceBytes(a.slotBytes);
  std::vector<unsigned char> seen(bytes, 0);
  for (int j = 0; j < (int)ma->nch; j++) {
    const int steps = p2pSteps(bytes, ma->part, slice, j);
    REQUIRE(steps >= 1, "n %d bytes %zu: channel %d of %u is empty", n, bytes, j, ma->nch);
    for (int s = 0; s < steps; s++) {
      uint64_t lo, hi;
      sliceBounds(ma->part, slice, j, s, bytes, lo, hi);
      REQUIRE(lo < hi && hi <= bytes && hi - lo <= slice && hi - lo <= a.slotBytes && lo % 16 == 0,
              "n %d bytes %zu: channel %d step %d: [%lu, %lu)", n, bytes, j, s, (unsigned long)lo, (unsigned long)hi);
      for (uint64_t x = lo; x < hi; x++) {
        REQUIRE(!seen[x], "n %d bytes %zu: byte %lu moved twice", n, bytes, (unsigned long)x);
        seen[x] = 1;
      }
    }
    uint64_t lo, hi;  // ... and nothing beyond the last step
    sliceBounds(ma->part, slice, j, steps, bytes, lo, hi);
    REQUIRE(lo == hi, "n %d bytes %zu: channel %d has a slice past its %d steps", n, bytes, j, steps);
  }
  for (size_t x = 0; x < bytes; x++) REQUIRE(seen[x], "n %d bytes %zu: byte %zu never moved", n, bytes, x);
  return true;
}

static bool checkPack(int n, int budget, int* launches, int* split) {
  ncclComm comm;
  const int me = (int)(rnd() % n);
  initComm(comm, n, me, 4096, budget);
  std::vector<P2pOp> ops;
  const int nOps = 1 + (int)(rnd() % 40);
  std::map<std::pair<int, int>, std::vector<uint64_t>> want;  // (recv, peer) -> its messages' pointers in issue order
  for (int k = 0; k < nOps; k++) {
    int peer = (int)(rnd() % n);
    if (peer == me) peer = (peer + 1) % n;
    const bool recv = (rnd() & 1) != 0;
    const size_t sizes[] = {0, 1, 4096, 70001, 300001, (size_t)1 << 20, (size_t)5 << 20};
    const size_t bytes = sizes[rnd() % 7];
    const uint64_t ptr = 0x10000000ull + (uint64_t)k * 0x1000000ull;
    ops.push_back({&comm, nullptr, (void*)(uintptr_t)ptr, bytes, peer, recv});
    if (bytes) want[{recv ? 1 : 0, peer}].push_back(ptr);
  }
  P2pPlan plan;
  const ncclResult_t r = p2pPlan(&comm, ops, &plan);
  REQUIRE(r == ncclSuccess, "n %d budget %d: plan failed with %d", n, budget, (int)r);
  std::map<std::pair<int, int>, std::vector<uint64_t>> got;
  int lastRound = 0;
  for (const P2pLaunch& l : plan.launches) {
    REQUIRE(l.grid >= 1 && l.grid <= budget, "n %d budget %d: a launch of %d workgroups", n, budget, l.grid);
    REQUIRE(l.firstRound > lastRound && l.lastRound >= l.firstRound && l.lastRound < n,
            "n %d budget %d: launch rounds %d..%d after round %d", n, budget, l.firstRound, l.lastRound, lastRound);
    lastRound = l.lastRound;
    int off = 0, round = 0;
    for (const P2pStream& s : l.streams) {
      REQUIRE(s.wgOff == off && s.nch >= 1 && s.nch <= comm.maxChannels && s.nch <= budget / 2, "n %d budget %d: stream at %d of %d channels, expected at %d",
              n, budget, s.wgOff, s.nch, off);
      off += s.nch;
      // the round of a stream: send to me + r, recv from me - r
      const int rr = s.recv ? (me - s.peer + n) % n : (s.peer - me + n) % n;
      REQUIRE(rr >= l.firstRound && rr <= l.lastRound && rr >= round, "n %d budget %d: round %d in launch %d..%d", n, budget, rr, l.firstRound, l.lastRound);
      round = rr;
      int nchMax = 0;
      for (int k = 0; k < s.nMsgs; k++) {
        const P2pMsg& m = l.msgs[s.msgOff + k];
        got[{s.recv, s.peer}].push_back(m.ptr);
        nchMax = (int)m.nch > nchMax ? (int)m.nch : nchMax;
        const P2pCut cut = p2pCutFor(&comm, m.bytes);
        REQUIRE(m.bytes > 0 && (int)m.nch == cut.nch && m.part == cut.part, "n %d budget %d: a message's cut differs from p2pCutFor", n, budget);
      }
      REQUIRE(nchMax == s.nch, "n %d budget %d: stream of %d channels, its widest message has %d", n, budget, s.nch, nchMax);
    }
    REQUIRE(off == l.grid, "n %d budget %d: streams cover %d of %d workgroups", n, budget, off, l.grid);
  }
  // every stream whole in ONE launch (so a round's send and recv, both within the launch's round range, are together),
  // every message once and in issue order
  REQUIRE(got == want, "n %d budget %d: the planned messages are not the issued ones in issue order", n, budget);
  for (const auto& kv : want) {
    int in = 0;
    for (const P2pLaunch& l : plan.launches)
      for (const P2pStream& s : l.streams) in += s.recv == kv.first.first && s.peer == kv.first.second;
    REQUIRE(in == 1, "n %d budget %d: stream (%d, %d) appears in %d launches", n, budget, kv.first.first, kv.first.second, in);
  }
  *launches += (int)plan.launches.size();
  *split += plan.launches.size() > 1;
  return true;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "cut")) {
    int cases = 0, maxNch = 0;
    for (int n = 2; n <= 16; n++)
      for (size_t slot : {(size_t)4096, (size_t)0}) {
        ncclComm probe;
        initComm(probe, n, 0, slot, 256);
        const size_t sb = probe.slotBytes;
        const size_t mx = (size_t)p2pCutFor(&probe, (size_t)1 << 40).nch;  // the channel cap of one message
        const size_t sizes[] = {0, 1, 15, 16, 17, sb - 1, sb, sb + 1, 16 * mx - 1, 16 * mx + 1, 300001, ((size_t)1 << 20) | 3};
        for (size_t bytes : sizes) {
          if (!checkCut(n, bytes, slot, &maxNch)) return 1;
          cases++;
        }
      }
    printf("OK cases=%d maxnch=%d\n", cases, maxNch);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "pack")) {
    int cases = 0, launches = 0, split = 0;
    for (int n : {2, 5, 8, 16})
      for (int budget : {2, 4, 16, 32, 512})
        for (int rep = 0; rep < 25; rep++) {
          if (!checkPack(n, budget, &launches, &split)) return 1;
          cases++;
        }
    ncclComm comm;  // one workgroup cannot hold a round's two streams
    initComm(comm, 4, 0, 4096, 1);
    P2pPlan plan;
    const std::vector<P2pOp> one = {{&comm, nullptr, (void*)(uintptr_t)0x1000, 100, 1, false}};
    if (p2pPlan(&comm, one, &plan) == ncclSuccess) return fprintf(stderr, "FAIL: a budget of 1 was accepted\n"), 1;
    printf("OK cases=%d launches=%d split=%d\n", cases, launches, split);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "self")) {
    ncclComm comm, solo;
    initComm(comm, 3, 1, 0, 256);
    initComm(solo, 1, 0, 0, 256);
    void* p = (void*)(uintptr_t)0x1000;
    void* q = (void*)(uintptr_t)0x2000;
    P2pPlan plan;
    const std::vector<P2pOp> both = {{&comm, nullptr, p, 100, 1, false}, {&comm, nullptr, q, 100, 1, true}};
    const ncclResult_t matched = p2pPlan(&comm, both, &plan);
    const size_t copies = plan.self.size(), launches = plan.launches.size();
    const ncclResult_t sendOnly = p2pPlan(&comm, {{&comm, nullptr, p, 100, 1, false}}, &plan);
    const ncclResult_t recvOnly = p2pPlan(&comm, {{&comm, nullptr, q, 100, 1, true}}, &plan);
    const ncclResult_t oneRank = p2pPlan(&solo, {{&solo, nullptr, p, 100, 0, false}, {&solo, nullptr, q, 100, 0, true}}, &plan);
    const ncclResult_t oneRankAlone = p2pPlan(&solo, {{&solo, nullptr, p, 100, 0, false}}, &plan);
    printf("matched=%d copies=%zu launches=%zu sendonly=%d recvonly=%d onerank=%d onerankalone=%d\n", (int)matched, copies, launches,
           (int)sendOnly, (int)recvOnly, (int)oneRank, (int)oneRankAlone);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "args")) {
    ncclComm comm;
    initComm(comm, 4, 1, 0, 256);
    void* p = (void*)(uintptr_t)0x10000000;
    void* q = (void*)(uintptr_t)0x20000000;
    auto report = [&](const char* what, ncclResult_t r) {
      printf("%s=%d launches=%d\n", what, (int)r, gLaunches);
      gLaunches = 0;
    };
    report("send_peer4", ncclSend(p, 100, ncclUint8, 4, &comm, nullptr));
    report("recv_peer-1", ncclRecv(p, 100, ncclUint8, -1, &comm, nullptr));
    report("gather_root4", ncclGather(p, q, 100, ncclUint8, 4, &comm, nullptr));
    report("scatter_root-1", ncclScatter(p, q, 100, ncclUint8, -1, &comm, nullptr));
    report("send_type13", ncclSend(p, 100, (ncclDataType_t)13, 2, &comm, nullptr));  // (past ncclNumTypes, inside the enum's range)
    report("send_nullcomm", ncclSend(p, 0, ncclUint8, 0, nullptr, nullptr));
    report("send_ok", ncclSend(p, 100, ncclFloat32, 2, &comm, nullptr));
    report("send_empty", ncclSend(p, 0, ncclFloat32, 2, &comm, nullptr));
    report("alltoall_ok", ncclAlltoAll(p, q, 100, ncclFloat16, &comm, nullptr));
    report("gather_ok", ncclGather(p, q, 100, ncclUint8, 1, &comm, nullptr));
    report("scatter_ok", ncclScatter(p, q, 100, ncclUint8, 3, &comm, nullptr));
    return 0;
  }
  fprintf(stderr, "usage: p2p_plan_test cut | pack | self | args\n");
  return 2;
}
