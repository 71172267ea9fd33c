// p2p_zc_plan_test.cc — CPU test driver of the RDV (zero-copy rendezvous) planning of ncclSend / ncclRecv: p2p.cc with
// the launches stubbed, like p2p_plan_test, and the host-callable descriptor functions of device_abi.h.
//   desc   the descriptor's pack / unpack round trip at the serial and offset extremes, and the serial's wrap past 0
//   kind   a message's kind at the LL and RDV thresholds, alike on both ends; the receiver's descriptor for a recvbuff
//          inside, outside and straddling a window
//   cap    a launch that holds an RDV message respects the smaller message cap, one descriptor beside every message
// Each prints "OK <counts>".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "plan_stubs.h"

namespace ncclamd {
ncclResult_t launchP2pKernel(const ncclComm*, const P2pLaunch&, hipStream_t) { return ncclSuccess; }
bool groupActive() { return false; }
ncclResult_t groupStartInternal() { return ncclSuccess; }
ncclResult_t groupDeferColl(const CollInfo&) { return ncclSuccess; }
ncclResult_t groupDeferP2p(const P2pOp&) { return ncclSuccess; }
void groupRecordError(ncclResult_t) {}
ncclResult_t groupEndInternal(ncclSimInfo_t*) { return ncclSuccess; }
}  // namespace ncclamd

using namespace ncclamd;

#define REQUIRE(cond, ...)          \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, "FAIL: ");    \
      fprintf(stderr, __VA_ARGS__); \
      fputc('\n', stderr);          \
      return 1;                     \
    }                               \
  } while (0)

static constexpr size_t kLL = 256, kZc = 4096;
static P2pZcWinTable gTable;
static ncclWindow_vidmem gWin;

// a communicator with LL up to kLL bytes, RDV from kZc bytes, and one window [0x10000000, +1 MiB) under serial 7
static void initComm(ncclComm& comm, int n, int rank) {
  stubComm(comm, n, rank, 4096, 64);
  comm.tune.p2pLLBytes = kLL;
  comm.p2pLLChannels = 2;
  comm.p2pLLLineBytes = 256;
  comm.tune.p2pZcBytes = kZc;
  comm.p2pZcChannels = 32;
  memset(&gTable, 0, sizeof(gTable));
  memset(&gWin, 0, sizeof(gWin));
  gWin.comm = &comm;
  gWin.userPtr = (void*)(uintptr_t)0x10000000;
  gWin.size = 1 << 20;
  gTable.serial[7] = 7;
  gTable.win[7] = &gWin;
  comm.p2pZcTable = &gTable;
}

static int testDesc() {
  int cases = 0;
  for (uint32_t serial : {0u, 1u, 7u, kP2pZcSerialMax - 1, kP2pZcSerialMax})
    for (uint64_t off : {(uint64_t)0, (uint64_t)1, (uint64_t)15, (uint64_t)1 << 32, kP2pZcOffsetMax - 1, kP2pZcOffsetMax}) {
      const uint64_t d = p2pZcPack(serial, off);
      REQUIRE(p2pZcSerial(d) == serial && p2pZcOffset(d) == off, "serial %u offset %lu -> %lx", serial, (unsigned long)off, (unsigned long)d);
      cases++;
    }
  REQUIRE(p2pZcNextSerial(0) == 1 && p2pZcNextSerial(kP2pZcSerialMax - 1) == kP2pZcSerialMax && p2pZcNextSerial(kP2pZcSerialMax) == 1,
          "the serial wraps past 0");
  printf("OK cases=%d\n", cases);
  return 0;
}

static int testKind() {
  ncclComm a, b;
  int cases = 0;
  struct Case { size_t bytes; uint32_t kind; };
  for (const Case& k : {Case{kLL, P2P_LL}, Case{kLL + 1, P2P_STAGED}, Case{kZc - 1, P2P_STAGED}, Case{kZc, P2P_RDV},
                        Case{kZc + 1, P2P_RDV}, Case{(size_t)300001, P2P_RDV}}) {
    // recvbuff: inside the window at an odd offset, ending exactly at its end, one byte past it, outside any window
    for (uintptr_t rp : {(uintptr_t)0x10000003, (uintptr_t)0x10000000 + (1 << 20) - k.bytes,
                         (uintptr_t)0x10000001 + (1 << 20) - k.bytes, (uintptr_t)0x30000000}) {
      initComm(a, 3, 0);
      P2pPlan pa, pb;
      REQUIRE(p2pPlan(&a, {{&a, nullptr, (void*)(uintptr_t)0x10000040, k.bytes, 2, false}}, &pa) == ncclSuccess, "send plan");
      initComm(b, 3, 2);
      REQUIRE(p2pPlan(&b, {{&b, nullptr, (void*)rp, k.bytes, 0, true}}, &pb) == ncclSuccess, "recv plan");
      const P2pLaunch &la = pa.launches.at(0), &lb = pb.launches.at(0);
      const P2pMsg &ma = la.msgs.at(0), &mb = lb.msgs.at(0);
      REQUIRE(ma.ll == k.kind && mb.ll == k.kind && ma.nch == mb.nch && ma.part == mb.part, "bytes %zu: kinds %u / %u, want %u",
              k.bytes, ma.ll, mb.ll, k.kind);
      REQUIRE((la.nRdv == 1) == (k.kind == P2P_RDV) && la.descs.size() == (k.kind == P2P_RDV ? 1u : 0u), "bytes %zu: sender's launch", k.bytes);
      if (k.kind == P2P_RDV) {
        // the sender plans no descriptor, even with its sendbuff in the window; the receiver's names the window iff the
        // recvbuff lies wholly inside it
        const bool inside = rp >= 0x10000000 && rp + k.bytes <= 0x10000000 + (1 << 20);
        REQUIRE(la.descs[0] == 0 && lb.descs.size() == 1, "bytes %zu: descriptors", k.bytes);
        REQUIRE(lb.descs[0] == (inside ? p2pZcPack(7, rp - 0x10000000) : 0), "bytes %zu recvbuff %lx: descriptor %lx", k.bytes,
                (unsigned long)rp, (unsigned long)lb.descs[0]);
      }
      cases++;
    }
  }
  // without the area (the knob unset at init) nothing is RDV
  initComm(a, 3, 0);
  a.p2pZcChannels = 0;
  P2pPlan p;
  REQUIRE(p2pPlan(&a, {{&a, nullptr, (void*)(uintptr_t)0x10000000, 300001, 1, true}}, &p) == ncclSuccess &&
              p.launches.at(0).msgs.at(0).ll == P2P_STAGED && p.launches[0].descs.empty(), "no area: staged");
  printf("OK cases=%d\n", cases + 1);
  return 0;
}

// one round (n = 8, rank 0, peer 4) of `count` messages of 1000 bytes, sends and recvs in turn; message rdvAt is RDV
static std::vector<P2pOp> roundOf(ncclComm* c, int count, int rdvAt) {
  std::vector<P2pOp> ops;
  for (int k = 0; k < count; k++)
    ops.push_back({c, nullptr, (void*)(uintptr_t)(0x10000000 + 8192 * k), k == rdvAt ? kZc : (size_t)1000, 4, (k & 1) != 0});
  return ops;
}

static int testCap() {
  ncclComm a;
  initComm(a, 8, 0);
  P2pPlan p;
  REQUIRE(p2pPlan(&a, roundOf(&a, kP2pMaxMsgs, -1), &p) == ncclSuccess && p.launches.size() == 1 && p.launches[0].descs.empty(),
          "96 staged messages of one round: one launch, no descriptors");
  REQUIRE(p2pPlan(&a, roundOf(&a, kP2pZcMaxMsgs + 1, 5), &p) == ncclInvalidUsage, "81 messages of one round, one RDV: refused");
  REQUIRE(p2pPlan(&a, roundOf(&a, kP2pZcMaxMsgs, 5), &p) == ncclSuccess && p.launches.size() == 1, "80 messages, one RDV");
  const P2pLaunch& l = p.launches[0];
  REQUIRE(l.nRdv == 1 && l.descs.size() == l.msgs.size() && sizeof(P2pZcArgs<kP2pMaxStreams, kP2pZcMaxMsgs>) < 4096, "argument block");
  for (const P2pStream& s : l.streams)   // the received RDV message (issue index 5, a recv) alone has a descriptor
    for (int k = 0; k < s.nMsgs; k++)
      REQUIRE((l.msgs[s.msgOff + k].ll == P2P_RDV && s.recv) == (l.descs[s.msgOff + k] != 0), "descriptor beside its message");
  printf("OK launches=%zu\n", p.launches.size());
  return 0;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "desc")) return testDesc();
  if (!strcmp(mode, "kind")) return testKind();
  if (!strcmp(mode, "cap")) return testCap();
  fprintf(stderr, "usage: p2p_zc_plan_test desc|kind|cap\n");
  return 2;
}
