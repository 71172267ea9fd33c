// plan_test.cc — CPU test driver for the host-side planning of enqueue.cc (size table, protocol and
// algorithm choice, channel/slice plan, NCCL_ALGO / NCCL_PROTO handling). It is compiled together with
// the planning sources (no GPU, no HIP runtime): the launch entry points and the few HIP runtime calls
// they make are stubbed (plan_stubs.h) so every plan is recorded and printed instead of launched.
//
//   plan_test NRANKS FUNC(ar|rs|ag|reduce) DTYPE COUNT [ALIGN_OFFSET_BYTES] [CHANCAP]
// prints one line: algo=<copy|onerank|direct|oneshot|ll|ring|chain> nch=<channels> part=<elements|payloads>
//                  slice=<elements> steps=<n> chunk=<elements> (ring / chain also: kind= cbdlo= cbdhi=)
//   plan_test NRANKS many FUNC:DTYPE:COUNT[:ROOT] ...
// the same line for every op in turn, each planned alone on one communicator ("error=<ncclResult_t>" where planning fails)
//   PLAN_GEOMETRY=1 (both forms above): the communicator's shape as init.cc commDefaults reads it from the environment
//   (NCCL_MAX_CTAS / NCCL_MAX_NCHANNELS below CHANCAP, NCCL_MIN_CTAS, NCCL_AMD_NSLOTS, and the slot size from
//   NCCL_AMD_STAGING_MIB, NCCL_BUFFSIZE and NCCL_AMD_SLOT_BYTES); PLAN_WINDOW=1: every buffer lies in a symmetric window
//   plan_test NRANKS batch FUNC:DTYPE:COUNT[:OP] ...
// plans the ops as one group (enqueue.cc planColl / batchable / launchBatch, in group.cc's order) and prints one
// line per launch: algo=<...> ops=<ops in the launch> grid=<workgroups> ranges=<chOff+nch per op, comma-separated>
//   plan_test dump NRANKS FUNC DTYPE COUNT [ALIGN_OFFSET_BYTES] [CHANCAP]
//   plan_test dump NRANKS batch FUNC:DTYPE:COUNT[:OP[:ROOT]] ...
// the same op or group, printed as every member of what reached launchPlan / launchSymPlan (one line per launch,
// fields in hexadecimal), then "result=<ncclResult_t> kind=<-1 nothing|0 kernel|1 symmetric> opCount=<n>"
//   plan_test sweep | sweep-full | sweep-time [REPEATS]
// the dump in process over the grid of sweepAll() below: one line per (configuration, rank count) with the number of
// cases and, per collective, the 64-bit FNV-1a hash of their dump lines; then one line per (batch configuration, rank
// count) with a hash per channel-limit row (tests/golden/plan_digest.txt; tests/test_plan_golden.py). The dump also
// holds what planning passes out to findSymWindow / regLookup / regCovers / tunerPick (" C" lines).
// sweep-full prints the lines themselves, so that two builds can be diffed where a digest differs; sweep-time plans
// the grid REPEATS times without formatting anything and prints the plans per second.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <string>
#include <vector>

#define PLAN_STUBS_NO_GROUP
#include "plan_stubs.h"

using namespace ncclamd;

static const char* kAlgoNames[] = {"copy", "onerank", "direct", "oneshot", "ll", "pipe"};

// batch mode: one line per launch
static void printBatchLaunch(const LaunchPlan& p) {
  printf("algo=%s", kAlgoNames[p.algo]);
  if (p.algo == ALGO_LL) {
    printf(" ops=%d grid=%d ranges=", p.ll.nOps, p.nChannels);
    for (int k = 0; k < p.ll.nOps; k++) printf("%s%d+%d", k ? "," : "", p.ll.ops[k].chOff, p.ll.ops[k].nch);
    if (p.ll.nOps > 1) {  // per channel: the ops it runs (LLArgs::chMask)
      printf(" masks=");
      for (int c = 0; c < kMaxLLChannels; c++) printf("%s%x", c ? "," : "", p.ll.chMask[c]);
    }
  } else if (p.batch.nOps > 1) {
    printf(" ops=%d grid=%d ranges=", p.batch.nOps, p.nChannels);
    for (int k = 0; k < p.batch.nOps; k++) printf("%s%d+%d", k ? "," : "", p.batch.chOff[k], p.batch.nch[k]);
  } else {
    printf(" ops=1 grid=%d ranges=0+%d", p.nChannels, p.nChannels);
  }
  printf("\n");
}

// ---- the dump: every member of a launch as text, field by field (no raw bytes: padding never enters) ----
enum DumpMode { DUMP_OFF = 0, DUMP_HASH = 1, DUMP_PRINT = 2 };
static struct Dump {
  int mode = DUMP_OFF;
  uint64_t hash = 0;
  char buf[1 << 16];
  size_t n = 0;
  void str(const char* s) {
    while (*s) buf[n++] = *s++;
  }
  void val(uint64_t v) {
    char t[16];
    int k = 0;
    do t[k++] = "0123456789abcdef"[v & 15]; while (v >>= 4);
    while (k) buf[n++] = t[--k];
  }
  void f(const char* name, uint64_t v) {
    buf[n++] = ' ';
    str(name);
    buf[n++] = '=';
    val(v);
  }
  void f(const char* name, const void* v) { f(name, (uint64_t)(uintptr_t)v); }
  void f(const char* name, int v) { f(name, (uint64_t)(int64_t)v); }
  void f(const char* name, uint32_t v) { f(name, (uint64_t)v); }
  void f(const char* name, int64_t v) { f(name, (uint64_t)v); }
  void f(const char* name, bool v) { f(name, (uint64_t)v); }
  void endLine() {
    buf[n++] = '\n';
    for (size_t i = 0; i < n; i++) hash = (hash ^ (unsigned char)buf[i]) * 1099511628211ull;
    if (mode == DUMP_PRINT) fwrite(buf, 1, n, stdout);
    n = 0;
  }
} gDump;

static void dumpCollArgs(const char* tag, const CollArgs& a) {
  Dump& d = gDump;
  d.str(tag);
  d.f("sendbuff", a.sendbuff), d.f("recvbuff", a.recvbuff), d.f("comm", (const void*)a.comm), d.f("count", a.count);
  d.f("chunk", a.chunk), d.f("part", a.part), d.f("slice", a.slice), d.f("redArg", a.redArg), d.f("redArgPtr", a.redArgPtr);
  d.f("nSteps", a.nSteps), d.f("root", a.root), d.f("aligned", a.aligned), d.f("protoFlags", a.protoFlags);
  d.f("cbdLo", a.cbdLo), d.f("cbdHi", a.cbdHi), d.f("refSub", a.refSub), d.f("refPad", a.refPad);
}

static void dumpLaunchPlan(const LaunchPlan& p) {
  if (gDump.mode == DUMP_OFF) return;
  Dump& d = gDump;
  d.str(" K");
  d.f("func", (int)p.func), d.f("algo", p.algo), d.f("datatype", (int)p.datatype), d.f("eltSize", p.eltSize);
  d.f("devOp", p.devOp), d.f("nChannels", p.nChannels), d.f("bytes", (uint64_t)p.bytes), d.f("stream", (const void*)p.stream);
  d.f("copyVariant", p.copyVariant), d.f("copyGrid", p.copyGrid), d.f("copyXcdShift", p.copyXcdShift), d.f("pipeKind", p.pipeKind);
  dumpCollArgs(" args:", p.args);
  d.str(" ll:");
  d.f("comm", (const void*)p.ll.comm), d.f("counters", (const void*)p.ll.counters), d.f("redArg", p.ll.redArg);
  d.f("redArgPtr", p.ll.redArgPtr), d.f("nOps", p.ll.nOps);
  d.str(" chMask=");
  for (int c = 0; c < kMaxLLChannels; c++) d.val(p.ll.chMask[c]), d.str(c + 1 < kMaxLLChannels ? "," : "");
  for (int k = 0; k < p.ll.nOps && k < kMaxLLBatch; k++) {
    const LLOp& o = p.ll.ops[k];
    d.str(" op:");
    d.f("send", o.send), d.f("recv", o.recv), d.f("count", o.count), d.f("chunk", o.chunk), d.f("part", o.part);
    d.f("nch", o.nch), d.f("chOff", o.chOff), d.f("coll", o.coll), d.f("root", o.root), d.f("proto", o.proto);
  }
  d.str(" batch:");
  d.f("nOps", p.batch.nOps);
  for (int k = 0; k < p.batch.nOps && k < kMaxCollBatch; k++) {
    dumpCollArgs(" bop:", p.batch.op[k]);
    d.f("chOff", p.batch.chOff[k]), d.f("nch", p.batch.nch[k]);
  }
  d.endLine();
}

static void dumpSymPlan(const SymPlan& p) {
  if (gDump.mode == DUMP_OFF) return;
  Dump& d = gDump;
  d.str(" S");
  d.f("coll", p.coll), d.f("datatype", (int)p.datatype), d.f("eltSize", p.eltSize), d.f("devOp", p.devOp);
  d.f("nChannels", p.nChannels), d.f("stream", (const void*)p.stream);
  d.f("regUse0", (const void*)p.regUse[0]), d.f("regUse1", (const void*)p.regUse[1]), d.f("bounced", p.bounced);
  const SymArgs& a = p.args;
  d.str(" args:");
  d.f("comm", (const void*)a.comm);
  d.str(" send=");
  for (int r = 0; r < NCCL_AMD_MAX_RANKS; r++) d.val((uint64_t)(uintptr_t)a.send[r]), d.str(",");
  d.str(" recv=");
  for (int r = 0; r < NCCL_AMD_MAX_RANKS; r++) d.val((uint64_t)(uintptr_t)a.recv[r]), d.str(",");
  d.f("count", a.count), d.f("chunk", a.chunk), d.f("part", a.part), d.f("redArg", a.redArg), d.f("redArgPtr", a.redArgPtr);
  d.f("aligned", a.aligned), d.f("wtPublish", a.wtPublish), d.f("regMode", a.regMode), d.f("relFence", a.relFence);
  const SymA2AArgs& b = p.a2a;
  d.str(" a2a:");
  d.f("comm", (const void*)b.comm);
  d.str(" send=");
  for (int r = 0; r < NCCL_AMD_MAX_RANKS; r++) d.val((uint64_t)(uintptr_t)b.send[r]), d.str(",");
  d.f("recv", (const void*)b.recv), d.f("bytes", b.bytes), d.f("part", b.part), d.f("mode", b.mode), d.f("root", b.root);
  d.f("elementwise", b.elementwise), d.f("pad", b.pad);
  d.endLine();
}

// what planning passed out to findSymWindow / regLookup / regCovers / tunerPick (plan_stubs.h onCall)
static void dumpCall(const char* what, uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t e, uint64_t f) {
  if (gDump.mode == DUMP_OFF) return;
  Dump& dd = gDump;
  dd.str(" C "), dd.str(what);
  dd.f("a", a), dd.f("b", b), dd.f("c", c), dd.f("d", d), dd.f("e", e), dd.f("f", f);
  dd.endLine();
}

// "result=... kind=... opCount=..." closes a dumped op or group
static void dumpResult(ncclResult_t r, const ncclComm& comm) {
  if (gDump.mode == DUMP_OFF) return;
  gDump.f("result", (int)r), gDump.f("kind", gStubs.kind), gDump.f("opCount", comm.opCount);
  gDump.endLine();
}

// ---- drivers' communicator and ops ----
// A fake symmetric window over every address the drivers use, with fixed fake peer pointers
static ncclWindow_vidmem gWindow;
static void setWindow(ncclComm& comm, bool on) {
  comm.windows.clear();
  if (!on) return;
  memset(&gWindow, 0, sizeof(gWindow));
  gWindow.comm = &comm;
  gWindow.userPtr = (void*)0x1000;
  gWindow.size = (size_t)1 << 60;
  gWindow.flags = NCCL_WIN_COLL_SYMMETRIC;
  for (int r = 0; r < NCCL_AMD_MAX_RANKS; r++) {
    gWindow.peerPtr[r] = (char*)((uintptr_t)(r + 1) << 52);
    gWindow.peerSize[r] = gWindow.size;
  }
  comm.windows.push_back(&gWindow);
}

static void initComm(ncclComm& comm, int n, int rank, int chanCap) {
  stubComm(comm, n, rank, 0, chanCap);
  // PLAN_MULTIPROCESS=1: the peers live in other processes, every one serving registrations (init.cc)
  comm.multiProcess = comm.regIpcAll = getenv("PLAN_MULTIPROCESS") && atoi(getenv("PLAN_MULTIPROCESS"));
  resolveLinkChannels(&comm.tune, n, getenv("NCCL_MAX_CTAS") != nullptr);
}

// PLAN_GEOMETRY=1: what commDefaults (init.cc) takes from the environment for the communicator's shape, so that a plan
// printed here is the plan of a communicator created under the same variables
static void envGeometry(ncclComm& comm, int n) {
  if (getenv("PLAN_WINDOW") && atoi(getenv("PLAN_WINDOW"))) setWindow(comm, true);
  if (!getenv("PLAN_GEOMETRY") || !atoi(getenv("PLAN_GEOMETRY"))) return;
  auto envInt = [](const char* name, int64_t dflt) -> int64_t {
    const char* v = getenv(name);
    return v && *v ? strtoll(v, nullptr, 0) : dflt;
  };
  comm.minCTAs = (int)envInt("NCCL_MIN_CTAS", envInt("NCCL_MIN_NCHANNELS", 1));
  comm.maxCTAs = (int)envInt("NCCL_MAX_CTAS", envInt("NCCL_MAX_NCHANNELS", 256));
  comm.maxCTAs = std::max(1, std::min(comm.maxCTAs, NCCL_AMD_MAX_CHANNELS));
  comm.minCTAs = std::max(1, std::min(comm.minCTAs, comm.maxCTAs));
  comm.maxChannels = comm.maxCTAs;
  comm.chanCap = std::min(comm.chanCap, comm.maxChannels);
  resolveLinkChannels(&comm.tune, n, getenv("NCCL_MAX_CTAS") != nullptr || getenv("NCCL_MAX_NCHANNELS") != nullptr);
  comm.nSlots = std::max<int>(1, (int)envInt("NCCL_AMD_NSLOTS", 2));
  int64_t sb = (envInt("NCCL_AMD_STAGING_MIB", 1024) << 20) / ((int64_t)comm.maxChannels * 2 * comm.nSlots * (n > 1 ? n : 2));
  sb = std::max<int64_t>(16 << 10, std::min<int64_t>(sb, 1 << 20));
  if (int64_t buff = envInt("NCCL_BUFFSIZE", 0)) sb = buff / comm.nSlots;
  sb = envInt("NCCL_AMD_SLOT_BYTES", sb);
  comm.slotBytes = (size_t)std::max<int64_t>(4096, (sb + 4095) / 4096 * 4096);
}

static CollFunc funcOf(const char* f) {
  return !strcmp(f, "rs") ? FUNC_REDUCESCATTER : !strcmp(f, "ag") ? FUNC_ALLGATHER : !strcmp(f, "reduce") ? FUNC_REDUCE
       : !strcmp(f, "bcast") ? FUNC_BROADCAST : !strcmp(f, "a2a") ? FUNC_SYM_ALLTOALL : !strcmp(f, "gather") ? FUNC_SYM_GATHER
                                                                                                            : FUNC_ALLREDUCE;
}

// the group.cc loop over "FUNC:DTYPE:COUNT[:OP[:ROOT[:INPLACE]]]" specs: plan in order, extend the open run while
// batchable, else launch it. "flags:N" sets the protoFlags, "stream:N" the stream of the ops that follow.
static ncclResult_t runBatch(ncclComm& comm, int nSpecs, const char* const* specs, bool* badSpec = nullptr) {
  std::vector<PlannedColl> run;
  hipStream_t stream = nullptr;
  if (badSpec) *badSpec = false;
  for (int i = 0; i < nSpecs; i++) {
    char fn[16] = {};
    int dtype = 7, op = 0, root = 0, inPlace = 0;
    unsigned long long cnt = 0;
    const int fields = sscanf(specs[i], "%15[^:]:%d:%llu:%d:%d:%d", fn, &dtype, &cnt, &op, &root, &inPlace);
    if (fields >= 2 && !strcmp(fn, "flags")) {
      comm.tune.protoFlags = dtype;
      continue;
    }
    if (fields >= 2 && !strcmp(fn, "stream")) {
      stream = (hipStream_t)(uintptr_t)dtype;
      continue;
    }
    if (fields < 3) {
      if (badSpec) *badSpec = true;
      return ncclInvalidArgument;
    }
    PlannedColl pc;
    memset(&pc.info, 0, sizeof(pc.info));
    pc.info.func = funcOf(fn);
    pc.info.opName = specs[i];
    pc.info.sendbuff = (const void*)(0x10000000ull * (i + 4));
    pc.info.recvbuff = inPlace ? (void*)pc.info.sendbuff : (void*)(0x10000000ull * (i + 4) + 0x8000000ull);
    pc.info.count = cnt;
    pc.info.datatype = (ncclDataType_t)dtype;
    pc.info.op = (ncclRedOp_t)op;
    pc.info.root = root;
    pc.info.comm = &comm;
    pc.info.stream = stream;
    NCCLCHECK(planColl(pc.info, pc.p, pc.sp, &pc.kind));
    if (!batchable(run, pc)) {
      if (!run.empty()) NCCLCHECK(launchBatch(run));
      run.clear();
    }
    run.push_back(pc);
  }
  if (!run.empty()) NCCLCHECK(launchBatch(run));
  return ncclSuccess;
}

// ---- the sweep ----
struct EnvVar {
  const char* name;
  const char* value;
};
struct SweepConfig {
  const char* name;
  std::vector<EnvVar> env;
  bool window = false;
  int tunerAlgo = -1, tunerNch = 0;
  bool shared = false;  // the communicator shares its GPU with other ranks of the process (internal stream)
  bool bounce = false, capturing = false, regCovers = false, hostMemory = false;  // plan_stubs.h switches
  bool refuse = false;  // launchPlan / launchSymPlan fail: what the issuing code does with a failed launch
  bool allLimits = false;  // every (chanCap, minCTAs, nSlots) row below, not the first and the last alone
  bool fullCross = false;  // every (operator, offset, in place, rank, root) combination, not the four mixes
};
struct Limits {
  int chanCap, minCTAs, nSlots, maxChannels;
};
static const Limits kLimits[] = {{256, 1, 2, 256}, {16, 4, 2, 256}, {256, 4, 1, 256}, {16, 1, 1, 8}, {3, 1, 1, 256}};
static const char* const kSweepEnv[] = {
    "NCCL_PROTO", "NCCL_ALGO", "NCCL_AMD_REF_ORDER", "NCCL_AMD_REF_NCHANNELS", "NCCL_BUFFSIZE", "NCCL_AMD_LL128",
    "NCCL_AMD_LL_CHANNEL_BYTES", "NCCL_AMD_MIN_CHANNEL_BYTES", "NCCL_AMD_FORCE_ELEMENTWISE", "NCCL_AMD_P2P_FENCE",
    "NCCL_AMD_EAGER_REGISTER", "PLAN_MULTIPROCESS", "NCCL_AMD_SYM_ONESHOT", "NCCL_AMD_SYM_DISABLE", "NCCL_AMD_SYM_A2A",
    "NCCL_AMD_NO_AGGREGATION", "NCCL_MAX_CTAS", "NCCL_AMD_LINK_CHANNELS", "NCCL_AMD_EAGER_REGISTER_BYTES",
    "NCCL_AMD_LL_BYTES", "NCCL_AMD_LL128_BYTES", "NCCL_AMD_ONESHOT_BYTES", "NCCL_AMD_SIZE_TABLE", "NCCL_AMD_PROTO_FLAGS",
    "NCCL_AMD_ONESHOT_CHANNEL_BYTES", "NCCL_AMD_LL128_CHANNEL_BYTES", "NCCL_LL_BUFFSIZE", "NCCL_LL128_BUFFSIZE",
    "NCCL_AMD_AG_PULL", "NCCL_AMD_RS_PULL", "NCCL_AMD_SYM_WT", "NCCL_CHECK_POINTERS", "NCCL_AMD_HOST_COPY_GRID",
    "NCCL_AMD_COPY_GRID", "NCCL_AMD_COPY_VARIANT", "NCCL_AMD_COPY_XCD_SHIFT", "NCCL_GRAPH_REGISTER"};

static std::vector<SweepConfig> sweepConfigs() {
  std::vector<SweepConfig> c;
  auto add = [&](const char* name, std::vector<EnvVar> env) -> SweepConfig& {
    c.push_back({name, env});
    return c.back();
  };
  SweepConfig& base = add("unset", {});
  base.allLimits = base.fullCross = true;
  add("proto-ll", {{"NCCL_PROTO", "LL"}});
  add("proto-ll128", {{"NCCL_PROTO", "LL128"}});
  add("proto-simple", {{"NCCL_PROTO", "Simple"}}).allLimits = true;
  add("proto-not-ll", {{"NCCL_PROTO", "^LL"}});
  add("algo-ring", {{"NCCL_ALGO", "RING"}}).allLimits = true;
  add("algo-tree", {{"NCCL_ALGO", "TREE"}}).allLimits = true;
  add("algo-oneshot", {{"NCCL_ALGO", "ONESHOT"}});
  add("algo-direct", {{"NCCL_ALGO", "DIRECT"}});
  add("ring-ll", {{"NCCL_ALGO", "RING"}, {"NCCL_PROTO", "LL"}});
  add("ring-ll128", {{"NCCL_ALGO", "RING"}, {"NCCL_PROTO", "LL128"}});
  add("no-algo", {{"NCCL_ALGO", "NVLS"}});
  add("no-proto-per-func", {{"NCCL_ALGO", "allreduce:PAT;reduce:tree,ring"}});
  add("ref-order", {{"NCCL_AMD_REF_ORDER", "1"}}).allLimits = true;
  add("ref-order-ll", {{"NCCL_AMD_REF_ORDER", "1"}, {"NCCL_PROTO", "LL"}});
  add("ref-order-k4", {{"NCCL_AMD_REF_ORDER", "1"}, {"NCCL_AMD_REF_NCHANNELS", "4"}});
  add("ref-order-k100", {{"NCCL_AMD_REF_ORDER", "1"}, {"NCCL_AMD_REF_NCHANNELS", "100"}});
  add("ref-order-ring", {{"NCCL_AMD_REF_ORDER", "1"}, {"NCCL_ALGO", "RING"}});
  add("buffsize", {{"NCCL_BUFFSIZE", "65536"}, {"NCCL_ALGO", "RING"}});
  add("buffsize-ref", {{"NCCL_BUFFSIZE", "65536"}, {"NCCL_AMD_REF_ORDER", "1"}});
  add("ll128", {{"NCCL_AMD_LL128", "1"}});
  add("ll-channel-8", {{"NCCL_AMD_LL_CHANNEL_BYTES", "8"}});
  add("min-channel-1", {{"NCCL_AMD_MIN_CHANNEL_BYTES", "1"}});
  add("min-channel-4096", {{"NCCL_AMD_MIN_CHANNEL_BYTES", "4096"}});
  add("elementwise", {{"NCCL_AMD_FORCE_ELEMENTWISE", "1"}});
  add("no-fence", {{"NCCL_AMD_P2P_FENCE", "0"}});
  add("eager", {{"NCCL_AMD_EAGER_REGISTER", "1"}}).allLimits = true;
  add("eager-multiprocess", {{"PLAN_MULTIPROCESS", "1"}, {"NCCL_AMD_EAGER_REGISTER", "-1"}});
  add("eager-min-channel-1", {{"NCCL_AMD_EAGER_REGISTER", "1"}, {"NCCL_AMD_MIN_CHANNEL_BYTES", "1"}});
  add("link-channels-0", {{"NCCL_AMD_LINK_CHANNELS", "0"}});
  add("eager-link-channels-0", {{"NCCL_AMD_EAGER_REGISTER", "1"}, {"NCCL_AMD_LINK_CHANNELS", "0"}});
  add("ref-order-link-channels-0", {{"NCCL_AMD_REF_ORDER", "1"}, {"NCCL_AMD_LINK_CHANNELS", "0"}});
  add("eager-bounce", {{"NCCL_AMD_EAGER_REGISTER", "1"}}).bounce = true;
  add("shared-gpu", {}).shared = true;
  add("host-memory", {}).hostMemory = true;
  add("launch-refused", {}).refuse = true;
  SweepConfig& wr = add("window-launch-refused", {});
  wr.window = wr.refuse = true;
  SweepConfig& w = add("window", {});
  w.window = w.allLimits = w.fullCross = true;
  add("window-oneshot", {{"NCCL_AMD_SYM_ONESHOT", "1"}}).window = true;
  add("window-disable", {{"NCCL_AMD_SYM_DISABLE", "1"}}).window = true;
  add("window-no-a2a", {{"NCCL_AMD_SYM_A2A", "0"}}).window = true;
  add("window-min-channel-1", {{"NCCL_AMD_MIN_CHANNEL_BYTES", "1"}}).window = true;
  add("window-elementwise", {{"NCCL_AMD_FORCE_ELEMENTWISE", "1"}}).window = true;
  add("window-ring", {{"NCCL_ALGO", "RING"}}).window = true;
  add("window-link-channels-0", {{"NCCL_AMD_LINK_CHANNELS", "0"}}).window = true;
  SweepConfig& ws = add("window-shared-gpu", {});
  ws.window = ws.shared = true;
  static const struct { const char* name; int algo, nch; } tuners[] = {
      {"tuner-oneshot-0", TUNE_ONESHOT, 0}, {"tuner-direct-12", TUNE_DIRECT, 12}, {"tuner-ll-3", TUNE_LL, 3},
      {"tuner-ll128-5", TUNE_LL128, 5}, {"tuner-default-7", TUNE_DEFAULT, 7}};
  static std::string names[10];
  for (int w2 = 0; w2 < 2; w2++)
    for (int t = 0; t < 5; t++) {
      names[w2 * 5 + t] = std::string(tuners[t].name) + (w2 ? "-window" : "");
      SweepConfig& s = add(names[w2 * 5 + t].c_str(), {{"NCCL_AMD_LL128", t == 3 ? "1" : "0"}});
      s.window = w2, s.tunerAlgo = tuners[t].algo, s.tunerNch = tuners[t].nch, s.allLimits = !w2;
    }
  add("tuner-direct-12-eager", {{"NCCL_AMD_EAGER_REGISTER", "1"}});
  c.back().tunerAlgo = TUNE_DIRECT, c.back().tunerNch = 12;
  // what the plugin is told about the buffers (regBuff): registered, captured with and without NCCL_GRAPH_REGISTER
  add("tuner-default-7-registered", {});
  c.back().tunerAlgo = TUNE_DEFAULT, c.back().tunerNch = 7, c.back().regCovers = true;
  add("tuner-default-7-capture", {});
  c.back().tunerAlgo = TUNE_DEFAULT, c.back().tunerNch = 7, c.back().capturing = true;
  add("tuner-default-7-capture-no-graph-register", {{"NCCL_GRAPH_REGISTER", "0"}});
  c.back().tunerAlgo = TUNE_DEFAULT, c.back().tunerNch = 7, c.back().capturing = true;
  return c;
}

// One element on either side of every byte boundary the planner tests for this communicator, and the fixed counts
static std::vector<uint64_t> sweepCounts(const ncclComm& comm, int ts, bool fullGrid) {
  const int n = comm.nRanks;
  const CommTuning& t = comm.tune;
  const uint64_t epp = 16 / ts, area = (uint64_t)comm.llChannels * comm.llBytes;
  std::vector<uint64_t> bytes = {(uint64_t)t.tableLL[n], (uint64_t)t.tableLL128[n], (uint64_t)t.tableOneShot[n],
                                 (uint64_t)comm.slotBytes, (uint64_t)comm.slotBytes * n, area, area / 2, area / 64 * 56,
                                 (uint64_t)t.eagerBytes, (uint64_t)t.eagerBytes / n, (uint64_t)t.minChannelBytes * n,
                                 (uint64_t)t.oneShotChannelBytes * 32};
  // ringParts' channel-shrink thresholds (Simple, LL, LL128), where the reference's partition can be planned
  const bool ringParts = fullGrid || t.refOrder || t.fn[FUNC_ALLREDUCE].algo == FORCE_RING;
  for (uint64_t nc : {2, 4, 16, 64}) {
    if (!ringParts) break;
    bytes.push_back(nc * 512 * 64);
    bytes.push_back(nc * 512 * 8 * n);
    bytes.push_back(nc * 640 * 8);
  }
  std::vector<uint64_t> counts = {1, epp - 1, epp, epp + 1, n * epp - 1, n * epp + 1, ((uint64_t)256 << 20) / ts,
                                  ((uint64_t)1 << 32) + 5};
  for (uint64_t b : bytes)
    for (uint64_t c : {b / ts - 1, b / ts, b / ts + 1}) counts.push_back(c);
  std::sort(counts.begin(), counts.end());
  counts.erase(std::unique(counts.begin(), counts.end()), counts.end());
  counts.erase(std::remove_if(counts.begin(), counts.end(), [](uint64_t c) { return c == 0 || c > ((uint64_t)1 << 33); }),
               counts.end());
  return counts;
}

static const ncclDataType_t kTypeOfSize[9] = {ncclInt8, ncclInt8, ncclFloat16, ncclInt8, ncclFloat32,
                                              ncclInt8, ncclInt8, ncclInt8,    ncclFloat64};
static const char* const kFuncNames[] = {"ar", "rs", "ag", "reduce", "bcast", "a2a", "gather"};
static uint64_t gPlans = 0;

// one op through launchColl, dumped
static void sweepCase(ncclComm& comm, CollFunc func, int ts, uint64_t count, int opSel, size_t off, bool inPlace, int root) {
  const int n = comm.nRanks;
  CollInfo info;
  memset(&info, 0, sizeof(info));
  info.func = func;
  info.opName = kFuncNames[func];
  const uintptr_t send = ((uintptr_t)1 << 44) + off, recv = ((uintptr_t)1 << 45) + off;
  const uint64_t block = count * (uint64_t)ts * (uint64_t)comm.rank;
  info.sendbuff = (const void*)send;
  info.recvbuff = (void*)recv;
  if (inPlace) {  // as the reference defines in place for each collective
    if (func == FUNC_REDUCESCATTER) info.recvbuff = (void*)(send + block);
    else if (func == FUNC_ALLGATHER) info.sendbuff = (const void*)(recv + block);
    else info.recvbuff = (void*)send;
  }
  info.count = count;
  info.datatype = kTypeOfSize[ts];
  // opSel 0 sum, 1 avg, 2 the user PreMulSum operator of this type, 3 one of another type (refused)
  const int tsIx = ts == 1 ? 0 : ts == 2 ? 1 : ts == 4 ? 2 : 3;
  info.op = opSel == 0 ? ncclSum : opSel == 1 ? ncclAvg : (ncclRedOp_t)(ncclNumOps + (opSel == 2 ? tsIx : (tsIx + 1) % 4));
  info.root = root;
  info.comm = &comm;
  info.stream = (hipStream_t)0x7000;
  comm.opCount = 0;
  gStubs.kind = -1;
  if (gDump.mode != DUMP_OFF) {
    Dump& d = gDump;
    d.str("case");
    d.f("ts", ts), d.f("count", count), d.f("op", opSel), d.f("off", (uint64_t)off), d.f("inplace", inPlace);
    d.f("rank", comm.rank), d.f("root", root);
    // what the AlltoAll / Gather entry points ask before they record the op as a collective (p2p.cc)
    if (func >= FUNC_SYM_ALLTOALL) {
      const size_t B = count * (size_t)ts;
      d.f("eligible", symA2AEligible(&comm, info.sendbuff, func == FUNC_SYM_GATHER ? B : B * (size_t)n, count));
    }
    d.endLine();
  }
  const ncclResult_t r = launchColl(info);
  dumpResult(r, comm);
  gPlans++;
}

static void sweepFunc(const SweepConfig& cfg, int li, int n, CollFunc func, ncclComm* comms /* rank 0, rank n-1 */) {
  if (gDump.mode == DUMP_PRINT) printf("== %s/L%d n=%d %s\n", cfg.name, li, n, kFuncNames[func]);
  const bool rooted = func == FUNC_REDUCE || func == FUNC_BROADCAST || func == FUNC_SYM_GATHER;
  const bool folds = func == FUNC_ALLREDUCE || func == FUNC_REDUCESCATTER || func == FUNC_REDUCE;
  for (int ts : {1, 2, 4, 8}) {
    if (func == FUNC_BROADCAST && ts != 1) continue;  // (its callers normalise the datatype to bytes)
    for (uint64_t count : sweepCounts(comms[0], ts, cfg.fullCross)) {
      if (cfg.fullCross && li == 0) {
        for (int op = 0; op < (folds ? 3 : 1); op++)
          for (size_t off : {(size_t)0, (size_t)4})
            for (int inPlace = 0; inPlace < 2; inPlace++)
              for (int rk = 0; rk < 2; rk++)
                for (int rt = 0; rt < (rooted ? 2 : 1); rt++)
                  sweepCase(comms[rk], func, ts, count, op, off, inPlace, rt ? n / 2 : 0);
      } else {  // four mixes: every value of every dimension, not every combination
        sweepCase(comms[0], func, ts, count, 0, 0, false, 0);
        sweepCase(comms[1], func, ts, count, folds ? 1 : 0, 4, false, n / 2);
        sweepCase(comms[1], func, ts, count, folds ? 2 : 0, 0, true, 0);
        sweepCase(comms[0], func, ts, count, 0, 4, true, n / 2);
      }
    }
    if (folds && cfg.fullCross) sweepCase(comms[0], func, ts, 1000, 3, 0, false, 0);  // operator of another type
  }
}

static void sweepComm(ncclComm& comm, const SweepConfig& cfg, const Limits& L, int n, int rank) {
  initComm(comm, n, rank, L.chanCap);
  comm.minCTAs = L.minCTAs;
  comm.nSlots = L.nSlots;
  comm.maxChannels = L.maxChannels;
  comm.counters = (uint64_t*)0x2000;
  comm.tunerLoaded = cfg.tunerAlgo >= 0;
  comm.sharedDevInProcess = cfg.shared;
  comm.internalStream = (hipStream_t)0x9000;
  // a multi-process or capturing communicator has an fd server: its launches reach noteLaunch's capture check
  comm.fdServer = comm.multiProcess || cfg.capturing ? (FdServer*)0x10 : nullptr;
  gStubs.tunerAlgo = cfg.tunerAlgo, gStubs.tunerNch = cfg.tunerNch;
  gStubs.bounce = cfg.bounce, gStubs.regCoversAnswer = cfg.regCovers, gStubCapturing = cfg.capturing;
  gStubHostMemory = cfg.hostMemory;
  gStubs.refuseLaunch = gStubs.refuseSymLaunch = cfg.refuse;
  comm.userOps.clear();
  for (int k = 0; k < 4; k++)  // one PreMulSum operator per element size; the 4-byte one with a device scalar
    comm.userOps.push_back({true, kTypeOfSize[1 << k], DEV_PREMULSUM, 0x3c003c00ull + k, k == 2 ? (const void*)0x7700 : nullptr});
  comm.userOps.push_back({true, ncclFloat32, DEV_PREMULSUM, 0x3c003c02ull, nullptr});  // the 4-byte one, immediate scalar
  setWindow(comm, cfg.window);
}

// the batch groups (batch mode's syntax), dumped under a few configurations
static void sweepBatches() {
  static const char* const many64[] = {
      "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64",
      "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64",
      "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64",
      "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64", "ar:7:64"};
  static const std::vector<std::vector<const char*>> groups = {
      {"ar:7:100:0", "rs:7:64:0", "ag:7:64", "reduce:7:100:0:1", "ar:7:100:2", "ar:7:100:7", "rs:7:64:7"},
      {"ag:7:64", "ag:7:128", "ar:7:100:4", "rs:7:64:4", "ar:7:100:0"},
      {"ar:7:100:0", "ag:7:64", "ar:7:100:3", "ag:7:64"},
      {"bcast:0:1000:0:0", "bcast:0:2000:0:1", "bcast:0:3000:0:0", "ar:0:100", "bcast:0:8"},
      std::vector<const char*>(many64, many64 + 40),
      {"ar:7:4194304", "ar:7:4194304", "ar:7:4194304", "ar:7:4194304", "ar:7:4194304", "ar:7:4194304", "ar:7:4194304",
       "ar:7:4194304", "ar:7:4194304", "ar:7:4194305"},
      {"ar:7:65536", "ar:7:65536", "ar:7:65537", "rs:7:1048576", "rs:7:1048576", "ag:7:1048576", "ag:7:1048577",
       "reduce:7:1048576:0:1", "reduce:7:1048576:0:0", "bcast:0:1048576:0:1", "bcast:0:1048576:0:0"},
      {"ar:7:4194304", "flags:17", "ar:7:4194304", "ar:7:4194304"},
      {"ar:7:100", "ar:6:100", "ar:6:100", "ar:7:4194304", "ar:7:100"},
      {"ar:7:50000", "ar:7:50000", "rs:7:14000", "ar:7:1000", "ar:7:50000"},
      {"ar:7:30000", "ar:7:30000", "ar:7:30000", "ar:7:30000", "ar:7:30000", "ar:7:30000"},
      {"ar:7:4194304"},
      {"ar:7:100"},
      // an op that may run zero-copy (window, eager registration) after and before LL and staged ops, and alone
      {"ar:7:100", "ar:7:4194304", "reduce:7:1048576:0:1", "ar:7:4194304", "ar:7:4194304", "ar:7:100", "rs:7:1048576",
       "bcast:0:4194304:0:1", "ag:7:1048576"},
      {"rs:7:4194304"},
      // ops that plan to nothing on one rank (an in-place Broadcast) among ops that launch
      {"ar:7:100", "bcast:0:1000:0:0:1", "bcast:0:1000:0:0:1", "ar:7:100", "ar:7:100", "bcast:0:1000:0:0:1"},
      {"bcast:0:64:0:0:1"},
      // what else ends a run: another stream, operators that differ in the scalar's place alone
      {"ar:7:100", "ar:7:100", "stream:4096", "ar:7:100", "ar:7:4194304", "stream:8192", "ar:7:4194304"},
      {"ar:7:100:7", "ar:7:100:9", "ar:7:100:9", "ar:7:4194304:9", "ar:7:4194304:7", "ar:7:100:2", "ar:7:100:3",
       "ar:7:4194304:2", "ar:7:4194304:3"}};
  static const SweepConfig cfgs[] = {{"unset", {}},
                                     {"proto-simple", {{"NCCL_PROTO", "Simple"}}},
                                     {"ll-channel-8", {{"NCCL_AMD_LL_CHANNEL_BYTES", "8"}}},
                                     {"ll128", {{"NCCL_AMD_LL128", "1"}}},
                                     {"no-aggregation", {{"NCCL_AMD_NO_AGGREGATION", "1"}}},
                                     {"ref-order", {{"NCCL_AMD_REF_ORDER", "1"}}},
                                     {"algo-ring", {{"NCCL_ALGO", "RING"}}},
                                     {"window", {}, true},
                                     {"eager", {{"NCCL_AMD_EAGER_REGISTER", "1"}}},
                                     {"eager-bounce", {{"NCCL_AMD_EAGER_REGISTER", "1"}}, false, -1, 0, false, true},
                                     {"shared-gpu", {}, false, -1, 0, true},
                                     {"window-shared-gpu", {}, true, -1, 0, true},
                                     {"window-no-aggregation", {{"NCCL_AMD_NO_AGGREGATION", "1"}}, true},
                                     {"tuner-direct-12-capture", {}, false, TUNE_DIRECT, 12, false, false, true},
                                     {"launch-refused", {}, false, -1, 0, false, false, false, false, false, true},
                                     {"window-launch-refused", {}, true, -1, 0, false, false, false, false, false, true}};
  for (const SweepConfig& cfg : cfgs) {
    for (const char* v : kSweepEnv) unsetenv(v);
    for (const EnvVar& e : cfg.env) setenv(e.name, e.value, 1);
    for (int n : {1, 2, 4, 8}) {
      std::string line;
      // channel caps 256 and 16, and 16 with 8 channels allocated (the grid check refuses inside a group)
      for (int row = 0; row < 3; row++) {
        const int chanCap = row == 0 ? 256 : 16;
        gDump.hash = 14695981039346656037ull;
        if (gDump.mode == DUMP_PRINT) printf("== batch %s n=%d cap=%d row=%d\n", cfg.name, n, chanCap, row);
        ncclComm comm;
        sweepComm(comm, cfg, {chanCap, 1, 2, row == 2 ? 8 : 256}, n, n - 1);
        for (const auto& g : groups) {
          gStubs.kind = -1;
          const int flags = comm.tune.protoFlags;
          const ncclResult_t r = runBatch(comm, (int)g.size(), g.data());
          comm.tune.protoFlags = flags;
          dumpResult(r, comm);
          gPlans += g.size();
        }
        char h[40];
        snprintf(h, sizeof(h), " %s=%016llx", row == 0 ? "cap256" : row == 1 ? "cap16" : "cap16of8", (unsigned long long)gDump.hash);
        line += h;
      }
      if (gDump.mode == DUMP_HASH) printf("batch/%s n=%d groups=%zu%s\n", cfg.name, n, groups.size(), line.c_str());
    }
  }
}

static void sweepAll() {
  const std::vector<SweepConfig> cfgs = sweepConfigs();
  const int nLimits = (int)(sizeof(kLimits) / sizeof(kLimits[0]));
  for (const SweepConfig& cfg : cfgs) {
    for (const char* v : kSweepEnv) unsetenv(v);
    for (const EnvVar& e : cfg.env) setenv(e.name, e.value, 1);
    // one digest line per (configuration, rank count), a hash per collective over the configuration's limits rows
    for (int n : {1, 2, 3, 4, 5, 8}) {
      const uint64_t plansN = gPlans;
      std::string line;
      for (int f = 0; f <= FUNC_SYM_GATHER; f++) {
        // the zero-copy AlltoAll / Gather: with the window, and once without (the window gone since the call)
        if (f >= FUNC_KINDS && !cfg.window && strcmp(cfg.name, "unset")) continue;
        gDump.hash = 14695981039346656037ull;
        for (int li = 0; li < nLimits; li++) {
          if (!cfg.allLimits && li != 0 && li != nLimits - 1) continue;
          ncclComm comms[2];
          sweepComm(comms[0], cfg, kLimits[li], n, 0);
          sweepComm(comms[1], cfg, kLimits[li], n, n - 1);
          sweepFunc(cfg, li, n, (CollFunc)f, comms);
        }
        char h[40];
        snprintf(h, sizeof(h), " %s=%016llx", kFuncNames[f], (unsigned long long)gDump.hash);
        line += h;
      }
      if (gDump.mode == DUMP_HASH)
        printf("%s n=%d cases=%llu%s\n", cfg.name, n, (unsigned long long)(gPlans - plansN), line.c_str());
    }
  }
  sweepBatches();
  gStubs.tunerAlgo = -1, gStubs.bounce = gStubs.regCoversAnswer = gStubCapturing = gStubHostMemory = false;
  gStubs.refuseLaunch = gStubs.refuseSymLaunch = false;
  for (const char* v : kSweepEnv) unsetenv(v);
}

// one line per plan: what reached launchPlan / launchSymPlan last
static void printPlan() {
  if (gStubs.kind == 1) {
    const SymPlan& s = gStubs.sym;
    printf("algo=sym nch=%d part=%lu slice=0 steps=1 chunk=%lu symcoll=%d\n", s.nChannels, (unsigned long)s.args.part,
           (unsigned long)s.args.chunk, s.coll);
    return;
  }
  const char* pipes[] = {"ring", "ring", "ring", "chain", "chain"};
  const LaunchPlan& p = gStubs.plan;
  if (p.algo == ALGO_PIPE) {
    const unsigned sub = p.args.refSub ? p.args.refSub : 1;
    printf("algo=%s kind=%d nch=%d part=%lu slice=%lu steps=%d chunk=%lu cbdlo=%lu cbdhi=%lu refnch=%d sub=%u\n",
           pipes[p.pipeKind], p.pipeKind, p.nChannels, (unsigned long)p.args.part, (unsigned long)p.args.slice,
           p.args.nSteps, (unsigned long)p.args.chunk, (unsigned long)p.args.cbdLo, (unsigned long)p.args.cbdHi,
           p.nChannels / (int)sub, sub);
    return;
  }
  if (p.algo == ALGO_LL)
    printf("algo=%s nch=%d part=%lu slice=0 steps=1 chunk=%lu\n", p.ll.ops[0].proto == LLP_LL64 ? "ll128" : "ll",
           p.nChannels, (unsigned long)p.ll.ops[0].part,
           (unsigned long)p.ll.ops[0].chunk);
  else
    printf("algo=%s nch=%d part=%lu slice=%lu steps=%d chunk=%lu cbdlo=%lu cbdhi=%lu refnch=%d sub=%u\n",
           kAlgoNames[p.algo], p.nChannels, (unsigned long)p.args.part, (unsigned long)p.args.slice, p.args.nSteps,
           (unsigned long)p.args.chunk, (unsigned long)p.args.cbdLo, (unsigned long)p.args.cbdHi,
           p.nChannels / (int)(p.args.refSub ? p.args.refSub : 1), p.args.refSub ? p.args.refSub : 1);
}

int main(int argc, char** argv) {
  gStubs.onLaunch = dumpLaunchPlan;
  gStubs.onSymLaunch = dumpSymPlan;
  gStubs.onCall = dumpCall;
  if (argc >= 2 && (!strcmp(argv[1], "sweep") || !strcmp(argv[1], "sweep-full"))) {
    gDump.mode = !strcmp(argv[1], "sweep") ? DUMP_HASH : DUMP_PRINT;
    sweepAll();
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "sweep-time")) {
    const int reps = argc > 2 ? atoi(argv[2]) : 1;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int i = 0; i < reps; i++) sweepAll();
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double s = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    printf("plans=%llu seconds=%.3f plans_per_second=%.0f\n", (unsigned long long)gPlans, s, (double)gPlans / s);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "peers")) {
    // the kernels' per-channel peer order (device_abi.h chanPeer): one line "me c p(1) ... p(n-1)" per (rank, channel)
    const int n = atoi(argv[2]), K = atoi(argv[3]);
    for (int me = 0; me < n; me++)
      for (int c = 0; c < K; c++) {
        printf("%d %d", me, c);
        for (int k = 1; k < n; k++) printf(" %d", chanPeer(me, n, c, k));
        printf("\n");
      }
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "cap")) {  // the co-residency channel cap for (CUs, ranks per GPU)
    printf("%d\n", coResidentChannelCap(atoi(argv[2]), atoi(argv[3])));
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "matrix")) {
    // NCCL_ALGO / NCCL_PROTO as loadTuning resolves them: "parse=<ncclResult_t>", then one line per collective
    CommTuning t;
    loadTuning(&t);
    printf("parse=%d\n", t.parseError);
    const char* fn[] = {"allreduce", "reducescatter", "allgather", "reduce"};
    const char* force[] = {"none", "oneshot", "direct", "ring", "tree"};
    for (int f = 0; f < FUNC_COUNT; f++) {
      const FuncTuning& ft = t.fn[f];
      printf("func=%s algo=%s oneshot=%d direct=%d noalgo=%d ll=%d ll128=%d simple=%d\n", fn[f], force[ft.algo],
             ft.oneShotOk, ft.directOk, ft.noAlgo, ft.llOn, ft.ll128On, ft.simpleOn);
    }
    return 0;
  }
  const bool dump = argc >= 2 && !strcmp(argv[1], "dump");
  if (dump) {
    gDump.mode = DUMP_PRINT;
    argc--, argv++;
  }
  if (argc < 5 && !(argc == 4 && !strcmp(argv[2], "many"))) {
    fprintf(stderr, "usage: plan_test NRANKS FUNC DTYPE COUNT [ALIGN_OFFSET] [CHANCAP]\n");
    return 2;
  }
  const int n = atoi(argv[1]);
  const char* f = argv[2];
  const bool many = !strcmp(f, "many");
  const bool batch = !strcmp(f, "batch") || many;
  const int dt = batch ? 0 : atoi(argv[3]);
  const size_t count = batch ? 0 : strtoull(argv[4], nullptr, 0);
  const size_t off = !batch && argc > 5 ? strtoull(argv[5], nullptr, 0) : 0;
  ncclComm comm;
  initComm(comm, n, 0, !batch && argc > 6 ? atoi(argv[6]) : 256);
  envGeometry(comm, n);
  if (many) {
    for (int i = 3; i < argc; i++) {
      char fn[16] = {};
      int dtype = 7, root = 0;
      unsigned long long cnt = 0;
      if (sscanf(argv[i], "%15[^:]:%d:%llu:%d", fn, &dtype, &cnt, &root) < 3) return 2;
      CollInfo info;
      memset(&info, 0, sizeof(info));
      info.func = funcOf(fn);
      info.opName = argv[i];
      info.sendbuff = (const void*)0x10000000ull;
      info.recvbuff = (void*)0x20000000ull;
      info.count = cnt;
      info.datatype = (ncclDataType_t)dtype;
      info.op = ncclSum;
      info.root = root;
      info.comm = &comm;
      gStubs.kind = -1;
      const ncclResult_t r = launchColl(info);
      if (r != ncclSuccess) printf("error=%d\n", (int)r);
      else printPlan();
    }
    return 0;
  }
  if (batch) {
    if (!dump) gStubs.onLaunch = printBatchLaunch;
    bool badSpec = false;
    const ncclResult_t r = runBatch(comm, argc - 3, argv + 3, &badSpec);
    dumpResult(r, comm);
    return badSpec ? 2 : r != ncclSuccess ? 1 : 0;
  }
  CollInfo info;
  memset(&info, 0, sizeof(info));
  info.func = funcOf(f);
  info.opName = f;
  info.sendbuff = (const void*)(0x10000000ull + off);
  info.recvbuff = (void*)(0x20000000ull + off);
  info.count = count;
  info.datatype = (ncclDataType_t)dt;
  info.op = ncclSum;
  info.comm = &comm;
  info.stream = nullptr;
  ncclResult_t r = launchColl(info);
  if (dump) {
    dumpResult(r, comm);
    return r != ncclSuccess;
  }
  if (r != ncclSuccess) {
    printf("error=%d\n", (int)r);
    return 1;
  }
  printPlan();
  return 0;
}
