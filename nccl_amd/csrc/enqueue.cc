// enqueue.cc — collective entry points, argument checks, op mapping, algorithm/channel choice, launch.
//
// Reference: src/collectives.cc:129-256 (entry points build ncclInfo), src/enqueue.cc:3124-3172
// (ncclEnqueueCheck: CommCheck → implicit group → ArgsCheck → taskAppend), :3014-3122 (taskAppend:
// count==0 no-op, nRanks==1 → ncclLaunchOneRank), :2479-2583 (hostToDevRedOp), src/misc/argcheck.cc:
// 12-45, 201-254 (pointer / comm / argument checks), src/graph/tuning.cc (algorithm cost model —
// replaced by the small MI355X table in choosePlan()).
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "core.h"

namespace ncclamd {

int typeSize(ncclDataType_t t) {
  switch (t) {
    case ncclInt8: case ncclUint8: case ncclFloat8e4m3: case ncclFloat8e5m2: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return -1;
  }
}

static uint16_t hostF32ToHalf(float f);
static uint16_t hostF32ToBf16(float f);
static uint8_t hostF32ToFp8(float f, bool e5m2);

// hostToDevRedOp (reference src/enqueue.cc:2479-2583).
static ncclResult_t hostToDevRedOp(ncclComm* comm, ncclRedOp_t op, ncclDataType_t dt, int* devOp,
                                   uint64_t* arg, const void** argPtr) {
  int nbits = 8 * typeSize(dt);
  if (nbits <= 0) return ncclInvalidArgument;
  uint64_t allBits = nbits == 64 ? ~0ull : ((1ull << nbits) - 1);
  uint64_t signBit = allBits ^ (allBits >> 1);
  *arg = 0;
  *argPtr = nullptr;
  switch ((int)op) {
    case ncclSum: *devOp = DEV_SUM; return ncclSuccess;
    case ncclProd: *devOp = DEV_PROD; return ncclSuccess;
    case ncclMin:
    case ncclMax:
      *devOp = DEV_MINMAX;
      if (dt == ncclInt8 || dt == ncclInt32 || dt == ncclInt64) *arg ^= signBit;
      if (op == ncclMax) *arg ^= allBits;
      return ncclSuccess;
    case ncclAvg: {
      int n = comm->nRanks;
      switch (dt) {
        case ncclInt8: case ncclInt32: case ncclInt64:
          *devOp = DEV_SUMPOSTDIV; *arg = ((uint64_t)n << 1) | 1; return ncclSuccess;
        case ncclUint8: case ncclUint32: case ncclUint64:
          *devOp = DEV_SUMPOSTDIV; *arg = (uint64_t)n << 1; return ncclSuccess;
        case ncclFloat16: *devOp = DEV_PREMULSUM; *arg = hostF32ToHalf((float)(1.0 / n)); return ncclSuccess;
        case ncclBfloat16: *devOp = DEV_PREMULSUM; *arg = hostF32ToBf16((float)(1.0 / n)); return ncclSuccess;
        case ncclFloat8e4m3: *devOp = DEV_PREMULSUM; *arg = hostF32ToFp8((float)(1.0 / n), false); return ncclSuccess;
        case ncclFloat8e5m2: *devOp = DEV_PREMULSUM; *arg = hostF32ToFp8((float)(1.0 / n), true); return ncclSuccess;
        case ncclFloat32: { float s = (float)(1.0 / n); *devOp = DEV_PREMULSUM; memcpy(arg, &s, 4); return ncclSuccess; }
        case ncclFloat64: { double s = 1.0 / n; *devOp = DEV_PREMULSUM; memcpy(arg, &s, 8); return ncclSuccess; }
        default: return ncclInvalidArgument;
      }
    }
    default: {
      int ix = (int)op - (int)ncclNumOps;
      const UserRedOp& u = comm->userOps[ix];
      if (dt != u.datatype) {
        WARN("Data type supplied to user-created ncclRedOp_t does not match type given to reduction operation");
        return ncclInvalidArgument;
      }
      *devOp = u.devOp;
      *arg = u.scalarArg;
      *argPtr = u.scalarPtr;
      return ncclSuccess;
    }
  }
}

// ---- NCCL_ALGO / NCCL_PROTO (reference src/graph/tuning.cc:36-136 parseList, :440-462; names src/init.cc:52-55).
// "[func:]list[;func:list]...": a list of names separated by commas, or "^list" for all but those; an entry without a
// function prefix applies to every function and may only come first; names and prefixes match case-insensitively;
// an unknown name or prefix fails init with ncclInvalidUsage. The algorithm names are the reference's plus this
// engine's OneShot and Direct. One deviation: "^" re-enables the unlisted names at their DEFAULTS, where the
// reference writes 1 — the same for every name but LL128, whose default here is the engine's gate (NCCL_AMD_LL128,
// off until 64-byte lines are shown whole over xGMI), as the reference's 2 is its topology gate (tuning.cc:446,
// 518-536): naming LL128 enables it, excluding every other protocol leaves it on as the only one.
namespace {
constexpr int kRefFuncs = 5, kAlgoNames = 9, kProtoNames = 3;
enum { PROTO_LL = 0, PROTO_LL128 = 1, PROTO_SIMPLE = 2 };
enum { ALG_TREE = 0, ALG_RING = 1, ALG_ONESHOT = 7, ALG_DIRECT = 8 };
const char* const kRefFuncName[kRefFuncs] = {"Broadcast", "Reduce", "AllGather", "ReduceScatter", "AllReduce"};
const char* const kAlgoName[kAlgoNames] = {"Tree", "Ring", "CollNetDirect", "CollNetChain", "NVLS", "NVLSTree", "PAT",
                                           "OneShot", "Direct"};
const char* const kProtoName[kProtoNames] = {"LL", "LL128", "Simple"};
const int kRefFuncOf[FUNC_KINDS] = {4, 3, 2, 1, 0};  // CollFunc -> the reference's ncclFunc_t row
const char* const kForceName[] = {"", "OneShot", "Direct", "Ring", "Tree"};

// the non-empty pieces of s between separators, each with its offset (strtok_r's tokens)
std::vector<std::pair<size_t, std::string>> tokens(const std::string& s, char sep) {
  std::vector<std::pair<size_t, std::string>> out;
  for (size_t pos = 0; pos <= s.size();) {
    size_t e = s.find(sep, pos);
    if (e == std::string::npos) e = s.size();
    if (e > pos) out.push_back({pos, s.substr(pos, e - pos)});
    pos = e + 1;
  }
  return out;
}
}  // namespace

// list: [kRefFuncs][nnames] enables, holding the defaults on entry (a "^" entry restores them, see above)
static ncclResult_t parseEnableList(const char* var, const char* str, const char* const* names, int nnames, int* list) {
  std::vector<int> defaults(list, list + nnames);  // row 0 = every row's default
  for (const auto& entry : tokens(str, ';')) {
    const auto parts = tokens(entry.second, ':');
    std::string prefix, elems;
    if (parts.size() >= 2) {
      prefix = parts[0].second;
      elems = parts[1].second;
    } else if (parts.size() == 1) {
      if (entry.first != 0) {  // every function before it would be overwritten
        WARN("%s: all entries except the first must have a prefix: \"%s\"", var, str);
        return ncclInvalidUsage;
      }
      elems = parts[0].second;
    } else {
      WARN("%s: empty entry in \"%s\"", var, str);
      return ncclInvalidUsage;
    }
    const bool exclude = !elems.empty() && elems[0] == '^';
    if (exclude) elems.erase(0, 1);
    std::vector<int> row(nnames);
    for (int e = 0; e < nnames; e++) row[e] = exclude ? defaults[e] : 0;
    for (const auto& tok : tokens(elems, ',')) {
      int e = 0;
      while (e < nnames && strcasecmp(tok.second.c_str(), names[e]) != 0) e++;
      if (e == nnames) {
        WARN("%s: unrecognized element token \"%s\" when parsing \"%s\"", var, tok.second.c_str(), str);
        return ncclInvalidUsage;
      }
      row[e] = exclude ? 0 : 1;
    }
    bool found = false;
    for (int f = 0; f < kRefFuncs; f++) {
      if (!prefix.empty() && strcasecmp(prefix.c_str(), kRefFuncName[f]) != 0) continue;
      found = true;
      for (int e = 0; e < nnames; e++) list[f * nnames + e] = row[e];
    }
    if (!found) {
      WARN("%s: unrecognized prefix token \"%s\" when parsing \"%s\"", var, prefix.c_str(), str);
      return ncclInvalidUsage;
    }
  }
  return ncclSuccess;
}

// One collective's enables onto this engine's kernels. Exactly one implemented algorithm enabled (OneShot, Direct,
// Ring or Tree) forces it, as NCCL_ALGO=<name> always did here; several leave the choice to the size table, as the
// reference's cost model chooses among the enabled ones, restricted to the kernels that stand in for them in the
// tuner's cost table (tuner.cc: (TREE, SIMPLE) = one-shot, (RING, SIMPLE) = direct); none — only CollNet / NVLS /
// PAT, absent from an xGMI mesh — or no protocol leaves the collective without an algorithm (it fails, as the
// reference's does, enqueue.cc:2052-2065).
static void resolveFuncTuning(const int* algoOn, const int* protoOn, int ll128Default, FuncTuning* ft) {
  memset(ft, 0, sizeof(*ft));
  ft->llOn = protoOn[PROTO_LL] != 0;
  ft->simpleOn = protoOn[PROTO_SIMPLE] != 0;
  ft->ll128On = protoOn[PROTO_LL128] == 2 ? (ll128Default != 0 || (!ft->llOn && !ft->simpleOn))
                                          : protoOn[PROTO_LL128] != 0;
  const int one = algoOn[ALG_ONESHOT] != 0, dir = algoOn[ALG_DIRECT] != 0, ring = algoOn[ALG_RING] != 0,
            tree = algoOn[ALG_TREE] != 0;
  const int impl = one + dir + ring + tree;
  ft->algo = FORCE_NONE;
  if (impl == 1) ft->algo = one ? FORCE_ONESHOT : dir ? FORCE_DIRECT : ring ? FORCE_RING : FORCE_TREE;
  ft->oneShotOk = one || tree;
  ft->directOk = dir || ring;
  ft->noAlgo = impl == 0 || (!ft->llOn && !ft->simpleOn && !ft->ll128On);
}

void loadTuning(CommTuning* t) {
  memset(t, 0, sizeof(*t));
  t->checkPointers = (int)paramInt("NCCL_CHECK_POINTERS", 0);
  t->forceElementwise = (int)paramInt("NCCL_AMD_FORCE_ELEMENTWISE", 0);
  // Release fence (buffer_wbl2) before data flags: NCCL_AMD_P2P_FENCE=1 keeps it, =0 drops it (every byte a
  // peer reads from this rank's writes is a write-through system-scope store, drained before the flag store,
  // DESIGN.md §4). Unset (-1): dropped only when every rank shares one GPU, where that ordering has been
  // tested; kept across devices until a multi-GPU run shows the drain suffices over xGMI.
  // Resolved by resolveFence() once the peer table is known.
  t->p2pFence = (int)paramInt("NCCL_AMD_P2P_FENCE", -1);
  // Gather direction: phase C of the staged AllReduce / AllGather PULLS each owner's reduced
  // block from the owner's staging (one published copy read by every peer over its link) — the north star's
  // peer-mapped reads, and on the n = 8 rehearsal 1.585 vs 1.867 ms for the push gather
  // (profiles/r04d_scale_rehearsal_n8_onegpu.json). NCCL_AMD_AG_PULL=0 restores the push gather (n-1 remote
  // writes per reduced block). The scatter stays a push unless NCCL_AMD_RS_PULL=1 (no measured gain at n = 8).
  t->protoFlags = (int)paramInt("NCCL_AMD_PROTO_FLAGS", 0) | (t->p2pFence == 0 ? 8 : 0) |
                  (paramInt("NCCL_AMD_AG_PULL", 1) ? 16 : 0) | (paramInt("NCCL_AMD_RS_PULL", 0) ? 32 : 0);
  // NCCL_ALGO / NCCL_PROTO in the reference's grammar (parseEnableList below), one enable row per collective
  int algoOn[kRefFuncs][kAlgoNames], protoOn[kRefFuncs][kProtoNames];
  for (int f = 0; f < kRefFuncs; f++) {
    for (int a = 0; a < kAlgoNames; a++) algoOn[f][a] = 1;
    // LL128: 2 = this engine's default gate (the reference's 2 is its topology gate, tuning.cc:446, 518-536): the LL128
    // class (LL64 lines, kernels.h ll64ChannelOp) is off unless NCCL_AMD_LL128=1 or NCCL_PROTO names it, until the
    // 8-GPU suite's probe shows 64-byte lines arrive whole over xGMI
    for (int p = 0; p < kProtoNames; p++) protoOn[f][p] = p == PROTO_LL128 ? 2 : 1;
  }
  const char* protoStr = paramStr("NCCL_PROTO");
  const char* algoStr = paramStr("NCCL_ALGO");
  t->parseError = 0;
  if (protoStr && parseEnableList("NCCL_PROTO", protoStr, kProtoName, kProtoNames, &protoOn[0][0]) != ncclSuccess)
    t->parseError = ncclInvalidUsage;
  if (algoStr && parseEnableList("NCCL_ALGO", algoStr, kAlgoName, kAlgoNames, &algoOn[0][0]) != ncclSuccess)
    t->parseError = ncclInvalidUsage;
  const int ll128Default = (int)paramInt("NCCL_AMD_LL128", 0);
  for (int f = 0; f < FUNC_KINDS; f++) resolveFuncTuning(algoOn[kRefFuncOf[f]], protoOn[kRefFuncOf[f]], ll128Default, &t->fn[f]);
  if (algoStr || protoStr) {
    for (int f = 0; f < FUNC_KINDS; f++) {
      const FuncTuning& ft = t->fn[f];
      INFO("NCCL_ALGO / NCCL_PROTO: %s: %s%s, protocols LL %d LL128 %d Simple %d", kRefFuncName[kRefFuncOf[f]],
           ft.noAlgo ? "no algorithm available" : ft.algo != FORCE_NONE ? "forced " : "size table over",
           ft.noAlgo ? "" : ft.algo != FORCE_NONE ? kForceName[ft.algo]
                          : ft.oneShotOk && ft.directOk ? " one-shot, direct" : ft.oneShotOk ? " one-shot" : " direct",
           ft.llOn, ft.ll128On, ft.simpleOn);
    }
  }
  t->symDisable = (int)paramInt("NCCL_AMD_SYM_DISABLE", 0);
  // ncclAlltoAll / ncclGather whose sendbuff lies in a symmetric window pull straight from the peers' windows
  // (symA2AKernel); 0: the staged send / recv expansion whatever the buffers are
  t->symA2A = (int)paramInt("NCCL_AMD_SYM_A2A", 1);
  t->symOneShot = (int)paramInt("NCCL_AMD_SYM_ONESHOT", 0);
  // write-through publish in the symmetric kernels: n = 2 one-GPU rehearsal 0.291-0.295 -> 0.234-0.241 ms at
  // 256 MiB fp32 (no per-channel L2 write-back; profiles/r02_sym_wt_ab_onegpu.txt)
  t->symWtPublish = (int)paramInt("NCCL_AMD_SYM_WT", 1);
  // reference register.cc:16 / enqueue.cc:283 (both default on): ncclCommRegister'd buffers and, under stream
  // capture, the captured collectives' buffers run the zero-copy kernel (register.cc)
  t->localRegister = (int)paramInt("NCCL_LOCAL_REGISTER", 1);
  t->graphRegister = (int)paramInt("NCCL_GRAPH_REGISTER", 1);
  t->noAggregation = (int)paramInt("NCCL_AMD_NO_AGGREGATION", 0);
  // Eager registration (register.cc regLookup): collectives of at least eagerBytes whose staged plan would be direct
  // register their unregistered allocations on first use and run the zero-copy kernel. 1: on; -1:
  // on for communicators spanning processes whose peers all serve registrations (eagerOn; one-GPU rehearsal 2.50 S vs
  // 4.0 S of HBM per rank at n = 2 by PMC); 0 (default): off. Round 6 made its costs bounded without a blocking call
  // and added the bounce allocation and the init probe, and measured on the one-GPU n = 8 rehearsal that the runtime
  // can hand one process's export another process's fresh dma-buf (§10.3): so it stays opt-in.
  t->eagerRegister = (int)paramInt("NCCL_AMD_EAGER_REGISTER", 0);
  t->eagerBytes = paramInt("NCCL_AMD_EAGER_REGISTER_BYTES", 1 << 20);
  t->eagerMax = (int)paramInt("NCCL_AMD_EAGER_REGISTER_MAX", 64);
  if (t->eagerMax < 1) t->eagerMax = 1;
  // bytes of eager-only registrations kept (their peers map them; once the owner frees one, until the next
  // collective's upkeep finds it, that HBM stays held): the least recently used beyond it are retired
  t->eagerMaxBytes = paramInt("NCCL_AMD_EAGER_REGISTER_MAX_BYTES", (int64_t)32 << 30);
  // ncclSend / ncclRecv (p2p.cc p2pCutFor): one channel part per 128 KiB (the reference's p2p chunk), at most 32
  // channels per peer and direction — both suppositions until a multi-GPU node is measured. The
  // reference's NCCL_MIN_P2P_NCHANNELS / NCCL_MAX_P2P_NCHANNELS bound the count as they do there.
  t->p2pChunkBytes = paramInt("NCCL_AMD_P2P_CHUNK_BYTES", 128 << 10);
  if (t->p2pChunkBytes < 16) t->p2pChunkBytes = 16;
  t->p2pMinCh = (int)std::max<int64_t>(1, paramInt("NCCL_MIN_P2P_NCHANNELS", 1));
  t->p2pMaxCh = (int)std::max<int64_t>(1, paramInt("NCCL_MAX_P2P_NCHANNELS", 32));
  // the size table's ranges (per rank count; NCCL_AMD_SIZE_TABLE overrides rows, the three knobs below all rows)
  (void)loadSizeTable(t, paramStr("NCCL_AMD_SIZE_TABLE"));
  t->oneShotBytes = paramInt("NCCL_AMD_ONESHOT_BYTES", 0);  // 0: size table default (2 MiB / nRanks; 2 MiB at 2 ranks)
  t->llBytes = paramInt("NCCL_AMD_LL_BYTES", 0);  // 0: size table default (256 KiB / nRanks)
  t->llChannelBytes = paramInt("NCCL_AMD_LL_CHANNEL_BYTES", 4096);
  if (t->llChannelBytes < 8) t->llChannelBytes = 8;
  t->ll128Bytes = paramInt("NCCL_AMD_LL128_BYTES", 0);  // 0: size table default (1 MiB / nRanks)
  t->ll128ChannelBytes = paramInt("NCCL_AMD_LL128_CHANNEL_BYTES", 4096);
  if (t->ll128ChannelBytes < kLL64Payload) t->ll128ChannelBytes = kLL64Payload;
  // 16 KiB: mid-size direct AllReduces spread over more channels (one-GPU rehearsal, n = 4, 4 MiB: 51 -> 30 us,
  // profiles/r02_channel_granularity_onegpu.txt); 256 MiB plans are capped at the channel limit either way
  t->minChannelBytes = paramInt("NCCL_AMD_MIN_CHANNEL_BYTES", 16 << 10);
  t->oneShotChannelBytes = paramInt("NCCL_AMD_ONESHOT_CHANNEL_BYTES", 16 << 10);
  t->copyVariant = (int)paramInt("NCCL_AMD_COPY_VARIANT", 0);
  t->copyGrid = paramInt("NCCL_AMD_COPY_GRID", 1 << 30);
  // a copy that crosses PCIe (a pinned host send or receive buffer) is bound by the link's outstanding requests, not
  // by CUs: one workgroup per CU moves a 256 MiB host-to-host bucket in 5.37 ms against 6.28 ms for the HBM default
  // of one per tile (grid caps 64-320 within 1 %, scripts/host_direct_sweep.sh)
  t->hostCopyGrid = paramInt("NCCL_AMD_HOST_COPY_GRID", 256);
  t->copyXcdShift = (int)paramInt("NCCL_AMD_COPY_XCD_SHIFT", 6);
  // the reference's RING/SIMPLE chunk: stepSize (NCCL_BUFFSIZE / NCCL_STEPS) x ALLREDUCE_CHUNKSTEPS (NCCL_STEPS / 2),
  // in 512-byte grains (enqueue.cc:2222-2225, 2321; collectives.h:19-20; default NCCL_BUFFSIZE 4 MiB, init.cc:813)
  // NCCL_AMD_REF_ORDER=1: every AllReduce folds in the reference's RING/SIMPLE order at any size, on the fast
  // direct kernel (planColl below)
  t->refOrder = (int)paramInt("NCCL_AMD_REF_ORDER", 0);
  // the reference run's channel count for the modes that walk its partition (NCCL_AMD_REF_ORDER, NCCL_ALGO=RING):
  // 0 = the communicator's channel cap, clamped to the reference's MAXCHANNELS (refChannelCount)
  t->refChannels = (int)paramInt("NCCL_AMD_REF_NCHANNELS", 0);
  const int64_t buff = paramInt("NCCL_BUFFSIZE", 4 << 20);
  t->ringChunkBytes = buff / 8 * 4 / 512 * 512;
  if (t->ringChunkBytes < 512) t->ringChunkBytes = 512;
  // The partition REF_ORDER walks is the reference's ring partition of the protocol NCCL_PROTO names alone (LL or
  // LL128; Simple otherwise), with that protocol's chunk: stepSize = buffer / NCCL_STEPS, Simple x 4 in 512-byte
  // grains, LL / 2 in 16-byte grains, LL128 x 15/16 in 1920-byte grains (enqueue.cc:2222-2227, 2321; buffers
  // init.cc:810-827: 4 MiB, 8 x 512 x 8 x 16 B, 120 x 640 x 8 x 8 B). A chunk below one grain (which never
  // advances in the reference) is raised to one grain.
  const FuncTuning& ar = t->fn[FUNC_ALLREDUCE];
  t->refProto = ar.llOn && !ar.simpleOn && !ar.ll128On ? 0 : ar.ll128On && !ar.llOn && !ar.simpleOn ? 1 : 2;
  if (t->refProto == 2) {
    t->refChunkBytes = t->ringChunkBytes;
  } else if (t->refProto == 0) {
    t->refChunkBytes = paramInt("NCCL_LL_BUFFSIZE", 8 * 512 * 8 * 16) / 8 / 2 / 16 * 16;
    if (t->refChunkBytes < 16) t->refChunkBytes = 16;
  } else {
    t->refChunkBytes = paramInt("NCCL_LL128_BUFFSIZE", 120 * 640 * 8 * 8) / 8 / 16 * 15 / 1920 * 1920;
    if (t->refChunkBytes < 1920) t->refChunkBytes = 1920;
  }
}

// ---- the size table (reference: the per-(algorithm, protocol) latency / bandwidth tables and the cost model that
// picks the cheapest, src/graph/tuning.cc:148-212, 630-655). One node, one mesh: what the table decides here is
// where LL ends, where the LL128 class ends and where one-shot gives way to the direct kernel, per rank count.
// Built-in rows (one-GPU rehearsal crossovers): LL up to max(16 KiB, 256 KiB / n), the LL128 class
// (when enabled) up to max(64 KiB, 1 MiB / n), one-shot up to 2 MiB / n (2 MiB at n = 2). NCCL_AMD_SIZE_TABLE=<file>
// replaces rows without a rebuild, so the crossovers an 8-GPU sweep measures can be adopted as data:
//   # nranks  ll      ll128   oneshot      (bytes; K / M / G suffixes; '-' keeps the built-in value; 0 = off)
//   8         48K     -       512K
//   *         -       -       1M           ('*': every rank count; later lines override earlier ones)
// Rank 0's table is the communicator's (the tuning block is agreed at init), so every rank plans alike.
// A byte count, or -1 for '-' (keep the built-in value). 0 is a size like any other (e.g. "8 0 - -": no LL at n = 8).
static int64_t parseBytes(const char* tok, bool* ok) {
  *ok = true;
  if (!strcmp(tok, "-")) return -1;
  char* end = nullptr;
  const double v = strtod(tok, &end);
  if (end == tok || !std::isfinite(v) || v < 0) {  // 'nan' / 'inf' are malformed sizes
    *ok = false;
    return 0;
  }
  double m = 1;
  if (*end == 'k' || *end == 'K') m = 1024.0, end++;
  else if (*end == 'm' || *end == 'M') m = 1024.0 * 1024, end++;
  else if (*end == 'g' || *end == 'G') m = 1024.0 * 1024 * 1024, end++;
  if (*end == 'b' || *end == 'B') end++;
  if (*end != '\0') *ok = false;
  const double bytes = v * m;
  return bytes >= 9.0e18 ? INT64_MAX : (int64_t)bytes;  // (beyond any buffer: "always")
}

bool loadSizeTable(CommTuning* t, const char* path) {
  for (int n = 0; n <= NCCL_AMD_MAX_RANKS; n++) {
    const int64_t d = n > 0 ? n : 1;
    t->tableLL[n] = std::max<int64_t>(16 << 10, ((int64_t)256 << 10) / d);
    t->tableLL128[n] = std::max<int64_t>(64 << 10, ((int64_t)1 << 20) / d);
    t->tableOneShot[n] = n == 2 ? ((int64_t)2 << 20) : ((int64_t)2 << 20) / d;
  }
  if (path == nullptr || path[0] == '\0') return true;
  FILE* f = fopen(path, "r");
  if (f == nullptr) {
    WARN("NCCL_AMD_SIZE_TABLE=%s: cannot open (%s); using the built-in size table", path, strerror(errno));
    return false;
  }
  char line[512];
  int lineNo = 0, rows = 0;
  bool good = true;
  while (fgets(line, sizeof(line), f)) {
    lineNo++;
    if (char* hash = strchr(line, '#')) *hash = '\0';
    char a[64], b[64], c[64], d[64], extra[8];
    const int k = sscanf(line, "%63s %63s %63s %63s %7s", a, b, c, d, extra);
    if (k <= 0) continue;  // blank or comment
    bool okB = false, okC = false, okD = false;
    int lo = 0, hi = 0;
    if (k == 4) {
      const int64_t vb = parseBytes(b, &okB), vc = parseBytes(c, &okC), vd = parseBytes(d, &okD);
      char* end = nullptr;
      const long nr = strtol(a, &end, 10);
      if (!strcmp(a, "*")) lo = 1, hi = NCCL_AMD_MAX_RANKS;
      else if (end != a && *end == '\0' && nr >= 1 && nr <= NCCL_AMD_MAX_RANKS) lo = hi = (int)nr;
      if (lo && okB && okC && okD) {
        for (int n = lo; n <= hi; n++) {
          if (vb >= 0) t->tableLL[n] = vb;
          if (vc >= 0) t->tableLL128[n] = vc;
          if (vd >= 0) t->tableOneShot[n] = vd;
        }
        rows++;
        continue;
      }
    }
    WARN("NCCL_AMD_SIZE_TABLE=%s:%d: expected 'nranks|* ll ll128 oneshot' (bytes, K/M/G, '-' = built-in); line ignored",
         path, lineNo);
    good = false;
  }
  fclose(f);
  INFO("NCCL_AMD_SIZE_TABLE=%s: %d rows applied", path, rows);
  return good;
}

// CU budget of the large staged and zero-copy plans at n >= 3 (reference: channels and threads shrink below
// saturation, enqueue.cc:2091-2105; tuning.cc:243-400). The links bound those plans on the 8-GPU node: a rank
// sends 2S/n over each of its n-1 links, taking 2S/n / B_link, while its local HBM moves (3 + 2(n-1)/n) S (staged
// path with the pull gather), so keeping the links busy takes (2.5n - 1) B_link of HBM traffic. A
// workgroup of the staged kernel sustains R_wg ≈ 23 GB/s of it (n = 4 rehearsal, 4 ranks x 32 channels = 128
// workgroups each on its own CU, far from the HBM limit: 4 x 4.5 S = 4.83 GB in 1.609 ms; the handshakes and the
// fold's several sources halve the pure-copy rate of ≈ 40-50 GB/s per workgroup, profiles/r02_wg_rate_probe.txt).
// With B_link = 76.8 GB/s per direction (153.6 GB/s per link read as bidirectional) and 2x headroom,
// rounded up to a power of two (>= 32): 64 channels at n = 3..4, 128 at n = 5..8 — the rest of the chip stays free
// for the compute a collective overlaps. n = 2 keeps every channel (one link, nothing to overlap in the bench).
// NCCL_MAX_CTAS / NCCL_MAX_NCHANNELS / config.maxCTAs overrule it, as does NCCL_AMD_LINK_CHANNELS (0 = no budget).
// (Round 4's budget priced a workgroup at the pure-copy rate, 50 GB/s, and gave 32 channels at n = 3..4: its 2x
// headroom was the staged kernel's own factor of 2, none left for remote-store latency.)
int linkChannelBudget(int n) {
  if (n < 3) return 0;
  const double bLinkGBps = 76.8, wgGBps = 23.0, headroom = 2.0;
  const double need = (2.5 * n - 1.0) * bLinkGBps / wgGBps * headroom;
  int c = 32;
  while (c < need && c < NCCL_AMD_MAX_CHANNELS) c *= 2;
  return c;
}

// Channels per launch that stay co-resident when several ranks share a GPU (NCCL_MULTI_RANK_GPU_ENABLE, the one-GPU
// rehearsals). A channel spins on the same channel of every peer, so a collective progresses only while, for some
// channel, every rank's workgroup is resident. A GPU holds 2 of these workgroups per CU (512 threads, 4 waves per
// SIMD, kernels.h kCoResident). One rank per GPU: 2 x CUs. Ranks sharing a GPU: CUs / ranks per GPU, half the slots
// kept free. Slot arithmetic says 2 x CUs / ranks per GPU would fit (a stream never has two launches resident,
// tests/native/barrier_probe), yet round 5's n = 8 rehearsal stalled once at exactly that; the cause is not
// established, so the margin stays.
int coResidentChannelCap(int minCUs, int ranksPerGpu) {
  if (minCUs < 1) minCUs = 256;
  if (ranksPerGpu < 1) ranksPerGpu = 1;
  const int cap = ranksPerGpu == 1 ? 2 * minCUs : minCUs / ranksPerGpu;
  return cap < 1 ? 1 : cap;
}

void resolveLinkChannels(CommTuning* t, int nranks, bool userMaxCTAs) {
  const int64_t env = paramInt("NCCL_AMD_LINK_CHANNELS", -1);
  t->linkChannels = env >= 0 ? (int)env : userMaxCTAs ? 0 : linkChannelBudget(nranks);
}

// The fence default once the ranks' devices are known (all ranks see the same peer table and rank 0's knobs).
void resolveFence(CommTuning* t, bool oneDevice) {
  if (t->p2pFence < 0 && oneDevice) t->protoFlags |= 8;
}

// pinned (or registered) host memory mapped for the device: a kernel's accesses to it cross PCIe
static bool isHostMemory(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// Pointer check (reference argcheck.cc:12-28), active with NCCL_CHECK_POINTERS=1.
ncclResult_t ptrCheck(const void* p, ncclComm* comm, const char* name, const char* opname) {
  hipPointerAttribute_t attr;
  hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess || attr.devicePointer == nullptr) {
    (void)hipGetLastError();
    WARN("%s : %s %p is not a valid pointer", opname, name, p);
    return ncclInvalidArgument;
  }
  if (attr.type == hipMemoryTypeDevice && attr.device != comm->device) {
    WARN("%s : %s allocated on device %d mismatchs with NCCL device %d", opname, name, attr.device, comm->device);
    return ncclInvalidArgument;
  }
  return ncclSuccess;
}

// ArgsCheck (reference argcheck.cc:201-254).
static ncclResult_t argsCheck(CollInfo* info) {
  ncclComm* comm = info->comm;
  if (info->root < 0 || info->root >= comm->nRanks) {
    WARN("%s : invalid root %d (root should be in the 0..%d range)", info->opName, info->root, comm->nRanks);
    return ncclInvalidArgument;
  }
  if (info->datatype < 0 || info->datatype >= ncclNumTypes) {
    WARN("%s : invalid type %d", info->opName, info->datatype);
    return ncclInvalidArgument;
  }
  if (info->op < 0 || ncclMaxRedOp < info->op) {
    WARN("%s : invalid reduction operation %d", info->opName, info->op);
    return ncclInvalidArgument;
  }
  int opIx = (int)info->op - (int)ncclNumOps;
  if (ncclNumOps <= info->op && (opIx >= (int)comm->userOps.size() || !comm->userOps[opIx].used)) {
    WARN("%s : reduction operation %d unknown to this communicator", info->opName, info->op);
    return ncclInvalidArgument;
  }
  if (comm->tune.checkPointers && info->count > 0) {
    // Broadcast reads sendbuff on the root only (reference argcheck.cc:236-238): elsewhere it may be anything
    if (info->func != FUNC_BROADCAST || comm->rank == info->root)
      NCCLCHECK(ptrCheck(info->sendbuff, comm, "sendbuff", info->opName));
    if (info->func != FUNC_REDUCE || comm->rank == info->root)
      NCCLCHECK(ptrCheck(info->recvbuff, comm, "recvbuff", info->opName));
  }
  return ncclSuccess;
}

// ---- algorithm / channel choice (reference tuning.cc:243-400, enqueue.cc:2028-2180, 576-857) ----
// One node, full xGMI mesh: the only algorithm is the direct scatter-reduce-gather; what is tuned is
// the channel (workgroup) count and the pipeline slice. Every rank computes the same plan from the
// same (count, type, nRanks, params), which the protocol requires.
static void planChannels(ncclComm* comm, size_t blockBytes, int eltSize, LaunchPlan& p, size_t minPart,
                         int maxCh) {
  if (minPart < 16) minPart = 16;
  int nch = (int)((blockBytes + minPart - 1) / minPart);
  if (nch < comm->minCTAs) nch = comm->minCTAs;
  if (nch > maxCh) nch = maxCh;
  if (nch > comm->chanCap) nch = comm->chanCap;
  if (nch < 1) nch = 1;
  const uint64_t epp = 16 / eltSize;
  uint64_t blockElems = blockBytes / eltSize;
  uint64_t part = (blockElems + nch - 1) / nch;
  part = (part + epp - 1) / epp * epp;
  if (part == 0) part = epp;
  uint64_t slice = comm->slotBytes / eltSize;
  slice = slice / epp * epp;
  if (slice > part) slice = part;
  p.nChannels = nch;
  p.args.part = part;
  p.args.slice = slice;
  p.args.nSteps = (int)((part + slice - 1) / slice);
}

// NCCL_ALGO=RING AllReduce: the reference's own partition, so that every element is finalised by the same ring
// position as in the reference's RING/SIMPLE AllReduce on a communicator of K channels (K = refChannelCount below,
// i.e. NCCL_MIN_NCHANNELS = NCCL_MAX_NCHANNELS = K there) with the same NCCL_BUFFSIZE — bit-identical results, floats
// included. NCCL_AMD_REF_ORDER walks the same partition, or the one of RING/LL or RING/LL128
// (`proto` 0 / 1). For one task, starting on channel 0 with no traffic planned yet:
//  * channels: K shrunk while the bytes are below K x threads x threshold — 512 x 64 (Simple), 512 x 8n (LL),
//    640 x 8 (LL128) (topoGetAlgoInfo, enqueue.cc:2091-2097; tuning.cc:244-257, 589-593);
//  * channel parts over cells of 32 KiB of traffic (AllReduce: 2 bytes of traffic per byte, 8 under LL,
//    enqueue.cc:461, 658): a first part sized to the traffic per channel, equal middle parts, a remainder part
//    (scheduleCollTasksToPlan, enqueue.cc:576-757);
//  * each part walked in loops of n chunks of tune.ringChunkBytes / refChunkBytes, the last loop re-cut (kernel,
//    pipe.h).
struct RingParts {
  int nch;
  uint64_t lo, mid, hi;
};
// The reference never runs more than MAXCHANNELS = 64 channels (src/include/device.h:91), so a partition of
// more parts than that is one no reference run produces: K = NCCL_AMD_REF_NCHANNELS, else the channel cap, and
// at most 64 (warned once when a larger count is clamped). Every part needs a workgroup of its own, so K never
// exceeds the channel cap either (several ranks per GPU, NCCL_MAX_CTAS): the staging holds that many channels.
constexpr int kRefMaxChannels = 64;
static int refChannelCount(ncclComm* comm) {
  const int want = comm->tune.refChannels > 0 ? comm->tune.refChannels : comm->chanCap;
  const int k = std::max(1, std::min(want, std::min(kRefMaxChannels, comm->chanCap)));
  if (k != want && !comm->warnedRefClamp && want >= 1) {
    comm->warnedRefClamp = true;
    WARN("the reference's partition is cut into %d channel parts, not %d (%s): at most %d (MAXCHANNELS, device.h:91) "
         "and at most the channel cap %d; set NCCL_AMD_REF_NCHANNELS to the reference run's channel count", k, want,
         comm->tune.refChannels > 0 ? "NCCL_AMD_REF_NCHANNELS" : "the channel cap", kRefMaxChannels, comm->chanCap);
  }
  return k;
}
static RingParts ringParts(uint64_t count, int ts, int K, int n, int proto) {
  const uint64_t bytes = count * (uint64_t)ts;
  const uint64_t threads = proto == 1 ? 640 : 512, threshold = proto == 0 ? 8 * (uint64_t)n : proto == 1 ? 8 : 64;
  int nc = K;
  while (nc >= 2 && bytes < (uint64_t)nc * threads * threshold) nc--;
  const uint64_t tpb = proto == 0 ? 8 : 2;  // traffic bytes per AllReduce byte
  const uint64_t cell = ((32 << 10) / tpb + 15) / 16 * 16, trafficCell = tpb * cell;
  const uint64_t eltsPerCell = cell / ts;
  const uint64_t cells = (bytes + cell - 1) / cell;
  const uint64_t traffic = std::max<uint64_t>(32 << 10, tpb * bytes);
  const uint64_t perChannel = (traffic / nc + 15) / 16 * 16;
  const uint64_t perChannelCells = (perChannel + trafficCell - 1) / trafficCell;
  uint64_t cellsPerCh = std::min(cells, perChannelCells);
  const uint64_t cellsLo = K == 1 ? cells : std::min(cells, perChannelCells);
  int64_t nMid = (int64_t)((cells - cellsLo) / cellsPerCh);
  uint64_t cellsHi = (cells - cellsLo) % cellsPerCh;
  if ((int64_t)K < (cellsLo ? 1 : 0) + nMid + (cellsHi ? 1 : 0)) {  // more parts than channels
    nMid = K - 2;
    cellsPerCh = (cells - cellsLo) / (uint64_t)(nMid + 1);
    cellsHi = cellsPerCh + (cells - cellsLo) % (uint64_t)(nMid + 1);
  }
  if (cellsHi == 0 && nMid != 0) {
    cellsHi = cellsPerCh;
    nMid--;
  }
  RingParts r;
  r.lo = cellsLo * eltsPerCell;
  r.mid = nMid ? cellsPerCh * eltsPerCell : 0;
  r.hi = cellsHi * eltsPerCell;
  (r.hi ? r.hi : r.lo) -= cells * eltsPerCell - count;  // the last part ends at count
  r.nch = (r.lo ? 1 : 0) + (int)nMid + (cellsHi ? 1 : 0);
  return r;
}

// Workgroups per reference channel part (CollArgs::refSub): the parts' chunks are cut into sub-chunks so that
// the launch fills `physCap` workgroups (the channel cap, and the CU budget at n >= 3 like the default plan)
// while no sub-chunk of a rank block drops below minChannelBytes (the default plan's per-channel granularity).
static uint32_t refSubCount(ncclComm* comm, const RingParts& r, uint64_t chunk, int n, int ts) {
  int physCap = comm->chanCap;
  if (n >= 3 && comm->tune.linkChannels > 0) physCap = std::min(physCap, std::max(comm->tune.linkChannels, r.nch));
  const uint64_t epp = 16 / ts;
  const uint64_t maxPart = std::max(r.lo, std::max(r.mid, r.hi));
  uint64_t ck = std::min<uint64_t>(chunk, ((maxPart + n - 1) / n + epp - 1) / epp * epp);  // largest chunk in use
  const uint64_t minSub = std::max<uint64_t>(epp, (uint64_t)comm->tune.minChannelBytes / ts);
  uint64_t g = std::min<uint64_t>(physCap / std::max(r.nch, 1), ck / minSub);
  return g < 1 ? 1 : (uint32_t)g;
}

// The plugin's regBuff (reference enqueue.cc:2141-2147): both buffers registered (an ncclCommRegister handle or a
// window), or a capture with NCCL_GRAPH_REGISTER on. Asked only when a tuner plugin is loaded. The plan must be the
// same on every rank, so regBuff rests only on what the user does on every rank alike: not on the eager cache, whose
// contents follow each rank's own LRU clock. A plugin must still not key on regBuff where its user
// registers buffers on some ranks only — the reference passes it the same way (enqueue.cc:2141-2148).
static int tunerRegBuff(ncclComm* comm, const CollInfo& info) {
  const int n = comm->nRanks;
  const size_t ts = (size_t)typeSize(info.datatype);
  size_t sb = info.count * ts, rb = info.count * ts;
  if (info.func == FUNC_REDUCESCATTER) sb *= n;
  if (info.func == FUNC_ALLGATHER) rb *= n;
  const bool sendOk = regCovers(comm, info.sendbuff, sb) || findSymWindow(comm, info.sendbuff, sb);
  const bool recvOk = info.recvbuff == nullptr || regCovers(comm, info.recvbuff, rb) || findSymWindow(comm, info.recvbuff, rb);
  if (sendOk && recvOk) return 1;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(info.stream, &st) == hipSuccess && st == hipStreamCaptureStatusActive;
  (void)hipGetLastError();
  return capturing && comm->tune.graphRegister ? 1 : 0;
}

// LL eligibility and channel plan of one AllReduce, ReduceScatter, AllGather or Reduce (reference tuning: LL for
// the smallest sizes, or as NCCL_PROTO dictates). Every rank must take the same decision from the same
// inputs, so it depends only on what all ranks share — count, type, op and the agreed knobs — never on the
// alignment of this rank's buffers (the kernel loads and stores payloads at any alignment). The blocked
// collectives need 8-byte multiples as rank blocks (a payload never straddles two blocks) and the line area
// must hold the payload space: the AllReduce / Reduce / Broadcast buffer or one ReduceScatter / AllGather rank block
// (a Broadcast arrives here with its count in bytes: planColl's callers normalised its datatype).
bool llPlan(const CollInfo& info, LLOp* op) {
  ncclComm* comm = info.comm;
  if (comm->nRanks == 1) return false;
  const int n = comm->nRanks;
  const int ts = typeSize(info.datatype);
  const size_t bytes = info.count * (size_t)ts;  // payload space
  const size_t npk = (bytes + 7) / 8;
  const size_t nLines = (bytes + kLL64Payload - 1) / kLL64Payload;  // LL64 lines
  const CommTuning& t = comm->tune;
  const FuncTuning& ft = t.fn[info.func];
  const bool blocked = info.func == FUNC_REDUCESCATTER || info.func == FUNC_ALLGATHER;
  const bool shape = !blocked || (bytes & 7) == 0;
  const bool fits = ft.llOn && shape && npk <= (size_t)comm->llChannels * (comm->llBytes / 16);
  const bool fits64 = ft.ll128On && shape && nLines <= (size_t)comm->llChannels * (comm->llBytes / 64);
  // a forced NCCL_ALGO (ONESHOT / DIRECT / RING / TREE) selects the SIMPLE-protocol kernels unless
  // NCCL_PROTO leaves only LL-class protocols enabled.
  // LL lines carry 2x the payload to each of the n-1 peers: its range shrinks with n like the one-shot's
  // (default 256 KiB / n: 128 KiB at n=2, 32 KiB at n=8; for ReduceScatter / AllGather that is per rank
  // block, i.e. 256 KiB of total data at any n, the same per-rank link bytes). LL64 lines carry 64/56 of
  // it, so the LL128 class takes the next range (default up to 1 MiB / n) before one-shot / direct.
  const size_t llLim = t.llBytes > 0 ? (size_t)t.llBytes : (size_t)t.tableLL[n];
  const size_t ll64Lim = t.ll128Bytes > 0 ? (size_t)t.ll128Bytes : (size_t)t.tableLL128[n];
  const bool sized = ft.algo == FORCE_NONE;
  int proto = -1;
  if (!ft.simpleOn) {  // only LL-class protocols enabled: the range's protocol, else whichever fits
    if (fits && (bytes <= llLim || !fits64)) proto = LLP_LL;
    else if (fits64) proto = LLP_LL64;
  } else if (fits && sized && bytes <= llLim) {
    proto = LLP_LL;
  } else if (fits64 && sized && bytes <= ll64Lim) {
    proto = LLP_LL64;
  }
  int tuned = TUNE_DEFAULT, tunedNch = 0;
  if (comm->tunerLoaded) {  // an external tuner plugin may overrule the size table (tuner.cc)
    tunerPick(comm, info.func, blocked ? bytes * n : bytes, 1, (fits ? 1 : 0) | (fits64 ? 2 : 0), tunerRegBuff(comm, info),
              &tuned, &tunedNch);
    if (tuned != TUNE_DEFAULT) proto = (fits && tuned == TUNE_LL) ? LLP_LL : (fits64 && tuned == TUNE_LL128) ? LLP_LL64 : -1;
  }
  if (proto < 0) return false;
  // LL: 8-byte payloads, one 16-byte line each; LL64: 56-byte lines of 64 bytes
  const uint64_t units = proto == LLP_LL ? npk : nLines;
  const uint64_t unitLine = proto == LLP_LL ? 16 : 64;
  const uint64_t perCh = proto == LLP_LL ? (uint64_t)t.llChannelBytes / 8 : (uint64_t)t.ll128ChannelBytes / kLL64Payload;
  int nch = (int)((units + perCh - 1) / perCh);
  if (tunedNch > 0 && (uint64_t)tunedNch * (comm->llBytes / unitLine) >= units) nch = tunedNch;
  if (nch < 1) nch = 1;
  if (nch > comm->llChannels) nch = comm->llChannels;
  if (nch > comm->chanCap) nch = comm->chanCap;
  uint64_t part = (units + nch - 1) / nch;
  if (part * unitLine > comm->llBytes) return false;
  // every channel of the op must carry at least one payload: an empty channel would advance its epoch
  // without exchanging lines, and the parity double-buffering (kernels.h llChannelOp) relies on each epoch
  // of a channel waiting for every peer's lines of the previous one (a tuner's channel count, or a tiny
  // NCCL_AMD_LL_CHANNEL_BYTES, can leave [lo,hi) empty for the last channels otherwise)
  nch = (int)((units + part - 1) / part);
  const uint64_t epp = 16 / ts;
  uint64_t blockElems = info.count;
  if (info.func == FUNC_ALLREDUCE) {
    blockElems = (info.count + n - 1) / n;
    blockElems = (blockElems + epp - 1) / epp * epp;
  }
  op->send = info.sendbuff;
  op->recv = info.recvbuff;
  op->count = info.count;
  op->chunk = blockElems ? blockElems : epp;
  op->part = part;
  op->nch = nch;
  op->chOff = 0;
  op->coll = info.func == FUNC_ALLREDUCE ? LL_AR : info.func == FUNC_REDUCESCATTER ? LL_RS
           : info.func == FUNC_ALLGATHER ? LL_AG : info.func == FUNC_BROADCAST ? LL_BCAST : LL_REDUCE;
  op->root = info.root;
  op->proto = proto;
  return true;
}

// Plan one op: the kernel launch (PLAN_KERNEL, in p), the symmetric-window launch (PLAN_SYM, in sp) or
// nothing (PLAN_NONE). Every rank derives the same plan from what all ranks share.
// Eager zero-copy for this communicator (NCCL_AMD_EAGER_REGISTER: 1 always, 0 never (default), -1 when it spans
// processes whose every peer serves registrations). Every rank computes the same answer from the shared peer table.
static bool eagerOn(const ncclComm* comm) {
  return comm->tune.eagerRegister > 0 || (comm->tune.eagerRegister < 0 && comm->multiProcess && comm->regIpcAll);
}

// Zero-copy AlltoAll / Gather (kernels.h symA2AKernel). Every rank makes the same call, so every rank
// decides alike from what all ranks share (n, count, the agreed knobs) and from its own sendbuff, which lies in a
// symmetric window on every rank or on none (same-offset contract of the other symmetric plans). Never from recvbuff
// (no peer reads it; a Gather non-root's is unused), the rank or the root: that would split the kernel kinds.
bool symA2AEligible(ncclComm* comm, const void* sendbuff, size_t sendBytes, size_t count) {
  return comm->nRanks >= 2 && count > 0 && !comm->tune.symDisable && comm->tune.symA2A != 0 &&
         findSymWindow(comm, sendbuff, sendBytes) != nullptr;
}

// The channel cap of a symA2AKernel launch: the co-resident cap and, at n >= 3, the CU budget of the other symmetric
// plans (linkChannels)
static int symA2AChannelCap(const ncclComm* comm) {
  int cap = comm->chanCap;
  if (comm->nRanks >= 3 && comm->tune.linkChannels > 0) cap = std::min(cap, comm->tune.linkChannels);
  return cap;
}

static ncclResult_t planSymA2A(const CollInfo& info, SymPlan& sp, int* kind) {
  ncclComm* comm = info.comm;
  const int n = comm->nRanks;
  const bool gather = info.func == FUNC_SYM_GATHER;
  const size_t B = info.count * (size_t)typeSize(info.datatype);
  ncclWindow_vidmem* ws = n >= 2 && B > 0 ? findSymWindow(comm, info.sendbuff, gather ? B : (size_t)n * B) : nullptr;
  if (!ws) {  // (the entry point asked symA2AEligible; a window deregistered inside the group since)
    WARN("%s: the symmetric window that held sendbuff %p at the call is gone", info.opName, info.sendbuff);
    return ncclInvalidUsage;
  }
  comm->opCount++;
  *kind = PLAN_SYM;
  memset(&sp, 0, sizeof(sp));
  sp.coll = gather ? 5 /*SYM_GATHER*/ : 4 /*SYM_A2A*/;
  sp.datatype = ncclInt8;  // bytes
  sp.eltSize = 1;
  sp.stream = info.stream;
  SymA2AArgs& a = sp.a2a;
  a.comm = comm->devComm;
  for (int r = 0; r < n; r++) a.send[r] = ws->peerPtr[r] + ((const char*)info.sendbuff - (const char*)ws->userPtr);
  a.send[comm->rank] = (const char*)info.sendbuff;
  a.recv = (char*)info.recvbuff;
  a.bytes = B;
  a.mode = gather ? SYM_A2A_GATHER : SYM_A2A_ALLTOALL;
  a.root = info.root;
  a.elementwise = comm->tune.forceElementwise;
  const SymA2ACut cut = symA2ACut(B, (uint64_t)std::max<int64_t>(1, comm->tune.minChannelBytes), comm->minCTAs,
                                  symA2AChannelCap(comm));
  a.part = cut.part;
  sp.nChannels = cut.nch;
  TRACE("%s: symmetric nch %d part %lu bytes %zu root %d", info.opName, cut.nch, (unsigned long)cut.part, B, info.root);
  return ncclSuccess;
}

ncclResult_t planColl(const CollInfo& info, LaunchPlan& p, SymPlan& sp, int* kind) {
  ncclComm* comm = info.comm;
  const int ts = typeSize(info.datatype);
  memset(&p, 0, sizeof(p));
  *kind = PLAN_KERNEL;
  if (info.func == FUNC_SYM_ALLTOALL || info.func == FUNC_SYM_GATHER) return planSymA2A(info, sp, kind);
  p.func = info.func;
  p.datatype = info.datatype;
  p.eltSize = ts;
  p.stream = info.stream;
  p.args.sendbuff = info.sendbuff;
  p.args.recvbuff = info.recvbuff;
  p.args.comm = comm->devComm;
  p.args.root = info.root;
  const void* argPtr = nullptr;
  if (info.func != FUNC_ALLGATHER && info.func != FUNC_BROADCAST) {
    NCCLCHECK(hostToDevRedOp(comm, info.op, info.datatype, &p.devOp, &p.args.redArg, &argPtr));
    p.args.redArgPtr = argPtr;
  }
  const int n = comm->nRanks;
  comm->opCount++;

  if (n == 1) {
    // reference taskAppend → ncclLaunchOneRank (enqueue.cc:3039-3041, onerank.cu:49-110)
    size_t bytes = info.count * (size_t)ts;
    if ((info.func == FUNC_REDUCE && info.recvbuff == nullptr) ||
        (info.func == FUNC_BROADCAST && info.recvbuff == info.sendbuff)) {  // (an in-place Broadcast: nothing to do)
      *kind = PLAN_NONE;
      return ncclSuccess;
    }
    if (p.devOp == DEV_PREMULSUM) {
      p.algo = ALGO_ONERANK;
      p.args.count = info.count;
      return ncclSuccess;
    }
    p.algo = ALGO_COPY;
    p.bytes = bytes;
    p.copyVariant = comm->tune.copyVariant;
    p.copyGrid = comm->tune.copyGrid;
    p.copyXcdShift = comm->tune.copyXcdShift;
    // one pointer query per out-of-place copy of >= 1 MiB (about a microsecond, overlapped with the GPU's work)
    if (comm->tune.hostCopyGrid > 0 && bytes >= (1u << 20) && info.sendbuff != info.recvbuff &&
        (isHostMemory(info.sendbuff) || isHostMemory(info.recvbuff)))
      p.copyGrid = std::min<int64_t>(p.copyGrid, comm->tune.hostCopyGrid);
    return ncclSuccess;
  }

  const FuncTuning& ft = comm->tune.fn[info.func];
  if (ft.noAlgo) {  // reference enqueue.cc:2052-2065 (ncclInvalidUsage when NCCL_ALGO / NCCL_PROTO caused it)
    WARN("No algorithm/protocol available for function %s with datatype %d. NCCL_ALGO was set to %s. NCCL_PROTO was "
         "set to %s.", info.opName, (int)info.datatype, paramStr("NCCL_ALGO") ? paramStr("NCCL_ALGO") : "(unset)",
         paramStr("NCCL_PROTO") ? paramStr("NCCL_PROTO") : "(unset)");
    return ncclInvalidUsage;
  }
  p.algo = ALGO_DIRECT;
  const uint64_t epp = 16 / ts;
  size_t count = info.count;
  uint64_t blockElems;
  switch (info.func) {
    case FUNC_ALLREDUCE:
    case FUNC_BROADCAST:  // (bytes: n blocks of alignUp(divUp(bytes, n), 16), kernels.h Channel::bcastA)
    case FUNC_REDUCE: {
      // rank block = alignUp(divUp(count, n), 16/sizeof(T)) (reference all_reduce.h:38); a Reduce over
      // n >= 3 ranks cuts n-1 blocks, none owned by the root (kernels.h Channel::rootless)
      const int nb = (info.func == FUNC_REDUCE && n >= 3) ? n - 1 : n;
      blockElems = (count + nb - 1) / nb;
      blockElems = (blockElems + epp - 1) / epp * epp;
      break;
    }
    default:  // RS: recvcount, AG: sendcount
      blockElems = count;
      break;
  }
  p.args.count = count;
  p.args.chunk = blockElems;
  uintptr_t bases = (uintptr_t)info.sendbuff | (uintptr_t)info.recvbuff;
  // (a Broadcast's sendbuff is read on the root only: elsewhere its value says nothing)
  if (info.func == FUNC_BROADCAST && comm->rank != info.root) bases = (uintptr_t)info.recvbuff;
  bool aligned = (bases & 15) == 0;
  if (info.func == FUNC_REDUCESCATTER || info.func == FUNC_ALLGATHER) aligned = aligned && ((count * ts) & 15) == 0;
  if (comm->tune.forceElementwise) aligned = false;  // diagnostics: T-sized accesses only
  p.args.aligned = aligned ? 1 : 0;
  // protoFlags bit 8 = no system release fence (buffer_wbl2) before data flags: all published bytes are
  // stored write-through at system scope and drained (§4); set when every rank shares one GPU or with
  // NCCL_AMD_P2P_FENCE=0 (resolveFence).
  p.args.protoFlags = comm->tune.protoFlags;
  // Algorithm choice (reference: NCCL_ALGO / tuning.cc cost model): one-shot for small AllReduce
  // (latency: one handshake), direct scatter-reduce-gather otherwise (bandwidth). NCCL_ALGO=ONESHOT or
  // DIRECT forces either; the reference's RING and TREE run their own kernels (pipe.h, below).
  bool oneShot = false;
  if (info.func == FUNC_ALLREDUCE) {
    // one-shot moves (n-1)S link bytes per rank vs 2(n-1)S/n for the direct path, but saves two
    // handshakes: the crossover shrinks with n (default 2 MiB / n: 512 KiB at n=4, 256 KiB at n=8). At n = 2
    // both move S over the one link and 4S of HBM per rank, so only one-shot's 32-channel cap ends its range:
    // 2 MiB there (one-GPU rehearsal, fp16: 2 MiB one-shot 14.1 us vs direct 16.0, 4 MiB 23.1 vs 17.7;
    // profiles/r02_scale_rehearsal_n2_onegpu.json)
    size_t bytes = count * (size_t)ts;
    size_t lim = comm->tune.oneShotBytes > 0 ? (size_t)comm->tune.oneShotBytes : (size_t)comm->tune.tableOneShot[n];
    // several algorithms enabled: the size table, over the SIMPLE kernels they leave (resolveFuncTuning)
    oneShot = ft.algo == FORCE_ONESHOT || (ft.algo == FORCE_NONE && ft.oneShotOk && (bytes <= lim || !ft.directOk));
  }
  // NCCL_AMD_REF_ORDER: AllReduce always on the direct kernel in the reference's partition (below)
  const bool refOrder = comm->tune.refOrder && info.func == FUNC_ALLREDUCE && ft.algo != FORCE_RING &&
                        ft.algo != FORCE_TREE;
  if (refOrder) oneShot = false;
  // NCCL_ALGO=RING with NCCL_PROTO naming LL or LL128 alone: the reference's RING/LL or RING/LL128 AllReduce, i.e.
  // the ring kernel on that protocol's partition (ringParts), not this engine's LL kernel (another fold order)
  const bool ringProtoPart = info.func == FUNC_ALLREDUCE && ft.algo == FORCE_RING && comm->tune.refProto != 2;
  int tunedNch = 0;
  if (comm->tunerLoaded) {  // external tuner plugin: one-shot (TREE/SIMPLE) vs direct (RING/SIMPLE), channels
    int tuned = TUNE_DEFAULT;
    tunerPick(comm, info.func, count * (size_t)ts * (info.func == FUNC_ALLGATHER || info.func == FUNC_REDUCESCATTER ? n : 1),
              1, false, tunerRegBuff(comm, info), &tuned, &tunedNch);
    if (tuned == TUNE_ONESHOT && info.func == FUNC_ALLREDUCE) oneShot = true;
    if (tuned == TUNE_DIRECT) oneShot = false;
  }
  const bool oneShotAR = oneShot;
  // LL protocol (reference NCCL_PROTO=LL, prims_ll.h): small AllReduce / ReduceScatter / AllGather /
  // Reduce, one launch, no fences
  if (!refOrder && !ringProtoPart && llPlan(info, &p.ll.ops[0])) {
    p.algo = ALGO_LL;
    p.ll.comm = comm->devComm;
    p.ll.counters = comm->counters;
    p.ll.redArg = p.args.redArg;
    p.ll.redArgPtr = p.args.redArgPtr;
    p.ll.nOps = 1;
    p.nChannels = p.ll.ops[0].nch;
    TRACE("%s: %s count %zu nch %d part %lu %s", info.opName, p.ll.ops[0].proto == LLP_LL64 ? "LL128(LL64)" : "LL",
          count, p.nChannels, (unsigned long)p.ll.ops[0].part, p.ll.ops[0].proto == LLP_LL64 ? "lines" : "payloads");
    return ncclSuccess;
  }
  // The reference's own algorithms, forced with NCCL_ALGO=RING / TREE (pipe.h): the ring for AllReduce,
  // ReduceScatter and AllGather, the chain (the intra-node tree) for AllReduce; Reduce's ring is the chain
  // to the root (reduce.h). Where the reference has no such algorithm the default plan runs, with a warning.
  // Broadcast has no fold order for a ring kernel to reproduce: NCCL_ALGO=RING (the reference's only Broadcast
  // algorithm) and DIRECT run the direct plan; TREE or ONESHOT alone name nothing Broadcast has
  if (info.func == FUNC_BROADCAST && (ft.algo == FORCE_TREE || ft.algo == FORCE_ONESHOT) &&
      !(comm->warnedAlgo & (1u << info.func))) {
    comm->warnedAlgo |= 1u << info.func;
    WARN("NCCL_ALGO=%s: no such algorithm for Broadcast; using the default plan", kForceName[ft.algo]);
  }
  if ((ft.algo == FORCE_RING || ft.algo == FORCE_TREE) && info.func != FUNC_BROADCAST) {
    const bool ring = ft.algo == FORCE_RING;
    int kind = -1;
    if (info.func == FUNC_ALLREDUCE) kind = ring ? PIPE_RING_AR : PIPE_CHAIN_AR;
    else if (ring) kind = info.func == FUNC_REDUCESCATTER ? PIPE_RING_RS : info.func == FUNC_ALLGATHER ? PIPE_RING_AG
                                                                                                   : PIPE_CHAIN_REDUCE;
    // A ring hop receives and sends on the same cycle of links: with one staging slot per link every rank
    // would hold its outgoing slot full while waiting for its successor to drain it (a cyclic wait), so the
    // ring needs at least two slots; the chain is acyclic and runs with one.
    const bool cyclic = kind == PIPE_RING_AR || kind == PIPE_RING_RS || kind == PIPE_RING_AG;
    if (kind < 0 || (cyclic && comm->nSlots < 2)) {
      if (!(comm->warnedAlgo & (1u << info.func))) {
        comm->warnedAlgo |= 1u << info.func;
        if (kind < 0)
          WARN("NCCL_ALGO=TREE: no tree algorithm for %s (the reference has none either); using the default plan",
               info.opName);
        else
          WARN("NCCL_ALGO=RING needs NCCL_AMD_NSLOTS >= 2 (have %d); %s uses the default plan", comm->nSlots,
               info.opName);
      }
    } else {
      p.algo = ALGO_PIPE;
      p.pipeKind = kind;
      const bool chain = kind == PIPE_CHAIN_AR || kind == PIPE_CHAIN_REDUCE;
      if (chain) p.args.chunk = count;  // one block: the chain folds every element in the same order
      const size_t span = chain ? count * ts : blockElems * ts;
      planChannels(comm, span, ts, p, (size_t)comm->tune.minChannelBytes, comm->chanCap);
      if (kind == PIPE_RING_AR) {  // the reference's channel parts and loop chunk (ringParts above)
        const RingParts r = ringParts(count, ts, refChannelCount(comm), n, comm->tune.refProto);
        p.args.cbdLo = r.lo;
        p.args.part = r.mid;
        p.args.cbdHi = r.hi;
        p.args.chunk = (uint64_t)comm->tune.refChunkBytes / ts;
        p.args.refSub = refSubCount(comm, r, p.args.chunk, n, ts);
        p.nChannels = r.nch * (int)p.args.refSub;
        p.args.slice = std::min<uint64_t>(p.args.chunk, comm->slotBytes / ts / epp * epp);
        p.args.nSteps = 0;  // per channel and loop (pipe.h)
      }
      TRACE("%s: %s kind %d nch %d part %lu slice %lu steps %d", info.opName, ring ? "RING" : "TREE", kind,
            p.nChannels, (unsigned long)p.args.part, (unsigned long)p.args.slice, p.args.nSteps);
      return ncclSuccess;
    }
  }
  if (refOrder) {
    // The reference's ring partition of the protocol NCCL_PROTO names (ringParts: channel parts, the protocol's
    // chunks, loops; Simple unless NCCL_PROTO is LL or LL128 alone) walked by the direct scatter-reduce-gather kernel: in each loop chunk q is finalised by rank q, as in the reference's ring,
    // so every element folds in its order — at the direct kernel's n-1 links instead of the ring's one (kernels.h
    // Channel::refPart). K reference parts (at most 64), each served by refSub workgroups (refSubCount).
    const RingParts r = ringParts(count, ts, refChannelCount(comm), n, comm->tune.refProto);
    p.args.cbdLo = r.lo;
    p.args.part = r.mid;
    p.args.cbdHi = r.hi;
    p.args.chunk = (uint64_t)comm->tune.refChunkBytes / ts;
    p.args.refSub = refSubCount(comm, r, p.args.chunk, n, ts);
    p.nChannels = r.nch * (int)p.args.refSub;
    p.args.slice = std::min<uint64_t>(p.args.chunk, comm->slotBytes / ts / epp * epp);
    p.args.nSteps = 0;  // per channel (kernels.h Channel::refInit)
    TRACE("%s: direct in the reference's partition, %d parts x %u workgroups, parts %lu/%lu/%lu chunk %lu slice %lu",
          info.opName, r.nch, p.args.refSub, (unsigned long)r.lo, (unsigned long)r.mid, (unsigned long)r.hi,
          (unsigned long)p.args.chunk, (unsigned long)p.args.slice);
    return ncclSuccess;
  }
  // Zero-copy kernels (kernels.h symKernel): buffers in NCCL_WIN_COLL_SYMMETRIC windows (reference: symmetric
  // kernels, src/enqueue.cc ncclSymkAvailable / src/device/symmetric/*), or registered with ncclCommRegister /
  // auto-registered under stream capture (reference: IPC-registered ring buffers, src/register/coll_reg.cc:
  // 326-395). Reduce and Broadcast keep the staged path whatever their buffers are.
  if (info.func != FUNC_REDUCE && info.func != FUNC_BROADCAST && !comm->tune.symDisable) {
    size_t sb = count * ts, rb = count * ts;
    if (info.func == FUNC_REDUCESCATTER) sb *= n;
    if (info.func == FUNC_ALLGATHER) rb *= n;
    const char* sendPtr[NCCL_AMD_MAX_RANKS] = {};
    char* recvPtr[NCCL_AMD_MAX_RANKS] = {};
    int regMode = -1;
    // AllGather reads only peers' outputs (symKernel SYM_AG), so its sendbuff needs no window
    ncclWindow_vidmem* ws = info.func == FUNC_ALLGATHER ? nullptr : findSymWindow(comm, info.sendbuff, sb);
    ncclWindow_vidmem* wr = (ws || info.func == FUNC_ALLGATHER) ? findSymWindow(comm, info.recvbuff, rb) : nullptr;
    if (wr && (ws || info.func == FUNC_ALLGATHER)) {
      regMode = 0;
      for (int r = 0; r < n; r++) {
        // AllGather: only my own input is read (peers' blocks come from their outputs)
        if (ws) sendPtr[r] = ws->peerPtr[r] + ((const char*)info.sendbuff - (const char*)ws->userPtr);
        else sendPtr[r] = r == comm->rank ? (const char*)info.sendbuff : nullptr;
        recvPtr[r] = wr->peerPtr[r] + ((char*)info.recvbuff - (char*)wr->userPtr);
      }
    } else if (regLookup(comm, info.stream, info.func == FUNC_ALLGATHER ? nullptr : info.sendbuff, sb,
                         info.recvbuff, rb, sendPtr, recvPtr,
                         // eager registration (NCCL_AMD_EAGER_REGISTER=1): ops of at least eagerBytes whose staged
                         // plan would be the direct kernel, decided from what every rank shares (bytes, the table)
                         eagerOn(comm) && !oneShotAR && std::max(sb, rb) >= (size_t)comm->tune.eagerBytes)) {
      regMode = 1;  // my buffers as mapped in each peer; the kernel exchanges them at entry
      if (info.func == FUNC_ALLGATHER) sendPtr[comm->rank] = (const char*)info.sendbuff;
    }
    if (regMode >= 0) {
      *kind = PLAN_SYM;
      memset(&sp, 0, sizeof(sp));
      sp.datatype = info.datatype;
      sp.eltSize = ts;
      sp.devOp = p.devOp;
      sp.args.comm = comm->devComm;
      sp.args.count = count;
      sp.args.chunk = blockElems;
      sp.args.redArg = p.args.redArg;
      sp.args.redArgPtr = p.args.redArgPtr;
      sp.args.regMode = regMode;
      sp.regUse[0] = regMode == 1 ? comm->regLastUse[0] : nullptr;  // their lastEv follow this launch (regRecordUse)
      sp.regUse[1] = regMode == 1 ? comm->regLastUse[1] : nullptr;
      sp.bounced = regMode == 1 && comm->bounceUsed;  // this rank's buffers go through the bounce allocation
      if (sp.bounced) sp.bounce = comm->bounceNext;
      uintptr_t al = 0;
      for (int r = 0; r < n; r++) {
        sp.args.send[r] = sendPtr[r];
        sp.args.recv[r] = recvPtr[r];
        al |= (uintptr_t)sendPtr[r] | (uintptr_t)recvPtr[r];
      }
      // registered buffers: peers' pointers are known only in the kernel, which adds their alignment
      bool symAligned = (regMode || (al & 15) == 0) && !comm->tune.forceElementwise;
      if (info.func != FUNC_ALLREDUCE) symAligned = symAligned && ((count * ts) & 15) == 0;
      sp.args.aligned = symAligned ? 1 : 0;
      sp.args.wtPublish = comm->tune.symWtPublish;
      sp.args.relFence = (comm->tune.protoFlags & 8) == 0;  // across devices: release fence kept (resolveFence)
      size_t spanBytes = blockElems * ts;  // what one channel plan divides
      size_t minPart = (size_t)comm->tune.minChannelBytes;
      int maxCh = comm->chanCap;
      if (info.func == FUNC_ALLREDUCE) {
        // One-shot needs out-of-place buffers on EVERY rank (in place, peers would still read what a rank
        // overwrites), and whether a peer runs in place is not known here: ranks choosing different kernels
        // would run different handshake sequences. So one-shot only when NCCL_AMD_SYM_ONESHOT=1 declares
        // every call out of place; the default two-shot kernel is correct either way.
        bool out = info.sendbuff != info.recvbuff;
        if (comm->tune.symOneShot && !out) {
          WARN("%s: NCCL_AMD_SYM_ONESHOT=1 but the call is in place", info.opName);
          return ncclInvalidUsage;
        }
        sp.coll = (oneShotAR && comm->tune.symOneShot) ? 1 /*SYM_AR1*/ : 0 /*SYM_AR*/;
        if (sp.coll == 1) {
          spanBytes = count * ts;
          minPart = (size_t)comm->tune.oneShotChannelBytes;
          maxCh = maxCh < 32 ? maxCh : 32;
        }
      } else {
        sp.coll = info.func == FUNC_REDUCESCATTER ? 2 /*SYM_RS*/ : 3 /*SYM_AG*/;
      }
      if (n >= 3 && comm->tune.linkChannels > 0 && tunedNch == 0) maxCh = std::min(maxCh, comm->tune.linkChannels);  // CU budget
      // a tuner plugin's nChannels sets the zero-copy plan's channels too, as it does the staged plan's (the
      // reference's nMaxChannels applies whichever buffers the collective runs on, enqueue.cc:2189)
      if (tunedNch > 0) minPart = (spanBytes + tunedNch - 1) / tunedNch;
      int nch = (int)((spanBytes + minPart - 1) / minPart);
      if (nch < comm->minCTAs) nch = comm->minCTAs;
      if (nch > maxCh) nch = maxCh;
      if (nch < 1) nch = 1;
      uint64_t spanElems = spanBytes / ts;
      uint64_t part = (spanElems + nch - 1) / nch;
      part = (part + epp - 1) / epp * epp;
      if (part == 0) part = epp;
      sp.args.part = part;
      sp.nChannels = nch;
      sp.stream = info.stream;
      TRACE("%s: %s coll %d nch %d part %lu aligned %d", info.opName, regMode ? "registered zero-copy" : "symmetric",
            sp.coll, nch, (unsigned long)part, sp.args.aligned);
      return ncclSuccess;
    }
  }
  if (oneShot) {
    p.algo = ALGO_ONESHOT;
    size_t minPart = tunedNch > 0 ? (count * ts + tunedNch - 1) / tunedNch : (size_t)comm->tune.oneShotChannelBytes;
    planChannels(comm, count * ts, ts, p, minPart, 32);
  } else {
    size_t minPart = tunedNch > 0 ? (blockElems * ts + tunedNch - 1) / tunedNch : (size_t)comm->tune.minChannelBytes;
    int maxCh = comm->chanCap;
    if (n >= 3 && comm->tune.linkChannels > 0 && tunedNch == 0) maxCh = std::min(maxCh, comm->tune.linkChannels);
    planChannels(comm, blockElems * ts, ts, p, minPart, maxCh);
  }
  TRACE("%s: count %zu dt %d op %d -> nch %d part %lu slice %lu steps %d aligned %d", info.opName, count,
        (int)info.datatype, (int)info.op, p.nChannels, (unsigned long)p.args.part, (unsigned long)p.args.slice,
        p.args.nSteps, p.args.aligned);
  return ncclSuccess;
}

// Host-side guard before any channel kernel launches: its grid never exceeds the channels the staging slab, flag
// block and counters were allocated for, nor the co-resident cap (a kernel indexing past them would fault the GPU).
static ncclResult_t checkGrid(const ncclComm* comm, int kind, const LaunchPlan& p, const SymPlan& sp) {
  int grid = 0, cap = comm->chanCap;
  if (kind == PLAN_SYM) grid = sp.nChannels;
  else if (p.algo == ALGO_LL) grid = p.nChannels, cap = std::min(cap, comm->llChannels);
  else if (p.algo == ALGO_DIRECT || p.algo == ALGO_ONESHOT || p.algo == ALGO_PIPE) grid = p.nChannels;
  else return ncclSuccess;  // one-rank kernels: no channels
  if (grid >= 1 && grid <= cap && grid <= comm->maxChannels) return ncclSuccess;
  WARN("internal: a plan of %d channels (cap %d, %d allocated) was refused before launch", grid, cap, comm->maxChannels);
  return ncclInternalError;
}

static void noteLaunch(ncclComm* comm, hipStream_t stream);

ncclResult_t launchColl(const CollInfo& info, bool forkJoin) {
  ncclComm* comm = info.comm;
  HIPCHECK(hipSetDevice(comm->device));
  LaunchPlan p;
  SymPlan sp;
  int kind;
  collProgress(comm, info.stream);
  NCCLCHECK(planColl(info, p, sp, &kind));
  if (kind == PLAN_NONE) return ncclSuccess;
  NCCLCHECK(checkGrid(comm, kind, p, sp));
  // a comm sharing its GPU with other ranks of this process runs on its own hardware queue, between a fork
  // and a join (see ncclComm::internalStream)
  const bool shared =
      comm->sharedDevInProcess && !(kind == PLAN_KERNEL && (p.algo == ALGO_COPY || p.algo == ALGO_ONERANK));
  if (shared) {
    if (forkJoin) NCCLCHECK(collFork(info));
    p.stream = sp.stream = comm->internalStream;
  }
  if (kind == PLAN_SYM) {
    NCCLCHECK(sp.bounced ? bounceLaunch(comm, sp) : launchSymPlan(sp));
    regRecordUse(comm, sp);
  } else {
    NCCLCHECK(launchPlan(p));
  }
  noteLaunch(comm, kind == PLAN_SYM ? sp.stream : p.stream);
  if (shared && forkJoin) NCCLCHECK(collJoin(info));
  return ncclSuccess;
}

// A multi-process communicator's launches leave their stream's tail event (ipc.cc ipcNoteLaunch): peers' released
// mappings are unmapped on the collective path only while none of this library's kernels is in flight here.
static void noteLaunch(ncclComm* comm, hipStream_t stream) {
  if (!comm->fdServer) return;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return;  // a graph's kernels are launched by its replays, each complete on every rank independently
  }
  ipcNoteLaunch(stream, comm->device);
}

// Upkeep on the collective path, before anything of this collective is planned or launched, never waiting (VERDICT r5
// item 4): this rank's registrations (register.cc regProgress) and the peers' mappings they released (ipc.cc).
// Never while `stream` is being captured: an unmap or free there would invalidate the capture (measured round 6,
// test_graph_registrations_released_with_their_graph: hipErrorStreamCaptureInvalidated); the next collective outside
// a capture, or a blocking call, does it instead.
void collProgress(ncclComm* comm, hipStream_t stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return;
  }
  regProgress(comm);
  ipcProgressReleases();
}

// ---- group aggregation (reference: a group's ops aggregated into one kernel plan, enqueue.cc:405-470) ----
// Consecutive planned ops of one comm become one launch when they share the stream, type and operator and
// were planned onto the same kernel: LL (any mix of AllReduce / ReduceScatter / AllGather / Reduce; the LL
// kernel dispatches per op) or the staged kernel with the same collective and one-shot / direct choice
// (collBatchKernel). Every rank of a comm issues the same op sequence and plans each op alike, so every
// rank forms the same batches.
static bool sameRedOp(const LaunchPlan& a, const LaunchPlan& b) {
  return a.devOp == b.devOp && a.args.redArg == b.args.redArg && a.args.redArgPtr == b.args.redArgPtr;
}

bool batchable(const std::vector<PlannedColl>& run, const PlannedColl& b) {
  if (run.empty()) return false;
  const PlannedColl& a = run[0];
  if (a.kind != PLAN_KERNEL || b.kind != PLAN_KERNEL || a.info.comm != b.info.comm || a.info.stream != b.info.stream ||
      a.info.datatype != b.info.datatype || a.info.comm->tune.noAggregation || a.p.algo != b.p.algo)
    return false;
  if (a.p.algo == ALGO_LL) {
    if (run.size() >= (size_t)kMaxLLBatch || a.p.ll.ops[0].proto != b.p.ll.ops[0].proto) return false;
    // Broadcasts (bytes, any roots) batch with each other only: they run in the byte-typed kernel, which folds nothing
    if (a.info.func == FUNC_BROADCAST || b.info.func == FUNC_BROADCAST) return a.info.func == b.info.func;
    // AllGather folds nothing: it joins any operator (its own plan carries none)
    if (b.info.func == FUNC_ALLGATHER) return true;
    for (const PlannedColl& x : run)
      if (x.info.func != FUNC_ALLGATHER && !sameRedOp(x.p, b.p)) return false;
    return true;
  }
  if (a.p.args.cbdLo || b.p.args.cbdLo) return false;  // the reference's partition (NCCL_AMD_REF_ORDER): alone
  if (a.p.algo == ALGO_DIRECT || a.p.algo == ALGO_ONESHOT)
    return run.size() < (size_t)kMaxCollBatch && a.info.func == b.info.func && sameRedOp(a.p, b.p) &&
           a.p.args.protoFlags == b.p.args.protoFlags;
  return false;
}

static const char* const kFuncName[FUNC_KINDS] = {"AllReduce", "ReduceScatter", "AllGather", "Reduce", "Broadcast"};

// One launch for run[0..k) (batchable with each other, in order); the caller forks/joins shared-GPU comms.
ncclResult_t launchBatch(std::vector<PlannedColl>& run) {
  ncclComm* comm = run[0].info.comm;
  HIPCHECK(hipSetDevice(comm->device));
  LaunchPlan& p = run[0].p;
  if (run[0].kind == PLAN_NONE) return ncclSuccess;
  const bool shared =
      comm->sharedDevInProcess && !(run[0].kind == PLAN_KERNEL && (p.algo == ALGO_COPY || p.algo == ALGO_ONERANK));
  if (shared) p.stream = run[0].sp.stream = comm->internalStream;
  for (const PlannedColl& x : run) NCCLCHECK(checkGrid(comm, x.kind, x.p, x.sp));
  if (run.size() == 1) {
    if (run[0].kind != PLAN_SYM) {
      NCCLCHECK(launchPlan(p));
      noteLaunch(comm, p.stream);
      return ncclSuccess;
    }
    NCCLCHECK(run[0].sp.bounced ? bounceLaunch(comm, run[0].sp) : launchSymPlan(run[0].sp));
    regRecordUse(comm, run[0].sp);
    noteLaunch(comm, run[0].sp.stream);
    return ncclSuccess;
  }
  if (p.algo == ALGO_LL) {
    int off = p.ll.ops[0].nch % comm->llChannels, used = p.ll.ops[0].nch;
    for (size_t k = 1; k < run.size(); k++) {
      LLOp& o = p.ll.ops[k];
      o = run[k].p.ll.ops[0];
      o.chOff = off;
      off = (off + o.nch) % comm->llChannels;
      used += o.nch;
      // the batch kernel is typed by its folding ops; AllGather runs in any element type of its size
      if (p.func == FUNC_ALLGATHER && run[k].info.func != FUNC_ALLGATHER) {
        p.func = run[k].info.func;
        p.devOp = run[k].p.devOp;
        p.ll.redArg = run[k].p.ll.redArg;
        p.ll.redArgPtr = run[k].p.ll.redArgPtr;
      }
    }
    p.ll.nOps = (int)run.size();
    p.nChannels = used < comm->llChannels ? used : comm->llChannels;
    // per channel, the ops it runs (the kernel walks these bits in batch order)
    std::fill(p.ll.chMask, p.ll.chMask + kMaxLLChannels, 0u);
    for (int k = 0; k < p.ll.nOps; k++)
      for (int j = 0; j < p.ll.ops[k].nch; j++) p.ll.chMask[(p.ll.ops[k].chOff + j) % comm->llChannels] |= 1u << k;
    TRACE("LL batch: %d ops (first %s), %d channels", p.ll.nOps, kFuncName[run[0].info.func], p.nChannels);
    NCCLCHECK(launchPlan(p));
    noteLaunch(comm, p.stream);
    return ncclSuccess;
  }
  CollBatchArgs& b = p.batch;
  int off = 0, used = 0;
  for (size_t k = 0; k < run.size(); k++) {
    b.op[k] = run[k].p.args;
    b.nch[k] = run[k].p.nChannels;
    b.chOff[k] = off;
    off = (off + b.nch[k]) % comm->chanCap;
    used += b.nch[k];
  }
  b.nOps = (int)run.size();
  p.nChannels = used < comm->chanCap ? used : comm->chanCap;
  TRACE("staged batch: %d %s ops (%s), %d channels", b.nOps, kFuncName[run[0].info.func],
        p.algo == ALGO_ONESHOT ? "one-shot" : "direct", p.nChannels);
  NCCLCHECK(launchPlan(p));
  noteLaunch(comm, p.stream);
  return ncclSuccess;
}

// Fork / join of a shared-GPU comm's internal stream with the caller's stream. A group issues every
// fork, then every launch, then every join: a join makes the user stream wait for the collective, and
// if two ranks' user streams share a hardware queue, a join enqueued before the peer's fork would
// hold that fork (and with it the peer's kernel) behind our unfinished kernel.
ncclResult_t collFork(const CollInfo& info) {
  ncclComm* comm = info.comm;
  if (!comm->sharedDevInProcess) return ncclSuccess;
  HIPCHECK(hipSetDevice(comm->device));
  HIPCHECK(hipEventRecord(comm->evIn, info.stream));
  HIPCHECK(hipStreamWaitEvent(comm->internalStream, comm->evIn, 0));
  return ncclSuccess;
}

ncclResult_t collJoin(const CollInfo& info) {
  ncclComm* comm = info.comm;
  if (!comm->sharedDevInProcess) return ncclSuccess;
  HIPCHECK(hipSetDevice(comm->device));
  HIPCHECK(hipEventRecord(comm->evOut, comm->internalStream));
  HIPCHECK(hipStreamWaitEvent(info.stream, comm->evOut, 0));
  return ncclSuccess;
}

ncclResult_t enqueueCheck(CollInfo* info) {
  logInit();
  // reference NVTX payload (collectives.cc:134,170): the comm and the message size
  ROCTX_RANGE("nccl%s comm=%p count=%zu datatype=%d op=%d root=%d", info->opName, (void*)info->comm, info->count,
              (int)info->datatype, (int)info->op, info->root);
  ncclResult_t ret = commCheck(info->comm, info->opName, "comm");
  if (ret != ncclSuccess) {
    groupRecordError(ret);
    return ret;
  }
  // (no ipcDrainReleases here: unmapping a peer's deregistered buffer is a device-synchronising hipFree, and a
  // collective must return once its work is enqueued, nccl.h.in:431-442; launchColl / the group end unmap only while
  // none of the library's kernels is in flight, collProgress, and the blocking entry points drain, ipc.cc)
  ret = argsCheck(info);
  // A kernel of this comm recorded a device error (spin timeout, abort, kernel mismatch): its peers' handshake state no
  // longer matches this rank's, and a zero-copy kernel would read peer pointers of some earlier collective — launch
  // nothing more (the reference's comm is equally unusable after an async error; its kernels, though, hang rather
  // than touch stale mappings)
  commPollAsync(info->comm);
  if (ret == ncclSuccess && info->comm->asyncResult.load() != ncclSuccess) {
    WARN("%s: communicator is in error state %d", info->opName, info->comm->asyncResult.load());
    ret = ncclInvalidUsage;
  }
  if (ret != ncclSuccess) {
    groupRecordError(ret);
    return ret;
  }
  INFO("%s: opCount %lx sendbuff %p recvbuff %p count %zu datatype %d op %d root %d comm %p [nranks=%d] stream %p",
       info->opName, (unsigned long)info->comm->opCount, info->sendbuff, info->recvbuff, info->count,
       (int)info->datatype, (int)info->op, info->root, (void*)info->comm, info->comm->nRanks, (void*)info->stream);
  if (info->count == 0) return ncclSuccess;  // reference enqueue.cc:3024
  if (groupActive()) return groupDeferColl(*info);
  // the caller's current device survives the call, as in the reference (an eager call is a one-op group
  // whose launch saves and restores the device: enqueue.cc:3137-3162, group.cc:860-863)
  DeviceRestore restore;
  return launchColl(*info);
}

// ---- small host conversions for the avg scalar ----
static uint16_t hostF32ToHalf(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
static uint16_t hostF32ToBf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1);
  return (uint16_t)(u >> 16);
}
static uint8_t hostF32ToFp8(float f, bool e5m2) {
  // 1/n for n in 1..16 is well inside both fp8 ranges: round via half, then RNE to 3/2 mantissa bits
  float h = (float)(_Float16)f;
  uint32_t u;
  memcpy(&u, &h, 4);
  int mbits = e5m2 ? 2 : 3, bias = e5m2 ? 15 : 7;
  int e = (int)((u >> 23) & 0xff) - 127;
  uint32_t man = u & 0x7fffff;
  if (e < 1 - bias) {  // subnormal fp8
    float q = h * (e5m2 ? 65536.0f : 512.0f);
    uint32_t qi = (uint32_t)q;
    float fr = q - (float)qi;
    if (fr > 0.5f || (fr == 0.5f && (qi & 1))) qi++;
    return (uint8_t)qi;
  }
  uint32_t code = ((uint32_t)(e + bias) << mbits) | (man >> (23 - mbits));
  uint32_t rem = man & ((1u << (23 - mbits)) - 1), halfway = 1u << (22 - mbits);
  if (rem > halfway || (rem == halfway && (code & 1))) code++;
  return (uint8_t)code;
}

}  // namespace ncclamd

using namespace ncclamd;

#define NCCL_ALIAS(ret, name, ...) extern "C" __attribute__((visibility("default"), alias(#name))) ret p##name(__VA_ARGS__);

NCCL_EXPORT ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                                       ncclRedOp_t op, ncclComm_t comm, hipStream_t stream) {
  CollInfo info = {FUNC_ALLREDUCE, "AllReduce", sendbuff, recvbuff, count, datatype, op, 0, comm, stream};
  return enqueueCheck(&info);
}
NCCL_ALIAS(ncclResult_t, ncclAllReduce, const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
           hipStream_t)

NCCL_EXPORT ncclResult_t ncclReduceScatter(const void* sendbuff, void* recvbuff, size_t recvcount,
                                           ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                                           hipStream_t stream) {
  CollInfo info = {FUNC_REDUCESCATTER, "ReduceScatter", sendbuff, recvbuff, recvcount, datatype, op, 0, comm, stream};
  return enqueueCheck(&info);
}
NCCL_ALIAS(ncclResult_t, ncclReduceScatter, const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
           hipStream_t)

NCCL_EXPORT ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount,
                                       ncclDataType_t datatype, ncclComm_t comm, hipStream_t stream) {
  CollInfo info = {FUNC_ALLGATHER, "AllGather", sendbuff, recvbuff, sendcount, datatype, ncclSum, 0, comm, stream};
  return enqueueCheck(&info);
}
NCCL_ALIAS(ncclResult_t, ncclAllGather, const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t)

NCCL_EXPORT ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                                    ncclRedOp_t op, int root, ncclComm_t comm, hipStream_t stream) {
  CollInfo info = {FUNC_REDUCE, "Reduce", sendbuff, recvbuff, count, datatype, op, root, comm, stream};
  return enqueueCheck(&info);
}
NCCL_ALIAS(ncclResult_t, ncclReduce, const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t,
           hipStream_t)

// Broadcast (reference collectives.cc:180-207): the payload moves as bytes, the datatype normalised to one byte
// (reference enqueue.cc:2733-2736), so Broadcasts of any types batch and one byte-typed kernel serves them all.
// An invalid datatype is left as it is for argsCheck to refuse.
NCCL_EXPORT ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                                       int root, ncclComm_t comm, hipStream_t stream) {
  const int ts = (int)datatype >= 0 && datatype < ncclNumTypes ? typeSize(datatype) : -1;
  if (ts > 0) count *= (size_t)ts, datatype = ncclInt8;
  CollInfo info = {FUNC_BROADCAST, "Broadcast", sendbuff, recvbuff, count, datatype, ncclSum, root, comm, stream};
  return enqueueCheck(&info);
}
NCCL_ALIAS(ncclResult_t, ncclBroadcast, const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)

NCCL_EXPORT ncclResult_t ncclBcast(void* buff, size_t count, ncclDataType_t datatype, int root, ncclComm_t comm,
                                   hipStream_t stream) {
  return ncclBroadcast(buff, buff, count, datatype, root, comm, stream);
}
NCCL_ALIAS(ncclResult_t, ncclBcast, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t)
