// bootstrap.cc — out-of-band rendezvous for ncclCommInitRank (one node).
//
// Reference: src/bootstrap.cc:405-462 (root listener created by ncclGetUniqueId, address carried in
// the 128-byte ncclUniqueId), :674-884 (bootstrapInit), :1194 (bootstrapAllGather), bootstrapBarrier.
// The reference builds a socket ring between ranks so it scales to thousands of nodes. This engine
// is intra-node only (≤ 8 GPUs of one MI355X node), so the root thread stays alive as a
// star: every rank keeps one TCP connection to it and each collective round is "the participating
// ranks send their block, the root returns the concatenation". Only init-time metadata travels here
// (peer info + HIP IPC handles), the destroy barrier and the rendezvous of ncclCommSplit /
// ncclCommShrink; nothing on the data path.
#include <arpa/inet.h>
#include <errno.h>
#include <fcntl.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <random>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "split.h"

namespace ncclamd {

static constexpr uint64_t kIdMagic = 0x424f4f5453545250ull;  // "BOOTSTRP"

struct IdPayload {  // lives inside ncclUniqueId::internal (128 bytes)
  uint64_t magic;
  uint64_t commId;
  struct sockaddr_in addr;
};
static_assert(sizeof(IdPayload) <= NCCL_UNIQUE_ID_BYTES, "unique id payload too large");

struct Hello {
  uint64_t magic;
  uint64_t commId;
  int32_t rank;
  int32_t nranks;
};

struct Bootstrap {
  int fd = -1;
  int rank = 0;
  int nranks = 0;
};

static bool sendAll(int fd, const void* p, size_t n) {
  const char* c = (const char*)p;
  while (n) {
    ssize_t k = ::send(fd, c, n, MSG_NOSIGNAL);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return false;
    c += k;
    n -= (size_t)k;
  }
  return true;
}
// returns 1 ok, 0 clean EOF before any byte, -1 error
static int recvAll(int fd, void* p, size_t n) {
  char* c = (char*)p;
  size_t got = 0;
  while (got < n) {
    ssize_t k = ::recv(fd, c + got, n - got, 0);
    if (k < 0 && errno == EINTR) continue;
    if (k == 0) return got == 0 ? 0 : -1;
    if (k < 0) return -1;
    got += (size_t)k;
  }
  return 1;
}

static int64_t bootstrapTimeoutMs() { return paramInt("NCCL_AMD_BOOTSTRAP_TIMEOUT_MS", 600000); }

// Hello.rank of a release message (ncclCommInitRankScalable): the root is not needed, exit.
static constexpr int32_t kReleaseRank = -1;

// One round's request as a rank sends it: the block size, the ranks taking part (bit r = rank r) and whether the
// round is a subset round, which the root bounds with the bootstrap timeout (a full round waits like a barrier does).
struct RoundHdr {
  uint64_t bytes;
  uint32_t mask;
  uint32_t subset;
};
static constexpr uint64_t kRoundOk = 0, kRoundFailed = 1;
static constexpr uint64_t kMaxBlockBytes = 64ull << 20;

static std::atomic<int> gLiveRoots{0};
int bootstrapLiveRoots() { return gLiveRoots.load(); }

// The rounds of one root, once every rank has connected. A round completes when every rank its mask names has sent a
// request with that mask and block size; the participants then get the blocks in rank order. A rank that hangs up
// leaves the service running for the others (ncclCommShrink goes on without it): only a round that names it fails,
// on every participant, as does a round whose participants disagree on the mask or the block size, or a subset round
// still incomplete after the bootstrap timeout. The ranks' sockets are polled, so a rank that sends nothing holds up
// only the rounds that name it. Ends when every rank has hung up.
static void serveRounds(std::vector<int>& fds) {
  using Clock = std::chrono::steady_clock;
  const int nranks = (int)fds.size();
  struct Pending {
    bool has = false;
    RoundHdr h = {};
    std::vector<char> block;
    Clock::time_point at;
  };
  std::vector<Pending> pend(nranks);
  const auto limit = std::chrono::milliseconds(bootstrapTimeoutMs());
  auto depart = [&](int r) {
    close(fds[r]);
    fds[r] = -1;
    pend[r].has = false;
  };
  auto reply = [&](int r, uint64_t status, const std::vector<char>* all) {
    pend[r].has = false;
    if (!sendAll(fds[r], &status, sizeof(status)) || (all && !all->empty() && !sendAll(fds[r], all->data(), all->size())))
      depart(r);
  };
  // settle one round that can be decided; false when none can
  auto settle = [&]() {
    for (int r = 0; r < nranks; r++) {
      if (!pend[r].has) continue;
      const uint32_t mask = pend[r].h.mask;
      bool bad = !((mask >> r) & 1) || (nranks < 32 && (mask >> nranks) != 0), waiting = false;
      for (int q = 0; q < nranks && !bad; q++) {
        if (!((mask >> q) & 1)) continue;
        if (fds[q] < 0) bad = true;
        else if (!pend[q].has) waiting = true;
        else if (pend[q].h.mask != mask || pend[q].h.bytes != pend[r].h.bytes) bad = true;
      }
      if (!bad && waiting && pend[r].h.subset && Clock::now() - pend[r].at > limit) bad = true;
      if (!bad && waiting) continue;
      if (bad) {
        WARN("bootstrap root: round of mask 0x%x fails (a rank it names left, the participants disagree, or it timed out)",
             mask);
        for (int q = 0; q < nranks; q++)
          if (pend[q].has && (q == r || ((mask >> q) & 1))) reply(q, kRoundFailed, nullptr);
        return true;
      }
      std::vector<char> all;
      for (int q = 0; q < nranks; q++)
        if ((mask >> q) & 1) all.insert(all.end(), pend[q].block.begin(), pend[q].block.end());
      for (int q = 0; q < nranks; q++)
        if ((mask >> q) & 1) reply(q, kRoundOk, &all);
      return true;
    }
    return false;
  };
  while (true) {
    while (settle()) {}
    std::vector<struct pollfd> pfds;
    std::vector<int> who;
    int live = 0;
    for (int r = 0; r < nranks; r++) {
      if (fds[r] < 0) continue;
      live++;
      if (pend[r].has) continue;
      pfds.push_back({fds[r], POLLIN, 0});
      who.push_back(r);
    }
    if (!live) return;
    int waitMs = -1;  // until the earliest deadline of a pending subset round
    for (int r = 0; r < nranks; r++) {
      if (!pend[r].has || !pend[r].h.subset) continue;
      int64_t left = std::chrono::duration_cast<std::chrono::milliseconds>(pend[r].at + limit - Clock::now()).count() + 1;
      if (left < 0) left = 0;
      if (waitMs < 0 || left < waitMs) waitMs = (int)left;
    }
    if (pfds.empty() && waitMs < 0) return;  // nothing can arrive and nothing times out
    int pr = poll(pfds.data(), pfds.size(), waitMs);
    if (pr < 0 && errno != EINTR) return;
    for (size_t i = 0; pr > 0 && i < pfds.size(); i++) {
      if (!(pfds[i].revents & (POLLIN | POLLHUP | POLLERR))) continue;
      const int r = who[i];
      Pending& p = pend[r];
      if (recvAll(fds[r], &p.h, sizeof(p.h)) != 1 || p.h.bytes > kMaxBlockBytes) {
        depart(r);  // hung up (or sent garbage): the others carry on
        continue;
      }
      p.block.resize(p.h.bytes);
      if (p.h.bytes && recvAll(fds[r], p.block.data(), p.h.bytes) != 1) {
        depart(r);
        continue;
      }
      p.has = true;
      p.at = Clock::now();
    }
  }
}

// Root service: accept nranks connections, then serve all-gather rounds until every rank hangs up.
static void rootThread(int listenFd, uint64_t commId) {
  std::vector<int> fds;
  int nranks = -1;
  auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(bootstrapTimeoutMs());
  while (true) {  // until every rank has said hello
    struct pollfd pfd = {listenFd, POLLIN, 0};
    int left = (int)std::chrono::duration_cast<std::chrono::milliseconds>(deadline - std::chrono::steady_clock::now()).count();
    if (left <= 0) { WARN("bootstrap root: timed out waiting for ranks"); goto done; }
    int pr = poll(&pfd, 1, left);
    if (pr <= 0) continue;
    int fd = accept(listenFd, nullptr, nullptr);
    if (fd < 0) continue;
    Hello h;
    const bool got = recvAll(fd, &h, sizeof(h)) == 1;
    if (got && h.magic == kIdMagic && h.commId == commId && h.rank == kReleaseRank && nranks < 0) {
      close(fd);  // an unused id of ncclCommInitRankScalable: no rank will connect here
      goto done;
    }
    if (!got || h.magic != kIdMagic || h.commId != commId || h.nranks <= 0 || h.nranks > 32 ||
        h.rank < 0 || h.rank >= h.nranks || (nranks >= 0 && h.nranks != nranks)) {
      WARN("bootstrap root: rejected connection (bad hello)");
      close(fd);
      continue;
    }
    if (nranks < 0) { nranks = h.nranks; fds.assign(nranks, -1); }
    if (fds[h.rank] != -1) { WARN("bootstrap root: duplicate rank %d", h.rank); close(fd); continue; }
    int one = 1;
    setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
    fds[h.rank] = fd;
    int connected = 0;
    for (int f : fds) connected += (f != -1);
    if (connected == nranks) break;
  }
  serveRounds(fds);
done:
  for (int f : fds)
    if (f >= 0) close(f);
  close(listenFd);
  gLiveRoots.fetch_sub(1);
}

ncclResult_t bootstrapGetUniqueId(ncclUniqueId* id) {
  memset(id, 0, sizeof(*id));
  IdPayload p;
  memset(&p, 0, sizeof(p));
  p.magic = kIdMagic;
  std::random_device rd;
  p.commId = ((uint64_t)rd() << 32) ^ rd() ^ (uint64_t)getpid();
  int fd = socket(AF_INET, SOCK_STREAM, 0);
  SYSCHECK(fd >= 0, "socket");
  struct sockaddr_in a;
  memset(&a, 0, sizeof(a));
  a.sin_family = AF_INET;
  const char* ip = paramStr("NCCL_AMD_BOOTSTRAP_ADDR");  // intra-node: loopback by default
  if (inet_pton(AF_INET, ip ? ip : "127.0.0.1", &a.sin_addr) != 1) {
    close(fd);
    WARN("bad NCCL_AMD_BOOTSTRAP_ADDR %s", ip);
    return ncclInvalidArgument;
  }
  a.sin_port = 0;
  if (bind(fd, (struct sockaddr*)&a, sizeof(a)) != 0 || listen(fd, 128) != 0) {
    close(fd);
    WARN("bootstrap: bind/listen failed: %s", strerror(errno));
    return ncclSystemError;
  }
  socklen_t len = sizeof(a);
  getsockname(fd, (struct sockaddr*)&a, &len);
  p.addr = a;
  memcpy(id->internal, &p, sizeof(p));
  gLiveRoots.fetch_add(1);
  std::thread(rootThread, fd, p.commId).detach();
  INFO("bootstrap root listening on %s:%d", inet_ntoa(a.sin_addr), ntohs(a.sin_port));
  return ncclSuccess;
}

ncclResult_t bootstrapInit(const ncclUniqueId* id, int rank, int nranks, Bootstrap** out) {
  IdPayload p;
  memcpy(&p, id->internal, sizeof(p));
  if (p.magic != kIdMagic) {
    WARN("ncclCommInitRank: invalid ncclUniqueId (was it produced by ncclGetUniqueId?)");
    return ncclInvalidArgument;
  }
  auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(bootstrapTimeoutMs());
  int fd = -1;
  while (true) {
    fd = socket(AF_INET, SOCK_STREAM, 0);
    SYSCHECK(fd >= 0, "socket");
    if (connect(fd, (struct sockaddr*)&p.addr, sizeof(p.addr)) == 0) break;
    int err = errno;
    close(fd);
    fd = -1;
    if (std::chrono::steady_clock::now() > deadline) {
      WARN("bootstrap: connect to root failed: %s", strerror(err));
      return ncclRemoteError;
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
  }
  int one = 1;
  setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
  Hello h = {kIdMagic, p.commId, rank, nranks};
  if (!sendAll(fd, &h, sizeof(h))) {
    close(fd);
    WARN("bootstrap: hello failed");
    return ncclRemoteError;
  }
  Bootstrap* b = new Bootstrap;
  b->fd = fd;
  b->rank = rank;
  b->nranks = nranks;
  *out = b;
  return ncclSuccess;
}

// ncclCommInitRankScalable hands every rank nId ids (reference bootstrap.cc:59-89 spreads the ranks over
// nId roots). This engine's star needs one root, so every rank rendezvouses at id 0 and the first rank of
// each other id's rank group (the reference's block partition, rootIdFromRank) tells that id's root to
// exit instead of waiting for ranks that never come. Bounded like every bootstrap connect.
ncclResult_t bootstrapRelease(const ncclUniqueId* id) {
  IdPayload p;
  memcpy(&p, id->internal, sizeof(p));
  if (p.magic != kIdMagic) {
    WARN("ncclCommInitRankScalable: invalid ncclUniqueId (was it produced by ncclGetUniqueId?)");
    return ncclInvalidArgument;
  }
  auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(bootstrapTimeoutMs());
  while (true) {
    int fd = socket(AF_INET, SOCK_STREAM, 0);
    SYSCHECK(fd >= 0, "socket");
    if (connect(fd, (struct sockaddr*)&p.addr, sizeof(p.addr)) == 0) {
      Hello h = {kIdMagic, p.commId, kReleaseRank, 0};
      bool ok = sendAll(fd, &h, sizeof(h));
      close(fd);
      if (ok) return ncclSuccess;
    } else {
      close(fd);
    }
    if (std::chrono::steady_clock::now() > deadline) {
      WARN("bootstrap: could not release an unused root");
      return ncclRemoteError;
    }
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
  }
}

// Root of rank r when nranks ranks are spread over nRoots ids (reference bootstrap.cc:59-69, offset 0).
static int rootIdFromRank(int r, int nranks, int nRoots) {
  const int rmr = nranks % nRoots, rpr = nranks / nRoots, D = rmr * (rpr + 1);
  return r < D ? r / (rpr + 1) : (r - D) / rpr + rmr;
}

// Each id k >= 1 is released by exactly one rank: the first rank of root k's group, or rank k % nranks
// for an id no rank maps to (nId > nranks). An id listed twice is one root (still in use if it equals id 0).
ncclResult_t bootstrapReleaseUnused(const ncclUniqueId* ids, int nId, int rank, int nranks) {
  for (int k = 1; k < nId; k++) {
    bool dup = false;
    for (int j = 0; j < k && !dup; j++) dup = memcmp(&ids[j], &ids[k], sizeof(ncclUniqueId)) == 0;
    if (dup) continue;
    int releaser = k % nranks;
    for (int r = 0; r < nranks; r++)
      if (rootIdFromRank(r, nranks, nId) == k) {
        releaser = r;
        break;
      }
    if (releaser == rank) NCCLCHECK(bootstrapRelease(&ids[k]));
  }
  return ncclSuccess;
}

// One round: this rank's block goes to the root, which answers with a status word and, when the round completed, the
// blocks of the ranks in `mask` in rank order.
static ncclResult_t bootstrapRound(Bootstrap* b, uint32_t mask, bool subset, const void* mine, void* out, size_t bytes) {
  RoundHdr h = {bytes, mask, subset ? 1u : 0u};
  if (!sendAll(b->fd, &h, sizeof(h)) || (bytes && !sendAll(b->fd, mine, bytes))) {
    WARN("bootstrap allgather: send failed (the process hosting the root exited?)");
    return ncclRemoteError;
  }
  uint64_t status = kRoundFailed;
  if (recvAll(b->fd, &status, sizeof(status)) != 1) {
    WARN("bootstrap allgather: recv failed (a peer exited?)");
    return ncclRemoteError;
  }
  if (status != kRoundOk) {
    WARN("bootstrap allgather: the round of mask 0x%x failed at the root (a rank it names left or never joined, or the "
         "participants disagree)", mask);
    return ncclRemoteError;
  }
  if (bytes && recvAll(b->fd, out, bytes * (size_t)__builtin_popcount(mask)) != 1) {
    WARN("bootstrap allgather: recv failed (a peer exited?)");
    return ncclRemoteError;
  }
  return ncclSuccess;
}

static uint32_t fullMask(int nranks) { return nranks >= 32 ? 0xffffffffu : (1u << nranks) - 1; }

// data holds nranks blocks of bytesPerRank; this rank's block (index rank) is sent, all are received.
ncclResult_t bootstrapAllGather(Bootstrap* b, void* data, size_t bytesPerRank) {
  char* d = (char*)data;
  return bootstrapRound(b, fullMask(b->nranks), false, d + (size_t)b->rank * bytesPerRank, d, bytesPerRank);
}

// The same among the ranks of `mask` only (this rank among them): data holds one block per participant in rank order.
// Ranks outside the mask take no part and may be gone; the root fails the round with ncclRemoteError on every
// participant if a rank it names has left, if the participants name different masks, or if it is still incomplete
// after NCCL_AMD_BOOTSTRAP_TIMEOUT_MS.
ncclResult_t bootstrapAllGatherSubset(Bootstrap* b, uint32_t mask, void* data, size_t bytesPerRank) {
  if (!((mask >> b->rank) & 1) || (mask & ~fullMask(b->nranks))) {
    WARN("bootstrap subset round: mask 0x%x does not fit rank %d of %d", mask, b->rank, b->nranks);
    return ncclInvalidArgument;
  }
  const int at = __builtin_popcount(mask & ((1u << b->rank) - 1));
  char* d = (char*)data;
  return bootstrapRound(b, mask, true, d + (size_t)at * bytesPerRank, d, bytesPerRank);
}

ncclResult_t bootstrapBarrier(Bootstrap* b) {
  std::vector<char> tmp(b->nranks);
  return bootstrapAllGather(b, tmp.data(), 1);
}

// ncclCommSplit's rendezvous over the parent's star (reference init.cc commGetSplitInfo + the child's own bootstrap):
// every parent rank, NCCL_SPLIT_NOCOLOR ones included, joins two full rounds — the (color, key) pairs, then the ids
// that each child's rank 0 created in between. *childRanks == 0: no child for this rank.
ncclResult_t bootstrapSplit(Bootstrap* b, int color, int key, ncclUniqueId* id, int* childRank, int* childRanks,
                            std::vector<int>* members) {
  const int n = b->nranks;
  std::vector<int> ck(2 * n, 0);
  ck[2 * b->rank] = color;
  ck[2 * b->rank + 1] = key;
  NCCLCHECK(bootstrapAllGather(b, ck.data(), 2 * sizeof(int)));
  std::vector<int> colors(n), keys(n);
  for (int r = 0; r < n; r++) {
    colors[r] = ck[2 * r];
    keys[r] = ck[2 * r + 1];
  }
  std::vector<int> mem;
  if (color != NCCL_SPLIT_NOCOLOR) mem = splitMembers(colors.data(), keys.data(), n, color);
  std::vector<ncclUniqueId> ids(n);
  memset(ids.data(), 0, n * sizeof(ncclUniqueId));
  ncclResult_t res = ncclSuccess;
  if (!mem.empty() && mem[0] == b->rank) res = bootstrapGetUniqueId(&ids[b->rank]);
  // a rank whose id could not be made still joins the round: its child's members then see a zeroed id and fail
  NCCLCHECK(bootstrapAllGather(b, ids.data(), sizeof(ncclUniqueId)));
  NCCLCHECK(res);
  *childRanks = (int)mem.size();
  *childRank = 0;
  for (size_t i = 0; i < mem.size(); i++)
    if (mem[i] == b->rank) *childRank = (int)i;
  if (!mem.empty()) *id = ids[mem[0]];
  if (members) *members = mem;
  return ncclSuccess;
}

// ncclCommShrink's rendezvous: one subset round among the surviving ranks (the excluded ones do not call and may be
// dead), carrying the id the lowest surviving rank created. Needs the process that hosts the parent's root alive.
ncclResult_t bootstrapShrink(Bootstrap* b, uint32_t excludeMask, ncclUniqueId* id, int* childRank, int* childRanks) {
  const uint32_t mask = fullMask(b->nranks) & ~excludeMask;
  if (!((mask >> b->rank) & 1)) return ncclInvalidArgument;
  const int cn = __builtin_popcount(mask);
  const int cr = __builtin_popcount(mask & ((1u << b->rank) - 1));
  std::vector<ncclUniqueId> ids(cn);
  memset(ids.data(), 0, cn * sizeof(ncclUniqueId));
  ncclResult_t res = ncclSuccess;
  if (cr == 0) res = bootstrapGetUniqueId(&ids[0]);
  NCCLCHECK(bootstrapAllGatherSubset(b, mask, ids.data(), sizeof(ncclUniqueId)));
  NCCLCHECK(res);
  *id = ids[0];
  *childRank = cr;
  *childRanks = cn;
  return ncclSuccess;
}

// In-process all-gather for the comms of one ncclCommInitAll (no sockets: they share this object).
// Two generation-counted barriers per round: all blocks are in, then all copies are out, so a fast rank
// cannot start the next round while a slow one still reads this one.
struct LocalClique {
  std::mutex m;
  std::condition_variable cv;
  int n = 0;
  int arrived = 0;
  uint64_t gen = 0;
  std::vector<char> buf;
};

std::shared_ptr<LocalClique> cliqueCreate(int nranks) {
  auto c = std::make_shared<LocalClique>();
  c->n = nranks;
  return c;
}

static void cliqueBarrier(LocalClique* c, std::unique_lock<std::mutex>& lk, int expected) {
  uint64_t g = c->gen;
  if (++c->arrived == expected) {
    c->arrived = 0;
    c->gen++;
    c->cv.notify_all();
  } else {
    c->cv.wait(lk, [&] { return c->gen != g; });
  }
}

// `expected` of the n ranks call (ncclCommShrink: the others are excluded); their blocks read as zeros.
ncclResult_t cliqueAllGatherAmong(LocalClique* c, int rank, void* data, size_t bytesPerRank, int expected) {
  std::unique_lock<std::mutex> lk(c->m);
  if (c->buf.size() < bytesPerRank * c->n) c->buf.resize(bytesPerRank * c->n);
  // the round's first arriver (every copy of the round before is out: its second barrier has closed)
  if (c->arrived == 0 && expected != c->n) memset(c->buf.data(), 0, bytesPerRank * c->n);
  memcpy(c->buf.data() + (size_t)rank * bytesPerRank, (char*)data + (size_t)rank * bytesPerRank, bytesPerRank);
  cliqueBarrier(c, lk, expected);
  memcpy(data, c->buf.data(), bytesPerRank * c->n);
  cliqueBarrier(c, lk, expected);
  return ncclSuccess;
}

ncclResult_t cliqueAllGather(LocalClique* c, int rank, void* data, size_t bytesPerRank) {
  return cliqueAllGatherAmong(c, rank, data, bytesPerRank, c->n);
}

void bootstrapClose(Bootstrap* b) {
  if (!b) return;
  if (b->fd >= 0) close(b->fd);
  delete b;
}

}  // namespace ncclamd
