// CPU sweep of the host and pure functions of include/nccl_device_ll_a2a.h: a stand-alone program, built under
// ASan+UBSan (tests/test_device_lla2a_cpu.py runs it). Prints "checks=<n> OK" or the first failure.
#include <stdio.h>
#include <string.h>

#include "nccl_device.h"

static long checks = 0;
#define CHECK(cond) \
  do { checks++; if (!(cond)) { printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

int main() {
  for (int elts = 0; elts <= 40; elts++)  // one line per 8 bytes of a value
    for (int size = 1; size <= 64; size++) CHECK(ncclLLA2ACalcSlots(elts, size) == elts * ((size + 7) / 8));
  // the requirement: size, alignment, handle wiring, everything else zero; the slot offsets: the epoch line, the even
  // and the odd slots of every block are disjoint, in this order, and fill the buffer exactly
  for (int nBlocks = 1; nBlocks <= 9; nBlocks++)
    for (int nSlots = 1; nSlots <= 33; nSlots++) {
      ncclLLA2AHandle_t h;
      ncclDevResourceRequirements_t req, zero;
      memset(&h, 0xab, sizeof(h));
      memset(&req, 0xab, sizeof(req));
      memset(&zero, 0, sizeof(zero));
      CHECK(ncclLLA2ACreateRequirement(nBlocks, nSlots, &h, &req) == ncclSuccess);
      CHECK(req.bufferSize == (size_t)nBlocks * (1 + 2 * nSlots) * 16 && req.bufferAlign == 16);
      CHECK(req.outBufferHandle == &h.bufHandle && h.nSlots == (uint32_t)nSlots);
      req.bufferSize = req.bufferAlign = 0;
      req.outBufferHandle = nullptr;
      CHECK(memcmp(&req, &zero, sizeof(req)) == 0);
      uint32_t next = 0;  // the first line not yet accounted for: the next block's epoch line
      for (int b = 0; b < nBlocks; b++) {
        const uint32_t even = ncclLLA2ASlotOffset(b, nSlots, 0xFFFFFFFEu), odd = ncclLLA2ASlotOffset(b, nSlots, 0xFFFFFFFFu);
        CHECK(even == next + 1 && odd == even + (uint32_t)nSlots);
        CHECK(ncclLLA2ASlotOffset(b, nSlots, 2) == even && ncclLLA2ASlotOffset(b, nSlots, 7) == odd);
        next = odd + nSlots;
      }
      CHECK((size_t)next * 16 == (size_t)nBlocks * (1 + 2 * nSlots) * 16);
    }
  // the next epoch: +1 away from the wrap; ...FE -> ...FF -> 2; never 0 or 1; the parity always alternates
  for (uint32_t e : {2u, 1000u, 0x7FFFFFF0u, 0xFFFFFF00u})
    for (int k = 0; k < 600; k++) {
      const uint32_t nx = ncclLLA2ANextEpoch(e);
      CHECK(nx != 0 && nx != 1 && (nx & 1) != (e & 1) && (e == 0xFFFFFFFFu ? nx == 2 : nx == e + 1));
      e = nx;
    }
  CHECK(ncclLLA2ANextEpoch(0xFFFFFFFEu) == 0xFFFFFFFFu && ncclLLA2ANextEpoch(0xFFFFFFFFu) == 2u);
  printf("checks=%ld OK\n", checks);
  return 0;
}
