// mraft_abi_fanin.hip — the RCCL fan-in's entry points (include/mraft.h;
// DESIGN.md §8e): the communicator, the status allgather and the fan-in
// stream. The only unit that uses RCCL; the fan-in's CU reservation is queue
// management and lives with the handle (mraft_engine.hip).
#include <rccl/rccl.h>

#include <cstring>

#include "mraft_engine.h"

using namespace mraft::host;

namespace {

#define NCCL_TRY(expr)                                                                  \
  do {                                                                                  \
    ncclResult_t r_ = (expr);                                                           \
    if (r_ != ncclSuccess)                                                              \
      return fail(MRAFT_E_HIP, "%s failed: %s", #expr, ncclGetErrorString(r_));         \
  } while (0)

int fanin_stream_of(mraft_engine *h, hipStream_t *out) {
  if (h->fanin_masked) {
    *out = h->fanin_masked;
    return MRAFT_OK;
  }
  if (!h->fanin_own) HIP_TRY(hipStreamCreateWithFlags(&h->fanin_own, hipStreamNonBlocking));
  *out = h->fanin_own;
  return MRAFT_OK;
}

}  // namespace

extern "C" {

int mraft_comm_unique_id(uint8_t out[MRAFT_COMM_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) == MRAFT_COMM_ID_BYTES, "RCCL unique id size");
  if (!out) return fail(MRAFT_E_INVAL, "out is null");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  std::memcpy(out, &id, sizeof id);
  return MRAFT_OK;
}

int mraft_comm_init(mraft_engine *h, int32_t nranks, int32_t rank, const uint8_t id[MRAFT_COMM_ID_BYTES],
                    void **out_comm) {
  TRY(enter_handle(h));
  if (!id || !out_comm) return fail(MRAFT_E_INVAL, "null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(MRAFT_E_INVAL, "bad rank %d of %d", rank, nranks);
  *out_comm = nullptr;
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof uid);
  ncclComm_t c = nullptr;
  NCCL_TRY(ncclCommInitRank(&c, nranks, uid, rank));
  *out_comm = (void *)c;
  return MRAFT_OK;
}

int mraft_comm_destroy(void *comm) {
  if (!comm) return MRAFT_OK;
  NCCL_TRY(ncclCommDestroy((ncclComm_t)comm));
  return MRAFT_OK;
}

int mraft_allgather_status(mraft_engine *h, void *comm, const int32_t *local, int32_t *gathered,
                           int32_t where, uint32_t flags) {
  TRY(enter_handle(h));
  if (!comm || !local || !gathered) return fail(MRAFT_E_INVAL, "null argument");
  // Without OVERLAP/ORDERED the gather runs on the engine stream, after the
  // shard launches (joined). With OVERLAP it waits for them on the fan-in
  // stream only, so the next tick's shards do not wait for this tick's others.
  if (where == MRAFT_HOST || !(flags & (MRAFT_FANIN_OVERLAP | MRAFT_FANIN_ORDERED))) TRY(join_shards(h));
  ncclComm_t c = (ncclComm_t)comm;
  int nranks = 0;
  NCCL_TRY(ncclCommCount(c, &nranks));
  const size_t words = 2 * (size_t)h->G;
  if (where == MRAFT_HOST) {
    Stage sg(h, where);
    const int32_t *l = sg.in(local, words);
    int32_t *g = sg.out(gathered, words * nranks);
    TRY(sg.status());
    NCCL_TRY(ncclAllGather(l, g, words, ncclInt32, c, h->stream));
    return sg.finish();
  }
  hipStream_t st = h->stream;
  if (flags & MRAFT_FANIN_ORDERED) {
    TRY(fanin_stream_of(h, &st));
  } else if (flags & MRAFT_FANIN_OVERLAP) {
    TRY(fanin_stream_of(h, &st));
    if (!h->fanin_ev) HIP_TRY(hipEventCreateWithFlags(&h->fanin_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->fanin_ev, h->stream));
    HIP_TRY(hipStreamWaitEvent(st, h->fanin_ev, 0));
    if (h->shards_pending)
      for (int k = 0; k < h->nshards; ++k) {
        HIP_TRY(hipEventRecord(h->shard_ev[k], h->shard_q[k]));
        HIP_TRY(hipStreamWaitEvent(st, h->shard_ev[k], 0));
      }
  }
  NCCL_TRY(ncclAllGather(local, gathered, words, ncclInt32, c, st));
  HIP_TRY(hipGetLastError());
  return MRAFT_OK;
}

int mraft_fanin_synchronize(mraft_engine *h) {
  TRY(enter_handle(h));
  hipStream_t st;
  TRY(fanin_stream_of(h, &st));
  HIP_TRY(hipStreamSynchronize(st));
  return MRAFT_OK;
}

void *mraft_fanin_stream(mraft_engine *h) {
  if (!h) return nullptr;
  hipStream_t st = nullptr;
  if (hipSetDevice(h->device) != hipSuccess || fanin_stream_of(h, &st) != MRAFT_OK) return nullptr;
  return (void *)st;
}

}  // extern "C"
