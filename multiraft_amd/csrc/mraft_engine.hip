// mraft_engine.hip — the handle of libmraft_hip.so (include/mraft.h): device
// state ownership (one HBM-resident SoA image per handle), the engine's
// streams and hardware queues, its stream-ordered memory and the error text.
// The calls that launch kernels are in mraft_abi_*.hip. No exception or C++
// type crosses the ABI.
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mraft_engine.h"

namespace mraft::host {

namespace {
thread_local std::string g_err;
}

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int join_shards(mraft_engine *h) {
  if (!h->shards_pending) return MRAFT_OK;
  for (int s = 0; s < h->nshards; ++s) {
    HIP_TRY(hipEventRecord(h->shard_ev[s], h->shard_q[s]));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->shard_ev[s], 0));
  }
  h->shards_pending = false;
  return MRAFT_OK;
}

int alloc_bytes(mraft_engine *h, void **p, size_t bytes, const char *what) {
  *p = nullptr;
  if (hipMallocAsync(p, bytes, h->stream) != hipSuccess || !*p) {
    (void)hipGetLastError();
    return fail(MRAFT_E_NOMEM, "%s: device allocation of %zu B failed", what, bytes);
  }
  return MRAFT_OK;
}

int scratch_bytes(mraft_engine *h, ScratchSlot slot, size_t bytes, void **out, bool *grew) {
  if (bytes == 0) bytes = 16;
  const bool grows = h->scratch_cap[slot] < bytes;
  if (grows) {
    if (h->scratch_ptr[slot]) HIP_TRY(hipFreeAsync(h->scratch_ptr[slot], h->stream));
    h->scratch_cap[slot] = 0;
    TRY(alloc_bytes(h, &h->scratch_ptr[slot], bytes, "scratch"));
    h->scratch_cap[slot] = bytes;
  }
  if (grew) *grew = grows;
  *out = h->scratch_ptr[slot];
  return MRAFT_OK;
}

int ensure_claim(mraft_engine *h) {
  const size_t gp = (size_t)gp_of(h);
  if (!h->claim) {
    TRY(alloc_async(h, &h->claim, gp, "claim", true));
    TRY(alloc_async(h, &h->srcmark, gp, "srcmark", true));
  }
  if (++h->epoch == 0) {  // wrapped: reset (and every epoch-tagged counter)
    HIP_TRY(hipMemsetAsync(h->claim, 0, gp * sizeof *h->claim, h->stream));
    HIP_TRY(hipMemsetAsync(h->srcmark, 0, gp * sizeof *h->srcmark, h->stream));
    if (h->scratch_ptr[kScrAeKin])
      HIP_TRY(hipMemsetAsync(h->scratch_ptr[kScrAeKin], 0, h->scratch_cap[kScrAeKin], h->stream));
    h->epoch = 1;
  }
  return MRAFT_OK;
}

int copy_array(mraft_engine *h, bool load, int32_t *eng, int32_t *usr, size_t bytes, int32_t where) {
  if (!usr) return MRAFT_OK;
  const hipMemcpyKind k = where != MRAFT_HOST ? hipMemcpyDeviceToDevice : load ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(hipMemcpyAsync(load ? eng : usr, load ? usr : eng, bytes, k, h->stream));
  return MRAFT_OK;
}

int finish_copies(mraft_engine *h, int32_t where) {
  if (where == MRAFT_HOST) HIP_TRY(hipStreamSynchronize(h->stream));
  return MRAFT_OK;
}

}  // namespace mraft::host

using namespace mraft::host;

namespace {

// Array table: pointer-to-member + element count.
struct ArrDesc { int32_t *mraft_soa::*ptr; int kind; };  // kind 0: G*P, 1: G*P*L, 2: G*P*P
const ArrDesc kArrays[] = {
    {&mraft_soa::current_term, 0}, {&mraft_soa::voted_for, 0},   {&mraft_soa::state, 0},
    {&mraft_soa::commit_index, 0}, {&mraft_soa::last_applied, 0}, {&mraft_soa::dummy_index, 0},
    {&mraft_soa::last_index, 0},   {&mraft_soa::granted_votes, 0}, {&mraft_soa::log_term, 1},
    {&mraft_soa::match_index, 2},  {&mraft_soa::next_index, 2},  {&mraft_soa::persist_dirty, 0},
    {&mraft_soa::log_head, 0},     {&mraft_soa::has_snapshot, 0}, {&mraft_soa::terms_sorted, 0}};

size_t arr_bytes(const mraft_engine *h, int kind) {
  int64_t gp = gp_of(h);
  int64_t n = kind == 0 ? gp : kind == 1 ? gp * h->L : gp * h->P;
  return (size_t)n * sizeof(int32_t);
}

// The one place that decides the engine stream, from the streams the handle
// has: the entry points change those and call this. It runs as soon as a
// stream is gone, before anything that can fail, so h->stream never names a
// destroyed stream.
void select_stream(mraft_engine *h) {
  h->stream = h->caller_stream ? h->caller_stream : h->tick_masked ? h->tick_masked : h->own_stream;
}

// Host wait for everything the engine has enqueued (engine, shard and fan-in
// streams). Errors are ignored (teardown paths).
void drain(mraft_engine *h) {
  (void)hipStreamSynchronize(h->stream);
  for (int s = 0; s < h->nshards; ++s)
    if (h->shard_q[s]) (void)hipStreamSynchronize(h->shard_q[s]);
  h->shards_pending = false;
}

// A stream on a hardware queue of its own (hipExtStreamCreateWithCUMask: a
// CU-masked stream gets a dedicated queue, a pooled stream may share one with
// another stream, and two launches on one queue run one after the other).
// tick_side: every CU but the fan-in's reserved ones; otherwise only those.
int make_queue(mraft_engine *h, bool tick_side, hipStream_t *out) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, h->device));
  const int ncu = prop.multiProcessorCount, nw = (ncu + 31) / 32;
  std::vector<uint32_t> mask(nw, 0);
  // the highest fan_cus CU bits go to the fan-in, the rest to the tick
  for (int cu = 0; cu < ncu; ++cu)
    if ((cu >= ncu - h->fan_cus) != tick_side) mask[cu / 32] |= 1u << (cu % 32);
  HIP_TRY(hipExtStreamCreateWithCUMask(out, (uint32_t)nw, mask.data()));
  return MRAFT_OK;
}

// Ends a CU-masked stream of the handle (*s, which may be null): waited for,
// taken out of the handle and of the engine stream's choice, then destroyed.
int destroy_masked(mraft_engine *h, hipStream_t *s) {
  const hipStream_t gone = *s;
  if (!gone) return MRAFT_OK;
  HIP_TRY(hipStreamSynchronize(gone));
  *s = nullptr;
  select_stream(h);
  HIP_TRY(hipStreamDestroy(gone));
  return MRAFT_OK;
}

void destroy_shard_queues(mraft_engine *h) {
  for (int s = 0; s < kMaxShards; ++s) {
    if (h->shard_q[s]) {
      (void)hipStreamSynchronize(h->shard_q[s]);
      (void)hipStreamDestroy(h->shard_q[s]);
      h->shard_q[s] = nullptr;
    }
    if (h->shard_ev[s]) (void)hipEventDestroy(h->shard_ev[s]);
    h->shard_ev[s] = nullptr;
  }
  h->shards_pending = false;
}

int create_shard_queues(mraft_engine *h, int n) {
  for (int s = 0; s < n; ++s) {
    TRY(make_queue(h, true, &h->shard_q[s]));
    HIP_TRY(hipEventCreateWithFlags(&h->shard_ev[s], hipEventDisableTiming));
  }
  if (!h->fork_ev) HIP_TRY(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
  return MRAFT_OK;
}

void free_owned(mraft_engine *h) {
  if (!h->owned) return;
  for (const auto &a : kArrays) {
    int32_t *p = h->dev.*(a.ptr);
    if (p) (void)hipFree(p);
    h->dev.*(a.ptr) = nullptr;
  }
  h->owned = false;
  h->bound = false;
}

// The stream, the pinned words and (without MRAFT_CREATE_NO_ALLOC) the state
// arrays of a new handle. On failure the handle is left partly built, for
// teardown().
int create_parts(mraft_engine *h, uint32_t flags) {
  if (flags & MRAFT_CREATE_DEDICATED_QUEUE)
    TRY(make_queue(h, true, &h->own_stream));
  else if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
    return fail(MRAFT_E_HIP, "hipStreamCreate failed");
  h->stream = h->own_stream;
  void *hp = nullptr, *dp = nullptr;
  if (hipHostMalloc(&hp, sizeof(long long) * kHintWords, hipHostMallocMapped) != hipSuccess)
    return fail(MRAFT_E_NOMEM, "pinned host word allocation failed");
  h->dhint = (volatile long long *)hp;
  h->dhint[kHintDeferred] = 0;
  h->dhint[kHintStageNeed] = 0;
  for (int s = 0; s < kMaxShards; ++s) h->dhint[kHintLite + s] = -1;  // no light tick yet
  if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) return fail(MRAFT_E_HIP, "hipHostGetDevicePointer failed");
  h->dhint_dev = (long long *)dp;
  if (flags & MRAFT_CREATE_NO_ALLOC) return MRAFT_OK;
  h->owned = true;
  for (const auto &a : kArrays)
    if (hipMalloc(&(h->dev.*(a.ptr)), arr_bytes(h, a.kind)) != hipSuccess)
      return fail(MRAFT_E_NOMEM, "device state allocation failed (G=%d P=%d L=%d)", h->G, h->P, h->L);
  h->bound = true;
  (void)hipMemsetAsync(h->dev.log_term, 0, arr_bytes(h, 1), h->stream);
  (void)hipMemsetAsync(h->dev.match_index, 0, arr_bytes(h, 2), h->stream);
  (void)hipMemsetAsync(h->dev.next_index, 0, arr_bytes(h, 2), h->stream);
  mraft::launch_init_state(dev_of(h), h->stream);
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(MRAFT_E_HIP, "init failed: %s", hipGetErrorString(e));
  return MRAFT_OK;
}

// Waits for the handle's work and releases everything it owns, then the
// handle. Every member is null until it is made, so a partly built handle
// (a failed mraft_create) takes the same path; one without a stream has
// enqueued nothing.
void teardown(mraft_engine *h) {
  (void)hipSetDevice(h->device);
  if (h->stream) drain(h);
  free_owned(h);
  if (h->stream) {
    // stream-ordered buffers (alloc_async): freed on the engine stream, then waited for
    for (void *p : h->scratch_ptr)
      if (p) (void)hipFreeAsync(p, h->stream);
    for (void *p : {(void *)h->claim, (void *)h->srcmark, (void *)h->ae_total, (void *)h->lite_list,
                    (void *)h->lite_cnt, (void *)h->tm_ed, (void *)h->tm_hd, (void *)h->reach})
      if (p) (void)hipFreeAsync(p, h->stream);
    (void)hipStreamSynchronize(h->stream);
  }
  if (h->fanin_own) (void)hipStreamSynchronize(h->fanin_own);
  if (h->fanin_masked) (void)hipStreamSynchronize(h->fanin_masked);
  destroy_shard_queues(h);
  for (hipStream_t s : {h->own_stream, h->fanin_own, h->fanin_masked, h->tick_masked})
    if (s) (void)hipStreamDestroy(s);
  if (h->fanin_ev) (void)hipEventDestroy(h->fanin_ev);
  if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
  if (h->dhint) (void)hipHostFree((void *)h->dhint);
  delete h;
}

}  // namespace

extern "C" {

const char *mraft_last_error_string(void) { return g_err.c_str(); }
int mraft_abi_version(void) { return MRAFT_ABI_VERSION; }

int mraft_create(int32_t groups, int32_t peers, int32_t log_capacity, int32_t device,
                 uint32_t flags, mraft_engine **out) {
  if (!out) return fail(MRAFT_E_INVAL, "out is null");
  *out = nullptr;
  if (groups < 1 || peers < 1 || peers > 8 || log_capacity < 1 || log_capacity > MRAFT_MAX_LOG_CAPACITY)
    return fail(MRAFT_E_INVAL, "bad dims G=%d P=%d L=%d (need G>=1, 1<=P<=8, 1<=L<=%d)", groups, peers,
                log_capacity, MRAFT_MAX_LOG_CAPACITY);
  if ((int64_t)groups * peers > INT32_MAX)
    return fail(MRAFT_E_INVAL, "G*P must fit in int32");
  HIP_TRY(hipSetDevice(device));
  mraft_engine *h = new mraft_engine();
  h->G = groups; h->P = peers; h->L = log_capacity; h->device = device;
  if (const char *e = getenv("MRAFT_DEFER_GRID_MIN")) {
    const long long v = atoll(e);
    if (v >= 1 && v <= kDeferGridMax) h->defer_grid_min = v;
  }
  const int rc = create_parts(h, flags);
  if (rc) {
    teardown(h);
    return rc;
  }
  *out = h;
  return MRAFT_OK;
}

int mraft_destroy(mraft_engine *h) {
  if (h) teardown(h);
  return MRAFT_OK;
}

int mraft_set_stream(mraft_engine *h, void *stream) {
  TRY(enter_handle(h));
  // outstanding shard ticks, then everything on the old stream (the engine's
  // stream-ordered buffers may still be in use there), are ordered before the
  // new stream's work: device-side waits, no host wait
  TRY(join_shards(h));
  const hipStream_t old = h->stream, old_caller = h->caller_stream;
  // the masked tick stream handed back as the caller's stays the engine's:
  // caller_stream never names a stream the engine may destroy
  h->caller_stream = (hipStream_t)stream == h->tick_masked ? nullptr : (hipStream_t)stream;
  select_stream(h);
  if (h->stream != old) {
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) {
      e = hipEventRecord(ev, old);
      if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, ev, 0);
      (void)hipEventDestroy(ev);  // released once the wait is satisfied
    }
    if (e != hipSuccess) {  // not ordered: the engine stays on the old stream
      h->caller_stream = old_caller;
      select_stream(h);
      return fail(MRAFT_E_HIP, "ordering the new stream: %s", hipGetErrorString(e));
    }
  }
  return MRAFT_OK;
}

// With tick shards, the engine stream is first ordered after the outstanding
// shard launches (a device-side wait), so work the caller puts on the returned
// stream sees the tick's outputs. NULL when that ordering fails
// (mraft_last_error_string says why): the stream would not see the outputs.
void *mraft_get_stream(mraft_engine *h) {
  if (have_handle(h)) return nullptr;
  if (h->shards_pending) {
    if (hipSetDevice(h->device) != hipSuccess) {
      fail(MRAFT_E_HIP, "hipSetDevice failed");
      return nullptr;
    }
    if (join_shards(h) != MRAFT_OK) return nullptr;
  }
  return (void *)h->stream;
}

int mraft_synchronize(mraft_engine *h) {
  TRY(enter_handle(h));
  TRY(join_shards(h));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return MRAFT_OK;
}

int mraft_dims(const mraft_engine *h, int32_t *g, int32_t *p, int32_t *l) {
  TRY(enter_handle(h));
  if (g) *g = h->G;
  if (p) *p = h->P;
  if (l) *l = h->L;
  return MRAFT_OK;
}

int mraft_load_state(mraft_engine *h, const mraft_soa *src, int32_t where) {
  TRY(enter(h));
  if (!src) return fail(MRAFT_E_INVAL, "src is null");
  for (const auto &a : kArrays)
    if (!(src->*(a.ptr))) return fail(MRAFT_E_INVAL, "load_state: every array is required");
  for (const auto &a : kArrays) TRY(copy_array(h, true, h->dev.*(a.ptr), src->*(a.ptr), arr_bytes(h, a.kind), where));
  mraft::launch_terms_sorted(dev_of(h), h->stream);  // the engine's own proof, not the source's claim
  HIP_TRY(hipGetLastError());
  return finish_copies(h, where);
}

int mraft_store_state(mraft_engine *h, const mraft_soa *dst, int32_t where) {
  TRY(enter(h));
  if (!dst) return fail(MRAFT_E_INVAL, "dst is null");
  for (const auto &a : kArrays) TRY(copy_array(h, false, h->dev.*(a.ptr), dst->*(a.ptr), arr_bytes(h, a.kind), where));
  return finish_copies(h, where);
}

int mraft_state_view(mraft_engine *h, mraft_soa *out) {
  TRY(enter(h));
  if (!out) return fail(MRAFT_E_INVAL, "out is null");
  *out = h->dev;
  return MRAFT_OK;
}

int mraft_bind_state(mraft_engine *h, const mraft_soa *d) {
  TRY(enter_handle(h));
  if (!d) return fail(MRAFT_E_INVAL, "state is null");
  for (const auto &a : kArrays)
    if (!(d->*(a.ptr))) return fail(MRAFT_E_INVAL, "bind_state: every array is required");
  if (h->owned) {
    drain(h);
    free_owned(h);
  }
  h->dev = *d;
  h->bound = true;
  return MRAFT_OK;
}

// ---------------------------------------------------------------- reachability

int mraft_set_reachable(mraft_engine *h, const uint8_t *reach, int32_t where) {
  TRY(enter(h));
  uint8_t *fresh = nullptr;
  if (reach) {
    // A new buffer per call: the handle sees it only after the allocation and
    // the copy were enqueued without error; the launches already enqueued keep
    // the old one, which is freed in stream order behind them.
    TRY(alloc_async(h, &fresh, (size_t)h->G, "reachability mask"));
    const hipError_t e = hipMemcpyAsync(fresh, reach, (size_t)h->G,
                                        where == MRAFT_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream);
    const hipError_t e2 = e == hipSuccess && where == MRAFT_HOST ? hipStreamSynchronize(h->stream) : e;
    if (e2 != hipSuccess) {
      (void)hipFreeAsync(fresh, h->stream);
      return fail(MRAFT_E_HIP, "copying the reachability mask failed: %s", hipGetErrorString(e2));
    }
  }
  if (h->reach) (void)hipFreeAsync(h->reach, h->stream);
  h->reach = fresh;
  return MRAFT_OK;
}

int mraft_get_reachable(mraft_engine *h, uint8_t *out, int32_t where) {
  TRY(enter(h));
  if (!h->reach) return 0;
  if (!out) return fail(MRAFT_E_INVAL, "out is null");
  HIP_TRY(hipMemcpyAsync(out, h->reach, (size_t)h->G,
                         where == MRAFT_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, h->stream));
  TRY(finish_copies(h, where));
  return 1;
}

// ---------------------------------------------------------------- queues

int mraft_fanin_reserve_cus(mraft_engine *h, int32_t n_cus) {
  TRY(enter_handle(h));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, h->device));
  const int ncu = prop.multiProcessorCount;
  if (n_cus < 0 || n_cus >= ncu) return fail(MRAFT_E_INVAL, "n_cus %d of %d CUs", n_cus, ncu);
  drain(h);
  // one shard: the tick runs on the engine stream, which takes the tick side's
  // mask in place of a caller's stream. Tick shards: their queues take it; the
  // engine stream carries no tick and stays as it is
  const int S = h->nshards;
  if (S <= 1) h->caller_stream = nullptr;
  select_stream(h);
  TRY(destroy_masked(h, &h->fanin_masked));
  TRY(destroy_masked(h, &h->tick_masked));
  h->fan_cus = n_cus;
  if (S > 1) {
    destroy_shard_queues(h);
    TRY(create_shard_queues(h, S));
  }
  if (n_cus == 0) return MRAFT_OK;
  if (S <= 1) {
    TRY(make_queue(h, true, &h->tick_masked));
    select_stream(h);
  }
  TRY(make_queue(h, false, &h->fanin_masked));
  return MRAFT_OK;
}

int mraft_set_tick_shards(mraft_engine *h, int32_t shards) {
  TRY(enter_handle(h));
  if (shards < 1 || shards > kMaxShards || shards > h->G)
    return fail(MRAFT_E_INVAL, "shards %d (need 1..%d and at most G = %d)", shards, kMaxShards, h->G);
  drain(h);
  destroy_shard_queues(h);
  h->nshards = 1;
  if (shards > 1) {
    TRY(create_shard_queues(h, shards));
    h->nshards = shards;
    // the masked tick stream of a one-shard engine (mraft_fanin_reserve_cus)
    // is not needed: the shard queues carry the mask
    TRY(destroy_masked(h, &h->tick_masked));
  } else if (h->fan_cus > 0 && !h->tick_masked) {
    TRY(make_queue(h, true, &h->tick_masked));
    select_stream(h);
  }
  return MRAFT_OK;
}

int32_t mraft_get_tick_shards(const mraft_engine *h) { return h ? h->nshards : 0; }

void *mraft_shard_stream(mraft_engine *h, int32_t shard) {
  if (!h || shard < 0 || shard >= h->nshards) return nullptr;
  return h->nshards > 1 ? (void *)h->shard_q[shard] : (void *)h->stream;
}

}  // extern "C"
