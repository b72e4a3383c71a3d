// mraft_engine.h — the handle behind include/mraft.h and what the host units
// (mraft_engine.hip and mraft_abi_*.hip) share: the entry prologues, the typed
// scratch and staging helpers, the claims and the reply folds' common part.
// Private: never installed. Everything in mraft::host has hidden visibility, so
// the library exports the C entry points only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mraft.h"
#include "mraft_device.h"
#include "mraft_internal.h"

constexpr int kMaxShards = 8;
// Default capacity of the AppendEntries stage (mraft_set_stage_capacity): 16 MiB.
constexpr int64_t kDefaultStageWords = (int64_t)1 << 22;
// The deferred launch's grid (mraft_handle_append_entries by reference): the
// last call's deferred count, read from a pinned word the device writes, in
// [kDeferGridMin, kDeferGridMax] workgroups (grid-stride beyond). With no
// deferred item the launch exits at once on kDeferGridMin workgroups; a
// deferred-heavy batch gets a workgroup per item from the next call on. The
// minimum bounds the first deferred-heavy call after calls without any (a
// partition healing): 512 workgroups take it 30.6 -> 1.07 ms (stale second
// leaders) and 96.9 -> 3.7 ms (2-cycles) against 8, with the message path's
// pipelines within noise (profiles/r6_g1; round 5 had chosen 8 for ~2 %
// there, r5_g1).
#ifndef MRAFT_DEFER_GRID_MIN
#define MRAFT_DEFER_GRID_MIN 512
#endif
constexpr int kDeferGridMin = MRAFT_DEFER_GRID_MIN;
constexpr int kDeferGridMax = 1 << 16;
// The light tick's fallback launch (MRAFT_TICK_LIGHT): at least this many
// workgroups, twice the previous light tick's count, at most the groups (a
// grid-stride loop makes any grid exact; an empty one costs a few µs).
constexpr long long kLiteGridMin = 2048;
constexpr long long kLiteGridUnknown = 8192;
constexpr int kAutoProbe = 32;  // MRAFT_TICK_AUTO: a light tick at least every 32 ticks
// The engine's pinned host words (device-written, read by the host through
// hint() when it enqueues).
enum Hint {
  kHintDeferred,   // the last by-reference AppendEntries call's deferred count
  kHintStageNeed,  // the staged words of the last call that exceeded the stage (its need)
  kHintLite,       // + s: the last light tick's fallback count of shard s
  kHintWords = kHintLite + kMaxShards
};
// The engine's grow-only device scratch buffers (scratch()), one slot per
// purpose. A slot that several calls name (the folds' segment errors, the
// persistence calls' headers and terms) is safe to share because calls on one
// handle do not overlap, every call's work is ordered on the engine stream,
// and each call writes a buffer before it reads it: nothing in these buffers
// outlives the call that filled it. The one exception is kScrAeKin, whose
// words carry the claim epoch of the call that wrote them and must survive
// from call to call (ensure_claim zeroes it when the epoch wraps); no other
// use may ever be given that slot. Stage (host-mode batches) maps a call's
// k-th buffer to kScrStage0 + k, a range no other use reaches.
constexpr int kStageMax = 7;  // buffers one call stages at most (mraft_start_and_tick)
enum ScratchSlot {
  kScrTickCount,     // mraft_replicate_tick_count: the counter stripes
  kScrSegErr,        // the three reply folds: per-segment claim errors
  kScrFoldScan,      // mraft_process_append_replies: launch_fold's scan lists
  kScrPersistSlots,  // mraft_read_persistent: the slots
  kScrPersistHdr,    // mraft_read_persistent, mraft_restore: the headers
  kScrPersistTerms,  // mraft_read_persistent, mraft_restore: the terms
  kScrRestoreErr,    // mraft_restore: the host's per-item verdicts
  kScrApplyBlocks,   // mraft_collect_apply_compact: per-block counts
  // AppendEntries by reference
  kScrAeSoff,     // per item: its stage offset
  kScrAeSetHead,  // per item: the set-head byte
  kScrAeStage,    // the stage (mraft_set_stage_capacity)
  kScrAeDefer,    // per stripe: the deferred items
  kScrAeOrder,    // the ordered fallback's records and cycle buffers
  kScrAeKin,      // the fallback's reader counts: epoch-tagged, persists across calls
  // mraft_clock_step: the words one launch hands to the next when the caller
  // gave no buffer for them, and the sender's terms
  kScrClockLp,
  kScrClockGf,
  kScrClockCommit,
  kScrClockTl,
  kScrClockTg,
  kScrTickerCnt,  // mraft_ticker: per-block counts of both lists
  kScrStage0,     // Stage: kScrStage0 ... kScrStage0 + kStageMax - 1
  kScrSlots = kScrStage0 + kStageMax
};
// MRAFT_STAGE_AUTO grows the stage to 5/4 of a batch's need, in 1 Mi-word
// steps, up to 2^31 - 1 words (8 GiB).
constexpr int64_t kStageStep = (int64_t)1 << 20;
// Words of the fallback's per-workgroup cycle buffers (nslot x L, at most this).
// A host constant (the kernels take nslot as an argument); the small-grid test
// library sets it to 128, so at L = 64 two workgroups have a buffer and the
// rest of the deferred grid only counts out.
#ifndef MRAFT_CYC_SLOT_WORDS
#define MRAFT_CYC_SLOT_WORDS ((int64_t)1 << 25)  // 8,192 buffers at L = 4,096 (128 MiB)
#endif
constexpr int64_t kCycSlotWords = MRAFT_CYC_SLOT_WORDS;

struct mraft_engine {
  int32_t G = 0, P = 0, L = 0, device = 0;
  bool owned = false, bound = false;
  mraft_soa dev{};
  // The engine stream: the caller's (mraft_set_stream) if there is one, else
  // the CU-masked tick stream (mraft_fanin_reserve_cus on one shard) if there
  // is one, else the engine's own. select_stream (mraft_engine.hip) derives it;
  // nothing else assigns it after mraft_create.
  hipStream_t own_stream = nullptr, caller_stream = nullptr, stream = nullptr;
  // fan-in (mraft_allgather_status): its own stream, ordered after the engine
  // stream by an event; optional CU-masked pair (mraft_fanin_reserve_cus)
  hipStream_t fanin_own = nullptr, fanin_masked = nullptr, tick_masked = nullptr;
  hipEvent_t fanin_ev = nullptr;
  int32_t fan_cus = 0;  // CUs reserved for the fan-in (the tick side's masks leave them out)
  // Tick group shards (mraft_set_tick_shards): S dedicated hardware queues the
  // engine owns; a tick forks onto them from the engine stream (fork_ev) and
  // the next call of any other kind joins them back (shard_ev), so one shard's
  // tick i+1 follows only its own tick i.
  int32_t nshards = 1;
  hipStream_t shard_q[kMaxShards] = {};
  hipEvent_t shard_ev[kMaxShards] = {};
  hipEvent_t fork_ev = nullptr;
  bool shards_pending = false;
  unsigned long long *claim = nullptr;
  uint32_t *srcmark = nullptr;             // per slot: epoch of the last call that read its row
  uint32_t epoch = 0;
  unsigned long long *ae_total = nullptr;  // AppendEntries by reference: the handler's counters (mraft_internal.h kAeCnt*)
  int64_t stage_cap = kDefaultStageWords;  // words of staged entries the deferred launch may use
  bool stage_auto = true;                  // MRAFT_STAGE_AUTO: grow stage_cap to the last overflow's need
  volatile long long *dhint = nullptr;  // the pinned host words (Hint): device-written
  long long *dhint_dev = nullptr;       // their device-side address
  // the deferred launch's minimum grid: kDeferGridMin, or the environment's
  // MRAFT_DEFER_GRID_MIN at mraft_create (tests run the small-grid paths with it)
  long long defer_grid_min = kDeferGridMin;
  // MRAFT_TICK_LIGHT (mraft_set_tick_mode): the lists of groups for the full
  // tick (shard s at lite_list_begin), a pair of counter sets per shard (the light
  // launch counts into one, the fallback zeroes the other for the next tick)
  // and per shard the last fallback count, pinned (dhint + kHintLite + s)
  int32_t tick_mode = MRAFT_TICK_AUTO;
  int32_t *lite_list = nullptr;
  unsigned *lite_cnt = nullptr;
  int lite_par[kMaxShards] = {};
  int auto_since[kMaxShards] = {};  // MRAFT_TICK_AUTO: full ticks since the last light one
  // Timers (mraft_timers_enable): both deadline arrays or neither, with the
  // configuration they were armed under
  int32_t *tm_ed = nullptr, *tm_hd = nullptr;
  mraft_timer_config tcfg{};
  // Reachability (mraft_set_reachable): the engine's copy of the mask, one
  // byte per group, or null when none is set (everyone connected). While it is
  // set the co-resident calls launch their kernels' masked instances with it.
  uint8_t *reach = nullptr;
  void *scratch_ptr[kScrSlots] = {};
  size_t scratch_cap[kScrSlots] = {};
};

namespace mraft {
namespace host __attribute__((visibility("hidden"))) {

// Records the calling thread's error text (mraft_last_error_string); returns code.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(MRAFT_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));          \
  } while (0)

#define TRY(expr)          \
  do {                     \
    int rc_ = (expr);      \
    if (rc_) return rc_;   \
  } while (0)

// ---------------------------------------------------------------- mraft_engine.hip
// Orders the engine stream after every shard launch still outstanding (no
// host wait): the shard queues record their join events and the engine
// stream waits on them.
int join_shards(mraft_engine *h);
// Device memory in stream order on the engine stream (hipMallocAsync /
// hipFreeAsync): allocating or growing a buffer never waits for the device, so
// MRAFT_DEVICE calls stay asynchronous when a batch is larger than any before
// (include/mraft.h). A freed buffer is released after the
// work already enqueued on the stream, which may still read it.
int alloc_bytes(mraft_engine *h, void **p, size_t bytes, const char *what);
// Grow-only device scratch slot of at least `bytes` (stream-ordered: no host
// wait); *grew (optional) tells whether the buffer is a new one.
int scratch_bytes(mraft_engine *h, ScratchSlot slot, size_t bytes, void **out, bool *grew = nullptr);
// The claim words (and the by-reference handler's source marks), allocated on
// first use, and the next claim epoch. Only for calls with n > 0: an empty
// call does not advance the epoch.
int ensure_claim(mraft_engine *h);
// One array of a load (into the engine's `eng`) or a store (out of it): the
// caller's array `usr` is host or device memory (`where`), and a null one is
// skipped. finish_copies() ends the call: a host-mode one waits for its copies.
int copy_array(mraft_engine *h, bool load, int32_t *eng, int32_t *usr, size_t bytes, int32_t where);
int finish_copies(mraft_engine *h, int32_t where);

// ---------------------------------------------------------------- mraft_abi_tick.hip
// The tick launch(es): one launch on the engine stream, or with S tick shards
// one launch per contiguous group range on its own queue, each queue first
// waiting for the engine stream's prior work (one event, fork_ev).
int launch_tick(mraft_engine *h, const int32_t *lp, int32_t *gf, int32_t *ec, int32_t *et,
                const StartIO *sio = nullptr);

// ---------------------------------------------------------------- prologues
// The entry points that return no code (getters): MRAFT_E_INVAL, with the
// message, for a null handle.
inline int have_handle(const mraft_engine *h) { return h ? MRAFT_OK : fail(MRAFT_E_INVAL, "null engine handle"); }

// A handle, on its device: the calls that need no bound state and join no shards.
inline int enter_handle(const mraft_engine *h) {
  TRY(have_handle(h));
  HIP_TRY(hipSetDevice(h->device));
  return MRAFT_OK;
}

// The ticks' prologue: the handle is usable, on its device. The ticks do not
// join earlier shard launches (launch_tick forks from the engine stream
// instead): with tick shards, shard s's tick follows its own previous tick
// only. A host-buffer tick joins them before its copies back.
inline int enter_tick(mraft_engine *h) {
  TRY(enter_handle(h));
  if (!h->bound) return fail(MRAFT_E_NOSTATE, "engine has no device state bound");
  return MRAFT_OK;
}

// Every other entry point's: also, earlier sharded ticks are ordered before
// this call's work on the engine stream.
inline int enter(mraft_engine *h) {
  TRY(enter_tick(h));
  return join_shards(h);
}

inline long long hint(const mraft_engine *h, int k) { return h->dhint[k]; }

inline int64_t gp_of(const mraft_engine *h) { return (int64_t)h->G * h->P; }

inline Dev dev_of(const mraft_engine *h) {
  Dev d;
  d.term = h->dev.current_term; d.voted = h->dev.voted_for; d.role = h->dev.state;
  d.commit = h->dev.commit_index; d.applied = h->dev.last_applied; d.dummy = h->dev.dummy_index;
  d.last = h->dev.last_index; d.votes = h->dev.granted_votes; d.log = h->dev.log_term;
  d.match = h->dev.match_index; d.next = h->dev.next_index; d.pdirty = h->dev.persist_dirty;
  d.head = h->dev.log_head; d.hsnap = h->dev.has_snapshot; d.srt = h->dev.terms_sorted;
  d.G = h->G; d.P = h->P; d.L = h->L;
  return d;
}

// Groups [g0, g1) of the engine's state as a state of their own (the SoA
// arrays are group-major: no copies).
inline Dev dev_slice(const mraft_engine *h, int32_t g0, int32_t g1) {
  Dev d = dev_of(h);
  const int64_t s0 = (int64_t)g0 * h->P;
  for (int32_t **p : {&d.term, &d.voted, &d.role, &d.commit, &d.applied, &d.dummy, &d.last, &d.votes, &d.pdirty,
                      &d.head, &d.hsnap, &d.srt})
    if (*p) *p += s0;
  d.log += s0 * h->L;
  d.match += s0 * h->P;
  d.next += s0 * h->P;
  d.G = g1 - g0;
  return d;
}

// ---------------------------------------------------------------- typed memory
// alloc_bytes for n elements of T, zeroed or not (stream-ordered).
template <class T>
int alloc_async(mraft_engine *h, T **p, size_t n, const char *what, bool zero = false) {
  void *v = nullptr;
  const int rc = alloc_bytes(h, &v, sizeof(T) * n, what);
  *p = (T *)v;
  if (rc == MRAFT_OK && zero) HIP_TRY(hipMemsetAsync(v, 0, sizeof(T) * n, h->stream));
  return rc;
}

// scratch_bytes for n elements of T.
template <class T>
int scratch(mraft_engine *h, ScratchSlot slot, size_t n, T **out) {
  void *p = nullptr;
  const int rc = scratch_bytes(h, slot, sizeof(T) * n, &p);
  *out = (T *)p;
  return rc;
}

// scratch() whose new buffer is zeroed when it is (re)allocated (stream-ordered):
// for epoch-tagged counters, whose stale contents must never carry a tag a
// later call could take for its own.
template <class T>
int scratch_zeroed(mraft_engine *h, ScratchSlot slot, size_t n, T **out) {
  void *p = nullptr;
  bool grew = false;
  TRY(scratch_bytes(h, slot, sizeof(T) * n, &p, &grew));
  if (grew) HIP_TRY(hipMemsetAsync(p, 0, h->scratch_cap[slot], h->stream));
  *out = (T *)p;
  return MRAFT_OK;
}

// Batch pointer staging: for MRAFT_HOST, input buffers are copied to device
// scratch (the call's k-th buffer to slot kScrStage0 + k) and output buffers
// are copied back by finish(); for MRAFT_DEVICE the caller's pointer is used
// as it is. A null pointer maps to null. The first failure sticks: the maps
// after it do nothing, and status() reports it before anything is launched.
struct Stage {
  mraft_engine *h;
  bool host;
  int rc = MRAFT_OK, n_map = 0, n_out = 0;
  struct Out { void *host; void *dev; size_t bytes; } outs[kStageMax];
  Stage(mraft_engine *hh, int32_t where) : h(hh), host(where == MRAFT_HOST) {}

  // in: n elements read by the kernel; out: n elements written by it.
  template <class T>
  const T *in(const T *p, size_t n) { return (const T *)map(p, sizeof(T) * n, true); }
  template <class T>
  T *out(T *p, size_t n) { return (T *)map(p, sizeof(T) * n, false); }
  int status() const { return rc; }
  int finish() {
    HIP_TRY(hipGetLastError());
    if (!host) return MRAFT_OK;
    for (int k = 0; k < n_out; ++k)
      if (outs[k].bytes)
        HIP_TRY(hipMemcpyAsync(outs[k].host, outs[k].dev, outs[k].bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return MRAFT_OK;
  }

 private:
  void *map(const void *p, size_t bytes, bool in) {
    if (!p || rc) return nullptr;
    if (!host) return const_cast<void *>(p);
    void *d = nullptr;
    rc = n_map == kStageMax ? fail(MRAFT_E_INVAL, "internal: a call stages more than %d buffers", kStageMax)
                            : scratch_bytes(h, (ScratchSlot)(kScrStage0 + n_map++), bytes, &d);
    if (rc == MRAFT_OK && in && bytes) rc = copy(d, p, bytes);
    if (rc) return nullptr;
    if (!in) outs[n_out++] = {const_cast<void *>(p), d, bytes};
    return d;
  }
  int copy(void *d, const void *p, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, h->stream));
    return MRAFT_OK;
  }
};

// ---------------------------------------------------------------- claims and folds
// The duplicate-slot claims of a batch of records (their slot member) or of
// bare slots, per item or per segment: stride and offset follow from the type.
template <class Rec>
constexpr int slot_offset() { return offsetof(Rec, slot); }
template <>
constexpr int slot_offset<int32_t>() { return 0; }
template <class Rec>
void claim(mraft_engine *h, const Rec *items, int64_t n, const int64_t *seg_begin, int32_t *err) {
  launch_claim(items, n, sizeof(Rec), slot_offset<Rec>(), seg_begin, gp_of(h), h->claim, h->epoch, err, h->stream);
}

// What the three reply folds share (mraft_process_*_replies): the argument
// checks, the next claim epoch, the staged buffers and the per-segment claim
// errors; launch(b) then enqueues the fold's own work.
template <class Rec>
struct FoldBufs {
  const Rec *it;
  const int64_t *sb;
  int64_t ns;
  int32_t *se, *fl, *e;
};
template <class Rec, class Launch>
int fold_replies(mraft_engine *h, const Rec *items, int64_t n, const int64_t *seg_begin, int64_t n_seg,
                 int32_t *out_flags, int32_t *item_err, int32_t where, Launch launch) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!items || !out_flags || !item_err)))
    return fail(MRAFT_E_INVAL, "null argument");
  if (seg_begin && n_seg < 0) return fail(MRAFT_E_INVAL, "n_seg < 0");
  if (n == 0) return MRAFT_OK;
  TRY(ensure_claim(h));
  Stage sg(h, where);
  FoldBufs<Rec> b{};
  b.it = sg.in(items, n);
  b.sb = sg.in(seg_begin, seg_begin ? n_seg + 1 : 0);
  b.ns = seg_begin ? n_seg : n;
  b.fl = sg.out(out_flags, n);
  b.e = sg.out(item_err, n);
  TRY(sg.status());
  TRY(scratch(h, kScrSegErr, (size_t)b.ns, &b.se));
  TRY(launch(b));
  return sg.finish();
}

// The InstallSnapshot and RequestVote folds: the outputs zeroed, the segment
// claims, then `fold` (launch_process_is, launch_tally).
template <class Rec>
int fold_records(mraft_engine *h, const Rec *items, int64_t n, const int64_t *seg_begin, int64_t n_seg,
                 int32_t *out_flags, int32_t *item_err, int32_t where,
                 void (*fold)(const Dev &, const Rec *, const int64_t *, int64_t, int32_t *, int32_t *, int32_t *,
                              hipStream_t)) {
  return fold_replies(h, items, n, seg_begin, n_seg, out_flags, item_err, where, [=](const FoldBufs<Rec> &b) -> int {
    HIP_TRY(hipMemsetAsync(b.fl, 0, sizeof(int32_t) * n, h->stream));
    HIP_TRY(hipMemsetAsync(b.e, 0, sizeof(int32_t) * n, h->stream));
    claim(h, b.it, b.ns, b.sb, b.se);
    fold(dev_of(h), b.it, b.sb, b.ns, b.se, b.fl, b.e, h->stream);
    return MRAFT_OK;
  });
}

}  // namespace host
}  // namespace mraft
