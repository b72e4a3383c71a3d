// mraft_internal.h — the host side of the launches: the launchers each kernel
// translation unit defines for the C-ABI implementation (mraft_abi_*.hip), under
// the name of the file that defines them, the helpers those launchers share,
// and the layout of each buffer a kernel indexes and the host sizes or carves
// (the handler's HsArgs, counters and order buffer; the light tick's lists and
// counters), stated here once for both sides.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/mraft.h"
#include "mraft_device.h"

namespace mraft {

// ---------------------------------------------------------------- launch helpers
// Workgroups of per_block threads for n items, a thread each (at least one).
inline int blocks_for(int64_t n, int per_block = 256) {
  int64_t b = (n + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : b);
}
// The kernels templated on the group size P: f(std::integral_constant<int, P>{})
// for a runtime P in [Lo, 8]; false, with f not called, outside it.
template <int Lo, class F>
bool with_peers(int P, F &&f) {
  if constexpr (Lo <= 8) {
    if (P != Lo) return with_peers<Lo + 1>(P, f);
    f(std::integral_constant<int, Lo>{});
    return true;
  } else {
    return false;
  }
}

#ifndef MRAFT_MSG_BLOCK
#define MRAFT_MSG_BLOCK 64  // workgroup size of the message path's lane-per-item kernels (gather, claims; r4_v26: 64 pipelines -3 %)
#endif
// (a smaller workgroup finds a CU with room sooner while another queue's
// handler or tick holds most wave slots: shard pipelines)
constexpr int kMsgBlock = MRAFT_MSG_BLOCK;

// ---------------------------------------------------------------- mraft_kernels.hip
void launch_init_state(const Dev &s, hipStream_t st);
void launch_terms_sorted(const Dev &s, hipStream_t st);  // terms_sorted recomputed from the logs

// Duplicate-slot claims: item i (slot read at byte offset slot_off of a record
// of `stride` bytes; or, with seg_begin, the slot of segment i's first item)
// wins iff it is the lowest index addressing its slot in this call.
void launch_claim(const void *items, int64_t n, int stride, int slot_off, const int64_t *seg_begin,
                  int64_t gp, unsigned long long *claim, uint32_t epoch, int32_t *err, hipStream_t st);

void launch_gather_args(const Dev &s, const int32_t *slots, const int32_t *peers, int64_t n,
                        mraft_ae_args *out, int32_t *err, hipStream_t st);
// Start: the slot claims (k_claim) and k_start, which checks them itself.
void launch_start(const Dev &s, const int32_t *slots, const int32_t *counts, int64_t n, int32_t *oi,
                  int32_t *ot, int32_t *ol, int32_t *err, unsigned long long *claim, uint32_t epoch,
                  hipStream_t st);
// mraft_start_and_tick: per group, counts[g] entries to Start at replica
// leader_peer[g] (0: none), and Start's outputs per group.
struct StartIO {
  const int32_t *counts;
  int32_t *oi, *ot, *ol, *err;
};
// Start at every group's leader replica (k_start per group; mraft_start_and_tick
// on the full tick's path).
void launch_start_groups(const Dev &s, const int32_t *lpeer, const StartIO &sio, hipStream_t st);
void launch_collect_apply(const Dev &s, int32_t *from, int32_t *to, int32_t *snap_index, int32_t *snap_term,
                          hipStream_t st);
// Ordered compaction (mraft_device.h): the workgroups of its count and emit
// launches over n items, and the scan between them — workgroup k < lists <= 2
// scans list k's nb block counts in place (exclusive) and writes total<k>.
inline int64_t compact_blocks(int64_t n) { return (n + kCompactBlock - 1) / kCompactBlock; }
void launch_compact_scan(int32_t *bcnt, int64_t nb, int lists, int64_t *total0, int64_t *total1, hipStream_t st);
void launch_collect_apply_compact(const Dev &s, int32_t *scratch_bcnt, int64_t cap, int32_t *oslot,
                                  int32_t *osnap_index, int32_t *osnap_term, int32_t *ofrom, int32_t *oto,
                                  int64_t *total, hipStream_t st);
void launch_snapshot(const Dev &s, const int32_t *slots, const int32_t *index, int64_t n,
                     int32_t *err, hipStream_t st);
void launch_gather_is(const Dev &s, const int32_t *slots, const int32_t *peers, int64_t n,
                      mraft_is_args *out, int32_t *err, hipStream_t st);
void launch_handle_is(const Dev &s, const mraft_is_args *args, int64_t n, mraft_is_reply *rep,
                      int32_t *flags, int32_t *err, hipStream_t st);
void launch_process_is(const Dev &s, const mraft_is_result *items, const int64_t *seg_begin, int64_t n_seg,
                       int32_t *seg_err, int32_t *flags, int32_t *item_err, hipStream_t st);
void launch_start_election(const Dev &s, const int32_t *slots, int64_t n, mraft_rv_args *out,
                           int32_t *err, hipStream_t st);
void launch_handle_rv(const Dev &s, const mraft_rv_args *args, int64_t n, mraft_rv_reply *rep,
                      int32_t *err, hipStream_t st);
void launch_tally(const Dev &s, const mraft_rv_result *items, const int64_t *seg_begin, int64_t n_seg,
                  int32_t *seg_err, int32_t *flags, int32_t *item_err, hipStream_t st);
void launch_collect_persist(const Dev &s, int32_t *out, hipStream_t st);
void launch_read_persistent_hdr(const Dev &s, const int32_t *slots, int64_t n,
                                mraft_persistent *out, hipStream_t st);
void launch_read_persistent_terms(const Dev &s, const mraft_persistent *hdr, int64_t n,
                                  int32_t *out, hipStream_t st);
void launch_restore(const Dev &s, const mraft_persistent *in, int64_t n, const int32_t *terms,
                    const int32_t *err, hipStream_t st);
// mraft_crash: ed / hd are the timer arrays, both or neither (null: no timers).
void launch_crash(const Dev &s, const int32_t *slots, int64_t n, int32_t *err, int32_t *ed, int32_t *hd,
                  hipStream_t st);
void launch_export(const Dev &s, const int32_t *lpeer, int32_t *commit, int32_t *term_leader,
                   hipStream_t st);

// ---------------------------------------------------------------- mraft_handle_ae.hip
// AppendEntries by reference (mraft_handle_append_entries, entry_terms NULL):
// the claims and the set heads (sethd, one byte per item), then the main and
// the deferred launch, every count on the device.
void launch_claim_ae(const mraft_ae_args *args, int64_t n, int64_t n_log, int L, int64_t gp, int ni,
                     unsigned long long *claim, uint32_t *srcmark, uint32_t epoch, int32_t *err, uint8_t *sethd,
                     unsigned long long *total, hipStream_t st);
// The by-reference handler's stripes (the main launch workgroup's XCD): stripe
// x lists its deferred items at defer[x * n] (the list buffer holds
// kAeStripes * n) and stages at stage[x * capacity / kAeStripes].
#ifndef MRAFT_AE_STRIPES
#define MRAFT_AE_STRIPES 8
#endif
constexpr int kAeStripes = MRAFT_AE_STRIPES;
// Its counter buffer (HsArgs::total, u64 words): two single words, then per
// stripe x one 128-B line (kAeCntStripe words) at kAeCntDeferred and one at
// kAeCntStaged, word + kAeCntStripe * x. k_claim_ae arms all but the
// published count for each call.
constexpr int kAeCntPublished = 2;     // the deferred count last published to the host's pinned word
constexpr int kAeCntFbDone = 3;        // the fallback's stripes whose workgroups have all finished
constexpr int kAeCntStripe = 16;
constexpr int kAeCntDeferred = 16;                        // stripe x's deferred items
constexpr int kAeCntFbStripeDone = kAeCntDeferred + 1;    // the fallback's finished workgroups of stripe x (same line)
constexpr int kAeCntStaged = kAeCntDeferred + kAeStripes * kAeCntStripe;  // stripe x's staged words
constexpr int kAeTotalWords = kAeCntStaged + kAeStripes * kAeCntStripe;

// Every argument of the handler kernels (k_handle_set, k_handle_deferred), as
// their one kernel argument, which the host fills (mraft_abi_msg.hip). Field
// order and types are the kernels' argument layout.
struct HsArgs {
  Dev s;
  const mraft_ae_args *args;
  int64_t n;
  const int32_t *ent0;  // entries in a caller buffer (launch_handle_ae_host)
  int64_t n_ent0;
  int32_t *stage;       // staged entries of deferred `read` items (the cycle buffer in the fallback)
  int64_t stage_cap;    // its capacity in words
  int64_t *soff;        // per deferred item: its staged offset, or -2 (in place)
  const uint8_t *sethd; // per item: the size of the set it heads, else 0
  int64_t *defer;       // the deferred items, a list of n per stripe
  unsigned long long *total;  // the counter buffer (kAeCnt*, kAeTotalWords words)
  const unsigned long long *claim;
  const uint32_t *srcmark;
  uint32_t epoch;
  // The deferred launch's fallback (staged words past the stage capacity),
  // per item, written by the main launch for its deferred items:
  int4 *fb;                  // {claimant of the row it reads (its writer, fb_writer), readers of its
                             // row already run, run flag, short-cycle readiness at the cycle's
                             // smallest item}: one 16-B record, zeroed but the first word
  unsigned long long *kin;   // epoch-tagged count of the deferred items that read this item's row
  int32_t *cslot;            // per-workgroup cycle buffers, nslot x L words
  int nslot;
  int32_t *cyc;              // the last workgroup's cycle buffer (L words)
  long long *hint;           // pinned host words: [0] the last deferred count (the next call's grid),
                             // [1] staged words of the last batch that exceeded the stage
  mraft_ae_reply *rep;
  int32_t *err;
  mraft_ae_result *res;  // optional: each item's reply as its co-resident leader folds it
};
// The fallback's `order` buffer, one allocation behind fb, cyc and cslot: n
// records, the L-word buffer, nslot cycle buffers (ka.n, ka.s.L and ka.nslot
// set). Returns its size in bytes and, given the buffer, points the three at
// their parts.
inline size_t ae_order_carve(HsArgs &ka, void *order) {
  const size_t n = (size_t)ka.n, L = (size_t)ka.s.L;
  if (order) {
    ka.fb = (int4 *)order;
    ka.cyc = (int32_t *)(ka.fb + n);
    ka.cslot = ka.cyc + L;
  }
  return n * sizeof(int4) + (1 + (size_t)ka.nslot) * L * sizeof(int32_t);
}
// The main launch (ni messages per set at most) and the deferred launch on
// `grid` workgroups, the host's choice from the last call's deferred count.
void launch_handle_ae_ref(const HsArgs &ka, int ni, int grid, hipStream_t st);
// AppendEntries with the entries in a caller buffer (claims by launch_claim).
void launch_handle_ae_host(const Dev &s, const mraft_ae_args *args, int64_t n, const int32_t *ent, int64_t n_ent,
                           mraft_ae_reply *rep, int32_t *err, mraft_ae_result *res, hipStream_t st);

// ---------------------------------------------------------------- mraft_handle_deferred.hip
// The deferred launch alone (launch_handle_ae_ref enqueues it after the main
// launch): k_handle_deferred, grid-stride over the deferred items.
void launch_handle_deferred(const HsArgs &ka, int grid, hipStream_t st);

// ---------------------------------------------------------------- mraft_fold.hip
void launch_fold(const Dev &s, const mraft_ae_result *items, int64_t n, const int64_t *seg_begin,
                 int64_t n_seg, int64_t gp, unsigned long long *claim, uint32_t epoch, int32_t *seg_err,
                 int32_t *flags, int32_t *item_err, void *scan_buf, hipStream_t st);
size_t fold_scan_bytes(int64_t n, int64_t n_seg);  // scratch launch_fold needs (a1 scan list, long segments)

// ---------------------------------------------------------------- mraft_tick.hip
// `reach` (here and in every launcher below that takes it): the groups'
// reachability bytes (mraft_set_reachable), or null when no mask is set. Null
// launches the kernels as they are without the feature; a mask launches the
// same templates with the reachability pack (mraft_device.h), which compiles
// the mask's tests into their bodies.
void launch_replicate_tick(const Dev &s, const int32_t *lpeer, int32_t *gflags, int32_t *exp_commit,
                           int32_t *exp_term_leader, const uint8_t *reach, hipStream_t st);
// The light tick (MRAFT_TICK_LIGHT): k_tick_lite (mraft_tick_lite.hip)
// settles the steady-state groups eight per wave, kLiteBlockGroups per
// workgroup, and lists the others, per XCD: list region x =
// [x * lite_cap(G), ...), its count at cnt[kLiteCntStride * x] (eight
// counters, one 128-B line each); the fallback launch (k_tick_list here, grid
// workgroups, grid-stride) runs them through the full tick, zeroes cnt_next
// (the next light tick's counters) and writes the total to the pinned host
// word hint. A list of G groups needs at most lite_list_words(G) words.
constexpr int kLiteBlockGroups = 32;
constexpr int kLiteCntStride = 32;
constexpr int kLiteCntWords = 8 * kLiteCntStride;  // one light tick's counters
constexpr int lite_blocks(int G) { return (G + kLiteBlockGroups - 1) / kLiteBlockGroups; }
constexpr int lite_cap(int G) { return (lite_blocks(G) + 7) / 8 * kLiteBlockGroups; }
constexpr int64_t lite_list_words(int G) { return 8 * (int64_t)lite_cap(G); }
// One list buffer serves every tick shard: the shard s of groups
// [g0, g0 + G_s) owns the words from lite_list_begin(g0, s), which the next
// shard's region cannot reach: 8 * lite_cap(G_s) <= kLiteBlockGroups *
// (lite_blocks(G_s) + 7) <= G_s + 8 * kLiteBlockGroups - 1, met at G_s = 257.
constexpr int kLiteListSlack = 512;  // words of a shard's region beyond its groups
static_assert(8 * kLiteBlockGroups - 1 <= kLiteListSlack && lite_list_words(257) == 257 + 8 * kLiteBlockGroups - 1,
              "a shard's list fits its region");
constexpr int64_t lite_list_begin(int g0, int s) { return g0 + (int64_t)kLiteListSlack * s; }
// The buffer for G groups in at most `shards` shards.
constexpr int64_t lite_list_alloc_words(int G, int shards) { return lite_list_begin(G, shards); }
struct LiteBufs {
  int32_t *list;
  unsigned *cnt, *cnt_next;
  long long *hint;
  int grid;
};
// The fallback launch alone, for P >= 2 (launch_replicate_tick_light enqueues
// it after k_tick_lite).
void launch_tick_list(const Dev &s, const int32_t *lpeer, int32_t *gflags, int32_t *exp_commit,
                      int32_t *exp_term_leader, const LiteBufs &lb, const uint8_t *reach, hipStream_t st);
// The algorithmic count's buffer (mraft_replicate_tick_count): kCountStripes
// stripes of {reads, writes, active groups}, one 128-B line each, by
// workgroup (one counter word per buffer took every wave's atomic in turn:
// 1.8 ms per config-#3 count); the host sums the stripes.
constexpr int kCountStripes = 64;
constexpr int kCountWords = 16;
void launch_replicate_tick_count(const Dev &s, const int32_t *lpeer, unsigned long long *counts,
                                 hipStream_t st);

// ---------------------------------------------------------------- mraft_tick_lite.hip
// The light tick's pair of launches; sio: Start at the leaders first, inside
// k_tick_lite. With P == 1 the full tick (a lane per group already).
void launch_replicate_tick_light(const Dev &s, const int32_t *lpeer, int32_t *gflags, int32_t *exp_commit,
                                 int32_t *exp_term_leader, const LiteBufs &lb, const StartIO *sio,
                                 const uint8_t *reach, hipStream_t st);

// ---------------------------------------------------------------- mraft_elect.hip
void launch_election_rounds(const Dev &s, const uint8_t *cand, int R, int32_t *gflags, const uint8_t *reach,
                            hipStream_t st);

// ---------------------------------------------------------------- mraft_clock.hip
// Timers (include/mraft.h "timers"): the two deadline arrays of a handle with
// its configuration.
struct TimerDev {
  int32_t *ed, *hd;  // election_due, heartbeat_due [G*P]
  mraft_timer_config cfg;
};
void launch_timers_arm_all(const TimerDev &t, int64_t gp, int32_t now, hipStream_t st);
void launch_timers_arm(const TimerDev &t, const int32_t *slots, int64_t n, int64_t gp, int32_t now,
                       hipStream_t st);
// mraft_ticker: an ordered compaction of two lists. bcnt holds
// 2 * ticker_blocks(gp) words: the election list's block counts, then the
// heartbeat list's.
inline int64_t ticker_blocks(int64_t gp) { return compact_blocks(gp); }
void launch_ticker(const Dev &s, const TimerDev &t, int32_t now, int32_t *bcnt, int32_t *oe, int64_t cap_e,
                   int64_t *n_e, int32_t *oh, int64_t cap_h, int64_t *n_h, hipStream_t st);
void launch_timers_note(const TimerDev &t, int kind, const void *records, const void *outcome,
                        const int32_t *item_err, int64_t n, int64_t gp, int32_t now, hipStream_t st);
// mraft_clock_step A-C (ticker, one election round, the sender; lpeer and tg,
// the sender's term, are required) and E (the tick's resets).
void launch_clock_round(const Dev &s, const TimerDev &t, int32_t now, uint32_t flags, uint8_t *cand,
                        int32_t *lpeer, int32_t *tg, int32_t *eflags, const uint8_t *reach, hipStream_t st);
void launch_clock_resets(const Dev &s, const TimerDev &t, int32_t now, const int32_t *gflags,
                         const int32_t *lpeer, const int32_t *tg, const uint8_t *reach, hipStream_t st);

}  // namespace mraft
