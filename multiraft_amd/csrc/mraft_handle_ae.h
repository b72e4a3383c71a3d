// mraft_handle_ae.h — what the two units of the message-level AppendEntries
// handler compile (mraft_handle_ae.hip: the claims and the main launch;
// mraft_handle_deferred.hip: the deferred launch and its ordered fallback):
// the keys that cut the batch into sets, the item classes and entry modes, the
// small device helpers, the main launch's deferral bookkeeping (defer_lanes)
// and the handler of one set of messages (handle_one). Private, like
// mraft_pass.h, whose streaming pass handle_one runs.
#pragma once
#include "mraft_device.h"
#include "mraft_internal.h"
#include "mraft_pass.h"
#include "mraft_rules.h"

namespace mraft {
namespace {

// The main launch's deferred list and stage offsets are counted per stripe
// (the workgroup's XCD, blockIdx % 8), each counter on its own 128-B line of
// the counter buffer (mraft_internal.h kAeCnt*, kAeTotalWords u64): one
// same-address counter took an atomic round trip per deferred item and per
// staged item, serialised — 1.3 ms of a 2-cycle-heavy batch (r6_l7). Stripe x
// lists its items at defer[x * n ...] and stages at stage[x * cap / 8 ...].
constexpr int kStripes = kAeStripes;
static_assert(16 + 2 * kStripes * 16 == kAeTotalWords, "the counter buffer's layout (mraft_internal.h)");

// ---------------------------------------------------------------- a4
// HandleAppendEntries (raft_append_entry.go:108-162, matchLog
// raft_log.go:92-96), message-level, fully on the device: the host enqueues
// three launches and returns (round 5; rounds 2-4 polled a pinned word for
// the batch plan before enqueuing the second half).
//
// Entries by reference into the engine's own log (entry_terms NULL):
// entries_offset = source slot * L + (Index - dummy) of the first entry, a
// logical position in that replica's ring. The reference copies args.Entries
// when it builds the message (appendOneRound, raft_append_entry.go:50-54),
// before any handler runs, so every item must see its source row as it was
// before the call, even when another item of the batch writes that row (two
// leaders of one group). Per item, from the claims of k_claim_ae (the lowest
// item addressed to a slot owns it; srcmark marks every row some item reads):
//   read   its source row is written by an item of this batch (claimed);
//   written  its own slot is some item's source row (srcmark).
// An item that is not `written` runs in the MAIN launch, reading its source in
// place (a row some item reads and another writes belongs to a `written`
// item, which is deferred: the row is pristine throughout the main launch).
// A `written` item is DEFERRED to a second launch,
// after every main item has read what it needs; if it is also `read`, its
// entries are staged (copied by the main launch, whose items never write the
// rows deferred items read) and the deferred launch reads the copy. Deferred
// items are independent given the copies and run in parallel. When the
// staged words exceed the stage capacity (mraft_set_stage_capacity), the
// deferred launch instead orders them itself on one wave: an item that reads a
// row runs before that row's writer (each item has at most one writer ahead of
// it, so the order is a forest of chains feeding cycles), and a cycle is
// broken by copying one member's entries to an L-word buffer first.
//
// Messages that read the same entries (same source row, same ring position of
// Index 0, same last Index: the P-1 messages one leader's gather makes for
// its followers, consecutive in the batch) form a *set*, up to NI messages,
// served by one wave with one streaming pass over the shared entries, as the
// fused tick serves a group (mraft_pass.h). k_claim_ae cuts the sets from the
// keys alone (a message whose run of same-entry predecessors is NI or longer is
// a set of its own) and writes each head's size; the main launch's wave v
// serves the sets whose heads lie in items [v*NI, (v+1)*NI) — one set per
// wave for a gathered batch — masking members that turn out to be
// duplicates, malformed or deferred.
struct AeKey {
  int64_t row;  // source slot (-1: no key, a set of its own)
  int base;     // ring position of the entries, relative: (offset mod L) - (prev + 1)
  int end;      // Index of the last entry
};

__device__ __forceinline__ bool ae_ref_ok(const mraft_ae_args &a, int64_t n_log, int L) {
  return !(a.n_entries < 0 || a.entries_offset < 0 || a.entries_offset + a.n_entries > n_log ||
           a.entries_offset % L + a.n_entries > L);
}

// The Index domain (include/mraft.h): the last entry's Index prev + n must
// leave room for nextIndex = Index + 1 in int32. Outside it the item is
// malformed (MRAFT_ITEM_BAD_SLOT), as in the oracle.
__device__ __forceinline__ bool ae_index_ok(const mraft_ae_args &a) {
  return index_in_domain((int64_t)a.prev_log_index + a.n_entries);
}

__device__ __forceinline__ AeKey ae_key(const mraft_ae_args &a, int64_t gp, int64_t n_log, int L) {
  if (a.slot < 0 || a.slot >= gp || !ae_ref_ok(a, n_log, L) || !ae_index_ok(a)) return AeKey{-1, 0, 0};
  return AeKey{a.entries_offset / L, (int)(a.entries_offset % L) - (a.prev_log_index + 1),
               a.prev_log_index + a.n_entries};
}

__device__ __forceinline__ bool same_key(const AeKey &x, const AeKey &y) {
  return x.row >= 0 && x.row == y.row && x.base == y.base && x.end == y.end;
}

// a4 for one set of messages per wave: lane q < size takes message first+q's
// prologue (its args, the claims, the receiving follower's scalars,
// log[prev]); conflict scans run wave-wide one message at a time; every
// merging message joins one streaming pass over the shared entries
// (mraft_pass.h).
enum : int { AE_DEFER = -1, AE_NONE = 0, AE_DONE, AE_BAD, AE_STALE, AE_BELOW, AE_MISS, AE_MERGE };
// The three ways handle_one is entered.
enum : int {
  HM_MAIN = 0,   // by reference, the main launch: classify, defer `written` items
  HM_DEFER = 1,  // by reference, a deferred item: entries staged (soff >= 0) or in place (-2)
  HM_HOST = 2,   // entries in a host-supplied buffer: one message per wave, nothing deferred
  HM_ORDER = 3   // by reference, the ordered fallback: entries in place (-2) or the cycle buffer (0)
};

#ifndef MRAFT_AE_MINW
#define MRAFT_AE_MINW 8  // __launch_bounds__ minimum waves per SIMD of the handler
#endif
// The deferred launch's: its register needs do not fit 8 waves per SIMD (the
// compiler reported 7 against a request of 8); asked for 7 its code is the
// allocator's own choice at that occupancy (profiles/r6_d6: deferred-heavy
// batches within noise or faster, the handler tests green)
#ifndef MRAFT_AE_DMINW
#define MRAFT_AE_DMINW 7
#endif

// The handler's persist mark at the end of a set's wave as a non-returning
// atomic OR: the wave does not wait for a load of the bits (a dependent round
// trip at its very end). Same-box A/B: handle call -8 us on average over three
// passes (profiles/r3_v8/message_path_ab.txt, r3w); the same change in the
// fused tick measured +0.7 % there and is not used.
__device__ __forceinline__ void mark_persist_ae(const Dev &s, int64_t slot, int bits) {
  if (s.pdirty && bits) (void)__hip_atomic_fetch_or(&s.pdirty[slot], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The kernels' one argument (HsArgs, mraft_internal.h) read afresh from the
// kernel-argument segment: the handler re-reads it after the streaming pass
// instead of holding ~16 pointers live across it (at 8 waves per SIMD they
// spilled through VGPR lanes to scratch: 28 B per lane, ~100 MB of scratch
// write-back per config-#3 call).
__device__ __forceinline__ HsArgs reload_hs() {
  const __attribute__((address_space(4))) HsArgs *kp =
      (const __attribute__((address_space(4))) HsArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  HsArgs k;
  k.s.term = kp->s.term; k.s.voted = kp->s.voted; k.s.role = kp->s.role; k.s.commit = kp->s.commit;
  k.s.applied = kp->s.applied; k.s.dummy = kp->s.dummy; k.s.last = kp->s.last; k.s.votes = kp->s.votes;
  k.s.log = kp->s.log; k.s.match = kp->s.match; k.s.next = kp->s.next; k.s.pdirty = kp->s.pdirty;
  k.s.head = kp->s.head; k.s.hsnap = kp->s.hsnap; k.s.srt = kp->s.srt; k.s.G = kp->s.G; k.s.P = kp->s.P; k.s.L = kp->s.L;
  k.args = kp->args; k.n = kp->n; k.ent0 = kp->ent0; k.n_ent0 = kp->n_ent0; k.stage = kp->stage;
  k.stage_cap = kp->stage_cap; k.soff = kp->soff; k.sethd = kp->sethd; k.defer = kp->defer; k.total = kp->total;
  k.claim = kp->claim; k.srcmark = kp->srcmark; k.epoch = kp->epoch; k.fb = kp->fb; k.kin = kp->kin;
  k.cslot = kp->cslot; k.nslot = kp->nslot; k.cyc = kp->cyc; k.hint = kp->hint;
  k.rep = kp->rep; k.err = kp->err; k.res = kp->res;
  return k;
}

// The args half of a failed item's reply record (slot = peer = -1), built
// where it is stored: as a plain constant the compiler kept it in four VGPRs
// from the prologue on and spilled them (a 16-B scratch store per lane in
// every wave of the main launch).
__device__ __forceinline__ int4 no_record() {
  int m = -1, z = 0;
  asm volatile("" : "+v"(m), "+v"(z));
  return make_int4(m, m, z, z);
}

// The number of set bits of m below this lane (v_mbcnt: no per-lane mask
// register, which the compiler would hoist and hold across the pass).
__device__ __forceinline__ int lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ int at_load(int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void at_store(int32_t *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// This wave's own global stores complete before its next loads (a copy it
// reads back): workgroup scope, no cache maintenance.
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_s_waitcnt(0);
}

// Epoch-tagged counters (high 32 bits: the call's epoch; a stale tag reads as
// 0), so no call has to zero them before counting.
__device__ __forceinline__ void tag_inc(unsigned long long *p, uint32_t epoch) {
  unsigned long long old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const unsigned long long nv =
        (uint32_t)(old >> 32) == epoch ? old + 1 : (((unsigned long long)epoch << 32) | 1ull);
    if (__hip_atomic_compare_exchange_strong(p, &old, nv, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
  }
}
__device__ __forceinline__ int tag_count(const unsigned long long *p, uint32_t epoch) {
  const unsigned long long v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (uint32_t)(v >> 32) == epoch ? (int)(uint32_t)v : 0;
}

// The main launch's bookkeeping for the `written` lanes of a wave (rare: a
// stale leader both sending and receiving in one batch): their place in the
// deferred list, and for those that also `read`, a staged offset and the copy
// of their entries (the source row is pristine: its writer is deferred too).
__device__ __forceinline__ void defer_lanes(const HsArgs &k0, bool dfr, bool stg, int64_t i, int n, const int32_t *row,
                                            int head, int from, int L, int wraw) {
  const unsigned long long m = __ballot(dfr);
  const int lane = lane_id(), q0 = first_lane(m);
  const int x = (int)(blockIdx.x & (kStripes - 1));  // this workgroup's stripe
  unsigned long long b = 0;
  if (lane == q0) b = atomicAdd(&k0.total[kAeCntDeferred + kAeCntStripe * x], (unsigned long long)__popcll(m));
  b = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(b >> 32), q0) << 32) |
      (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, q0);
  if (dfr) {
    k0.defer[x * k0.n + (int64_t)b + lanes_below(m)] = i;
    int64_t in_place = -2;  // made here (as a hoisted constant pair it was spilled across the pass)
    asm volatile("" : "+v"(in_place));
    if (!stg) k0.soff[i] = in_place;
    // the fallback's graph (used only when the staged words pass the stage
    // capacity): the claimant of the row this item reads (its writer when that
    // claimant is deferred too, which the fallback checks: fb_writer), its
    // count of readers there, and this item's own counters zeroed
    k0.fb[i] = make_int4(wraw, 0, 0, 0);  // one store (four separate arrays spilled the main launch)
    if (wraw >= 0) tag_inc(&k0.kin[wraw], k0.epoch);
  }
  // the staged lanes' offsets: one atomic per wave on the stripe's counter
  // (an exclusive scan of their sizes), the copies one by one on the wave
  const unsigned long long smask = __ballot(stg);
  if (!smask) return;
  const int64_t cap8 = k0.stage_cap / kStripes;  // stripe x stages in [x cap8, (x + 1) cap8)
  int64_t pre = stg ? (int64_t)n : 0;  // inclusive scan of the staged sizes over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t v = __shfl_up(pre, o, 64);
    if (lane >= o) pre += v;
  }
  const int64_t tot = __shfl(pre, 63, 64);
  unsigned long long sb = 0;
  if (lane == first_lane(smask)) sb = atomicAdd(&k0.total[kAeCntStaged + kAeCntStripe * x], (unsigned long long)tot);
  sb = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(sb >> 32), first_lane(smask)) << 32) |
       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)sb, first_lane(smask));
  const int64_t my = (int64_t)sb + pre - (stg ? (int64_t)n : 0);  // this lane's offset within the stripe
  if (stg) k0.soff[i] = x * cap8 + my;
  for (unsigned long long sm = smask; sm; sm &= sm - 1) {
    const int q = first_lane(sm);
    const int nq = __builtin_amdgcn_readlane(n, q);
    const int64_t oq = ((int64_t)__builtin_amdgcn_readlane((int)((uint64_t)my >> 32), q) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)my, q);
    const long long o = x * cap8 + oq;
    if (oq + nq <= cap8) {  // past the stripe's capacity the deferred launch takes the ordered fallback
      const uint64_t ra = (uint64_t)(uintptr_t)row;
      const int32_t *rq = (const int32_t *)(uintptr_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(ra >> 32), q) << 32) |
                                                      (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ra, q));
      wave_copy_from_ring(rq, 0, __builtin_amdgcn_readlane(head, q), L, __builtin_amdgcn_readlane(from, q),
                          k0.stage + o, nq);
    }
  }
}

template <int NI, int MODE>
__device__ __forceinline__ void handle_one(const HsArgs &k0, int64_t first, int size, int64_t so_force = -2) {
  const Dev &s = k0.s;
  const mraft_ae_args *__restrict__ args = k0.args;
  const int lane = lane_id();
  const bool mine = lane < size;
  int64_t i = first + (mine ? lane : 0);
  // Three round trips before the pass: the item (error word, args[, staged
  // offset]), the claims with the follower's scalars and the source's ring
  // head, then log[prev] (and the first entry, for a sorted-terms claim).
  const int e = mine ? k0.err[i] : 1;
  mraft_ae_args a = args[i];
  const int64_t so0 = MODE == HM_DEFER ? k0.soff[i] : so_force;  // HM_ORDER: the caller's choice
  asm volatile("" ::"v"(a.slot), "v"(a.term), "v"(a.prev_log_index), "v"(a.prev_log_term),
               "v"(a.n_entries), "v"(a.leader_commit), "v"(a.entries_offset), "v"(so0));
  // L re-read per set: the division by it (a reciprocal) is then computed here,
  // not hoisted out of the wave's loop over sets and held across the pass
  int L = s.L;
  asm volatile("" : "+s"(L));
  const int64_t gp = (int64_t)s.G * s.P;
  int f = a.slot;
  const int prev = a.prev_log_index, nn = a.n_entries;
  // every word that depends only on the args, in one round trip (e == 0: the
  // slot is in range; the follower's words are read before the claims decide
  // whether the item runs here: no extra dependent round trip)
  int fterm = 0, fdummy = 0, flast = 0, fc = 0, fhead = 0;
  if (!e) { fterm = s.term[f]; fdummy = s.dummy[f]; flast = s.last[f]; fc = s.commit[f]; fhead = s.head[f]; }
  // Where the entries are: Index x of this lane's message at src.at(x). A
  // flat source (host buffer, staged copy, cycle buffer) is built relative to
  // its first entry (row = that entry's word, base = -(prev + 1)), so at()'s
  // 32-bit lane offset is x - (prev + 1), small whatever the Raft Index
  // (flat_src; an absolute Index above 2^30 wrapped it).
  RingRow src = flat_src(k0.ent0, 0, prev);
  int64_t n_ent = k0.n_ent0;
  bool ok = true, dup = false, dfr = false, stg = false;
  int64_t srow = 0;  // by reference: the source row
  int rhead = 0;
  unsigned long long cr = 0;  // HM_MAIN: the claim word of the source row
  if (MODE == HM_HOST) {
    if (!e) src = flat_src(k0.ent0, a.entries_offset, prev);
  } else if (!e) {
    ok = ae_ref_ok(a, gp * L, L);
    srow = ok ? a.entries_offset / L : 0;
    unsigned long long cs = 0;
    uint32_t sm = 0;
    if (MODE == HM_MAIN) {
      cs = k0.claim[f];
      sm = k0.srcmark[f];
      if (ok && nn > 0) cr = k0.claim[srow];
    }
    // (the offset may name the end of the log image: (slot + 1) L, the heartbeat
    // of a full-log leader at the last slot. srow = G P then: no row, no head.
    // Any other heartbeat's head is needed: it may be the first merging member
    // of a set, whose source every member's entries are read through)
    if (ok && srow < gp) rhead = s.head[srow];
    if (MODE == HM_MAIN) {
      dup = !claim_won(cs, k0.epoch, i);
      dfr = !dup && ok && sm == k0.epoch;                              // `written`: deferred
      stg = dfr && nn > 0 && (uint32_t)(cr >> 32) == k0.epoch;        // and `read`: staged
    }
    const int64_t so = MODE == HM_MAIN ? -2 : so0;
    if (so >= 0) {  // staged copy (or the fallback's cycle buffer)
      src = flat_src(k0.stage, so, prev);
      n_ent = k0.stage_cap;  // (HM_ORDER: the cycle buffer, capacity L)
      a.entries_offset = so;
    } else {        // in place through the source ring
      src.p = s.log;
      src.row = srow * L;
      src.L = L;
      src.base = rhead + (int)(a.entries_offset % L) - (prev + 1);
      n_ent = INT64_MAX;
    }
  }
  int cls = e ? AE_NONE : AE_DONE;
  if (dup) cls = AE_NONE;
  else if (dfr) cls = AE_DEFER;
  else if (!e && (!ok || nn < 0 || a.entries_offset < 0 || !ae_index_ok(a) ||
                  (nn > 0 && src.L == INT32_MAX && a.entries_offset + nn > n_ent)))
    cls = AE_BAD;
  const bool live = cls == AE_DONE;
  if (dup && mine) k0.err[i] = MRAFT_ITEM_DUP_SLOT;
  if (MODE == HM_MAIN && __ballot(dfr)) {
    // the claimant of the row this item reads (from the claim word loaded above),
    // for an item that reads anything (the writer check is the fallback's)
    const int wraw = (nn > 0 && ae_index_ok(a) && (uint32_t)(cr >> 32) == k0.epoch) ? claim_index(cr) : -1;
    defer_lanes(k0, dfr, stg, i, nn, s.log + srow * L, rhead, (int)(a.entries_offset % L), L, wraw);
  }
  if (k0.res && mine && cls != AE_DEFER) {
    // the args half of the item's reply record for its co-resident leader's
    // fold, stored now (no reload of the args at the wave's end); the reply
    // half follows with the reply. Failed items: slot = peer = -1.
    int PP = s.P;
    asm volatile("" : "+s"(PP));  // (the division's reciprocal made here, not hoisted and spilled)
    int4 *rr = reinterpret_cast<int4 *>(k0.res + i);
    rr[0] = live ? make_int4((f / PP) * PP + a.leader_id, f % PP, a.term, prev) : no_record();
  }
  // MRAFT_AE_ENTRIES_SORTED is the sender's claim (it crosses the network):
  // honoured only where the terms prevLogTerm, entry 0, ... really never
  // decrease. Here the first step (prevLogTerm <= entry 0, in the round trip
  // of the follower's log[prev]); the entries themselves are checked on the
  // pass's loads (DescTrack). Same rule in the oracle (ae_flag_holds).
  const bool claim = live && nn > 0 && (a.flags & MRAFT_AE_ENTRIES_SORTED) != 0;
  const bool claim0 = claim && a.prev_log_term <= *src.at(prev + 1);
  mraft_ae_reply r = {0, 0, 0, 0};
  int ftp = 0;
  if (live) {
    if (a.term < fterm) {                                              // :112-115
      cls = AE_STALE;
      r.term = fterm;
    } else if (prev < fdummy) {                                        // :123-127
      cls = AE_BELOW;
      r.conflict_index = fdummy + 1;
    } else {
      ftp = prev > flast ? 0 : s.log[(int64_t)f * L + ring(prev - fdummy + fhead, L)];
      if (prev > flast || ftp != a.prev_log_term) {                    // matchLog, raft_log.go:92-96
        cls = AE_MISS;
        r.term = a.term;
        if (prev > flast) r.conflict_index = flast + 1;                // :131-133
        else r.conflict_index = prev;                                  // :136-142 below when prev > dummy + 1
      } else {
        cls = AE_MERGE;
      }
    }
  }
  // :136-142, the ConflictIndex scan, wave-wide for one message at a time
  for (unsigned long long m = __ballot(cls == AE_MISS && prev <= flast && prev > fdummy + 1); m; m &= m - 1) {
    const int q = first_lane(m);
    const int qf = __shfl(f, q, 64), qd = __shfl(fdummy, q, 64), qh = __shfl(fhead, q, 64),
              qp = __shfl(prev, q, 64), qa = __shfl(ftp, q, 64);
    const int ci = wave_conflict_scan(s.log + (int64_t)uni(qf) * L, uni(qd), uni(qh), L, uni(qp), uni(qa));
    if (lane == q) r.conflict_index = ci;
  }
  // :146-155 through the streaming pass the tick uses: compare entries with
  // every merging follower's terms, truncate-and-append from the first
  // mismatch. All messages of a set end at the same Index (AeKey).
  int newlast = -1, fcommit_new = -1, srt_new = -1;
  const int merge_m = (int)(__ballot(cls == AE_MERGE) & ((1ull << NI) - 1));
  // terms_sorted after an append from Index k (include/mraft.h): the args'
  // flag when k - 1 is the dummy, cleared without it, else unchanged — the
  // flag as checked (claim0 here, the entries' descents after the pass);
  // shint: -1 no flag, 1 flag and prev is the dummy, 0 flag otherwise
  int shint = claim0 ? (prev == fdummy ? 1 : 0) : -1;
  if (merge_m) {
    Fol<NI, true> fo;
    fo.log = s.log;
    fo.slot0 = 0;
    fo.skip = NI;
    fo.L = L;
    fo.cmp = merge_m;
    fo.copy = 0;
    fo.capok = (int)(__ballot(cls == AE_MERGE && (int64_t)prev + nn - fdummy <= (int64_t)L - 1) & ((1ull << NI) - 1));
    fo.full = 0;
    const int phi = uni(__shfl(prev + nn, first_lane((unsigned long long)merge_m), 64));
    int plo = phi + 1;
#pragma unroll
    for (int q = 0; q < NI; ++q)
      if ((merge_m >> q) & 1) plo = min(plo, uni(__shfl(prev, q, 64)) + 1);
    // The pass runs on Indexes relative to B = plo - kPassBias (pass_bias):
    // every Index it forms stays in [kPassBias - 35, kPassBias + L + 256], so
    // no chunk end (c + 256) overflows int32 near 2^31 and the lane offsets a
    // source's at() forms stay small. Rows see the same words (their bases
    // absorb B).
    const int B = pass_bias(plo);
    const int pl = plo - B, ph = phi - B, nend = ph + 1;
    // the source as the first merging message sees it (the same for every message of a set)
    const int q0 = first_lane((unsigned long long)merge_m);
    RingRow ss;
    {
      const uint64_t pa = (uint64_t)(uintptr_t)src.p;
      const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)pa, q0, 64), hi = (uint32_t)__shfl((int)(pa >> 32), q0, 64);
      ss.p = (const int32_t *)(uintptr_t)(((uint64_t)uni((int)hi) << 32) | (uint32_t)uni((int)lo));
      const uint64_t ra = (uint64_t)src.row;
      const uint32_t rlo = (uint32_t)__shfl((int)(uint32_t)ra, q0, 64), rhi = (uint32_t)__shfl((int)(ra >> 32), q0, 64);
      ss.row = (long long)(((uint64_t)uni((int)rhi) << 32) | (uint32_t)uni((int)rlo));
      ss.base = uni(__shfl(src.base, q0, 64)) + B;
      ss.L = uni(__shfl(src.L, q0, 64));
    }
    bool vec = (L & 3) == 0 && ((uintptr_t)s.log & 15) == 0;
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      fo.slot[q] = uni(__shfl(f, q, 64));
      const int sp = uni(__shfl(prev, q, 64)), sl = uni(__shfl(flast, q, 64));
      fo.base[q] = 0; fo.start[q] = 0; fo.cend[q] = 0;
      fo.cfrom[q] = 0;  // 0: no mismatch (a relative Index is >= kPassBias - 35 > 0)
      if ((merge_m >> q) & 1) {  // (only merging messages are ever addressed)
        fo.base[q] = uni(__shfl(fhead - fdummy, q, 64)) + B;
        fo.start[q] = sp + 1 - B;
        fo.cend[q] = min(phi, sl) + 1 - B;
        // dwordx4 when the entries and this follower's row are 16-B aligned alike
        vec = vec && ((((uintptr_t)ss.at(fo.start[q]) ^ (uintptr_t)fo.at(q, fo.start[q])) & 15) == 0);
      }
    }
    if (ss.L == INT32_MAX) {  // a flat buffer: every dwordx4 read must stay inside it
      // its size as the first merging message sees it: n_ent is per lane (a
      // lane with no item keeps the host-buffer size, 0 by reference), and a
      // per-lane `vec` would split the wave between the two passes
      const uint64_t nb = (uint64_t)n_ent;
      const uint32_t nlo = (uint32_t)__shfl((int)(uint32_t)nb, q0, 64), nhi = (uint32_t)__shfl((int)(nb >> 32), q0, 64);
      const int64_t sn = (int64_t)(((uint64_t)uni((int)nhi) << 32) | (uint32_t)uni((int)nlo));
      vec = vec && (((uintptr_t)ss.at(pl)) & ~(uintptr_t)15) >= (uintptr_t)ss.p &&
            (((uintptr_t)ss.at(ph)) | 15) < (uintptr_t)(ss.p + sn);
    }
    // the pass is wave-wide (ballots, shuffles): one choice for every lane
    vec = __ballot(!vec) == 0;
    int found = -1;
    DescTrack dt{__ballot(cls == AE_MERGE && claim0) != 0, 0, INT32_MIN};
    // This lane's reply inputs wait in LDS during the pass (the pass needs
    // the registers: at 8 waves per SIMD they would spill to scratch).
    // (plain LDS stores and loads across a compiler memory barrier: a
    // volatile generic pointer made them flat accesses with 64-bit addresses
    // the compiler hoisted and spilled)
    __shared__ int stash[12][64];
    stash[0][lane] = cls; stash[1][lane] = f; stash[2][lane] = fterm; stash[3][lane] = flast;
    stash[4][lane] = fc; stash[5][lane] = a.term; stash[6][lane] = a.leader_commit;
    stash[7][lane] = r.conflict_index; stash[8][lane] = r.term;
    stash[9][lane] = (int)(uint32_t)(uint64_t)i; stash[10][lane] = (int)((uint64_t)i >> 32);
    stash[11][lane] = shint;
    asm volatile("" ::: "memory");
    if (vec) {
      int c = pl - (int)(((uintptr_t)ss.at(pl) >> 2) & 31);            // 128-B aligned chunks
      if (c <= ph && fo.cmp) c = pass_pipe<false>(ss, fo, nend, 1, 0, 0, found, c, pl, ph, dt);
      copy_loop<true, false>(ss, fo, c, nend, pl, ph, 1, 0, 0, found, dt);
    } else {
      int c = pl;
      for (; c <= ph && fo.cmp; c += 256) pass_chunk<1, false, false>(ss, fo, nend, 1, 0, 0, found, c, pl, ph, dt);
      copy_loop<false, false>(ss, fo, c, nend, pl, ph, 1, 0, 0, found, dt);
    }
    asm volatile("" ::: "memory");
    cls = stash[0][lane]; f = stash[1][lane]; fterm = stash[2][lane]; flast = stash[3][lane];
    fc = stash[4][lane]; a.term = stash[5][lane]; a.leader_commit = stash[6][lane];
    r.conflict_index = stash[7][lane]; r.term = stash[8][lane];
    i = (int64_t)(((uint64_t)(uint32_t)stash[10][lane] << 32) | (uint32_t)stash[9][lane]);
    shint = stash[11][lane];
    // kernel arguments re-read from the kernarg segment, not held across the pass
    const HsArgs kr = reload_hs();
    int32_t *__restrict__ err = kr.err;
    mraft_ae_reply *__restrict__ rep = kr.rep;
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      if (lane != q || cls != AE_MERGE) continue;
      if ((fo.full >> q) & 1) {
        cls = AE_DONE;                                                 // engine capacity: no state change
        err[i] = MRAFT_ITEM_LOG_FULL;
        rep[i] = r;
      } else {
        int last_after = flast;
        if (fo.cfrom[q] > 0) {                                         // truncated and appended
          newlast = last_after = phi;
          // a descent among this message's entries (Index start+1 .. phi)
          // voids its flag
          if (dt.last > fo.start[q]) shint = -1;
          // appended from the dummy's successor (prev == dummy, first mismatch
          // at start): the entries are the whole log
          srt_new = shint < 0 ? 0 : (shint == 1 && fo.cfrom[q] == fo.start[q] ? 1 : -1);
        }
        if (a.leader_commit > fc) fcommit_new = min(a.leader_commit, last_after);  // :157-160
        r.term = a.term; r.success = 1;                                // :161
      }
    }
  }
  const HsArgs kt = reload_hs();
  const Dev &s2 = kt.s;
  int32_t *__restrict__ err2 = kt.err;
  mraft_ae_reply *__restrict__ rep2 = kt.rep;
  if (cls == AE_NONE) {
    if (mine) rep2[i] = r;
  } else if (cls == AE_BAD) {
    rep2[i] = r;
    err2[i] = MRAFT_ITEM_BAD_SLOT;
  } else if (cls == AE_STALE) {
    rep2[i] = r;
    mark_persist_ae(s2, f, MRAFT_PERSIST_STATE);                       // deferred :111
  } else if (cls >= AE_BELOW) {
    if (a.term > fterm) { s2.term[f] = a.term; s2.voted[f] = -1; }    // :116-118
    s2.role[f] = kFollower;                                            // :120
    if (newlast >= 0) s2.last[f] = newlast;
    if (srt_new >= 0) s2.srt[f] = srt_new;
    if (fcommit_new >= 0) s2.commit[f] = fcommit_new;
    mark_persist_ae(s2, f, MRAFT_PERSIST_STATE);                       // deferred :111
    rep2[i] = r;
  }
  mraft_ae_result *__restrict__ res = kt.res;
  if (res && mine && cls != AE_DEFER) {
    // the reply half of the record (nEntries, reply term, success,
    // ConflictIndex); an item rejected after the prologue (capacity: cls
    // AE_DONE) gets slot = peer = -1 as well
    int4 *rr = reinterpret_cast<int4 *>(res + i);
    if (cls == AE_DONE) rr[0] = no_record();
    rr[1] = cls >= AE_STALE ? make_int4(nn, r.term, r.success, r.conflict_index) : make_int4(0, 0, 0, 0);
  }
}

}  // namespace
}  // namespace mraft
