// mraft_rules.h — the item-level rules more than one kernel applies, each
// stated once: the Index domain, the reply segments' prologue, the claim word,
// Start, the applier's message, the quorum order statistic and the GetState
// word with the tick's export of it. Every helper inlines to
// the arithmetic it names (the hot kernels' code is the same with or without).
#pragma once
#include "../../include/mraft.h"
#include "mraft_device.h"

namespace mraft {

// An Index leaves room for nextIndex = Index + 1 in int32 (include/mraft.h):
// at most 2^31 - 2. Outside it a record is malformed, as in the oracle.
__device__ __forceinline__ bool index_in_domain(int64_t idx) { return idx <= (int64_t)INT32_MAX - 1; }

// ---------------------------------------------------------------- segments
// Items [b, e) of segment sg; without seg_begin, item sg alone. False: empty.
__device__ __forceinline__ bool segment_bounds(const int64_t *__restrict__ seg_begin, int64_t sg, int64_t &b,
                                               int64_t &e) {
  b = seg_begin ? seg_begin[sg] : sg;
  e = seg_begin ? seg_begin[sg + 1] : sg + 1;
  return b < e;
}

// The verdict on a reply segment before any state changes: the claim's error
// if it has one, else MRAFT_ITEM_BAD_SLOT unless every item addresses the
// first item's slot from another peer of its group and passes ok(item).
template <class Item, class Ok>
__device__ __forceinline__ int segment_verdict(const Item *__restrict__ items, int64_t b, int64_t e, int P,
                                               int claim_err, Ok ok) {
  if (claim_err) return claim_err;
  const int slot = items[b].slot;
  int bad = 0;
  for (int64_t i = b; i < e; ++i) {
    const Item it = items[i];
    if (it.slot != slot || it.peer < 0 || it.peer >= P || it.peer == slot % P || !ok(it)) bad = MRAFT_ITEM_BAD_SLOT;
  }
  return bad;
}

// A rejected segment: every item the error, no flag.
__device__ __forceinline__ void segment_reject(int64_t b, int64_t e, int bad, int32_t *__restrict__ flags,
                                               int32_t *__restrict__ item_err) {
  for (int64_t i = b; i < e; ++i) { item_err[i] = bad; flags[i] = 0; }
}

// ---------------------------------------------------------------- claims
// The claim word of item (or segment) i in the call with this epoch. Slots
// take it by atomicMax, so the lowest i addressing a slot wins and words of
// earlier calls (lower epochs) never do. claim_index: the item a word names.
__device__ __forceinline__ unsigned long long claim_tag(uint32_t epoch, int64_t i) {
  return ((unsigned long long)epoch << 32) | (0xFFFFFFFFull - (uint64_t)i);
}
__device__ __forceinline__ bool claim_won(unsigned long long word, uint32_t epoch, int64_t i) {
  return word == claim_tag(epoch, i);
}
__device__ __forceinline__ int claim_index(unsigned long long word) { return (int)(0xFFFFFFFFu - (uint32_t)word); }

// The slot item i claims: the slot member (byte offset slot_off of a record
// of `stride` bytes) of record i or, with seg_begin, of segment i's first
// record. False: an empty segment, which claims nothing.
__device__ __forceinline__ bool claim_slot_of(const char *__restrict__ items, int64_t i, int stride, int slot_off,
                                              const int64_t *__restrict__ seg_begin, int32_t &slot) {
  int64_t rec, end;
  if (!segment_bounds(seg_begin, i, rec, end)) return false;
  slot = *(const int32_t *)(items + rec * stride + slot_off);
  return true;
}

// Item i's claim: err[i] and, for a slot in range, the atomicMax.
__device__ __forceinline__ void claim_item(const char *__restrict__ items, int64_t i, int stride, int slot_off,
                                           const int64_t *__restrict__ seg_begin, int64_t gp,
                                           unsigned long long *__restrict__ claim, uint32_t epoch, int32_t *err) {
  int32_t slot;
  if (!claim_slot_of(items, i, stride, slot_off, seg_begin, slot)) { err[i] = 0; return; }
  if (slot < 0 || slot >= gp) { err[i] = MRAFT_ITEM_BAD_SLOT; return; }
  err[i] = 0;
  atomicMax(&claim[slot], claim_tag(epoch, i));
}

// Whether item i (err[i] == 0 after claim_item) lost its slot to a lower item.
__device__ __forceinline__ bool claim_lost(const char *__restrict__ items, int64_t i, int stride, int slot_off,
                                           const int64_t *__restrict__ seg_begin,
                                           const unsigned long long *__restrict__ claim, uint32_t epoch) {
  int32_t slot;
  return claim_slot_of(items, i, stride, slot_off, seg_begin, slot) && !claim_won(claim[slot], epoch, i);
}

// ---------------------------------------------------------------- Start
// Whether k entries after `last` fit the ring of L words (the dummy keeps
// one) and the Index domain; else Start refuses with MRAFT_ITEM_LOG_FULL.
__device__ __forceinline__ bool start_fits(int last, int k, int dummy, int L) {
  return (int64_t)last + k - dummy <= (int64_t)L - 1 && index_in_domain((int64_t)last + k);
}

// Start (raft.go:90-104) of k >= 1 entries at replica sl: Go's (index, term,
// isLeader) and the item error.
struct StartOutcome { int index, term, is_leader, err; };
__device__ __forceinline__ StartOutcome start_at(const Dev &s, int64_t sl, int k) {
  if (s.role[sl] != kLeader) return {-1, -1, 0, 0};                    // :93-95
  const int last = s.last[sl], dummy = s.dummy[sl], t = s.term[sl], h = s.head[sl];
  if (!start_fits(last, k, dummy, s.L)) return {-1, -1, 0, MRAFT_ITEM_LOG_FULL};
  // terms_sorted: k entries of currentTerm after the last one
  if (last > dummy && s.log[sl * s.L + ring(last - dummy + h, s.L)] > t) s.srt[sl] = 0;
  for (int j = 1; j <= k; ++j) s.log[sl * s.L + ring(last + j - dummy + h, s.L)] = t;  // :96-100
  s.last[sl] = last + k;
  mark_persist(s, sl, MRAFT_PERSIST_STATE);                            // :101
  return {last + 1, t, 1, 0};                                          // :103
}

// ---------------------------------------------------------------- applier
// The applier's message for slot i (raft.go:158-204) from its lastApplied la,
// commitIndex ci and hasSnapshot hs (0 for a caller that takes no snapshots):
// the snapshot first (:168-177, cleared once taken; -1, 0 without one), then
// the entries [la + 1, ci] (:179-190; none when from > to), lastApplied advanced (:200).
struct ApplyMsg { int snap_index, snap_term, from, to; };
__device__ __forceinline__ bool apply_pending(int hs, int la, int ci) { return hs != 0 || ci > la; }
__device__ __forceinline__ ApplyMsg apply_slot(const Dev &s, int64_t i, int hs, int la, int ci) {
  ApplyMsg m{-1, 0, la + 1, ci};
  if (hs) {
    m.snap_index = s.dummy[i];
    m.snap_term = s.log[i * s.L + s.head[i]];                          // dummyTerm
    s.hsnap[i] = 0;
  }
  if (ci > la) s.applied[i] = ci;
  return m;
}

// ---------------------------------------------------------------- quorum
// advanceCommitIndexForLeader's order statistic (raft_append_entry.go:91-98)
// over the first P words of m: the h-th largest (h = P/2) of matchIndex[j != me],
// the largest i for which #{j != me : matchIndex[j] >= i} + 1 > P/2. With no
// peer (h = 0) every Index has its quorum.
template <int P, int N>
__device__ __forceinline__ int quorum(const int (&m)[N], int me) {
  static_assert(P <= N, "m holds a word per peer");
  constexpr int h = P / 2;
  if (h == 0) return INT32_MAX;
  int best = INT32_MIN;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (j == me) continue;
    int c = 0;
#pragma unroll
    for (int q = 0; q < P; ++q) c += (q != me && m[q] >= m[j]) ? 1 : 0;
    if (c >= h && m[j] > best) best = m[j];
  }
  return best;
}

// ---------------------------------------------------------------- GetState
// GetState (raft.go:237-246) in one word: currentTerm << 1 | isLeader.
__device__ __forceinline__ int32_t term_leader_word(int term, int role) {
  return (int32_t)(((uint32_t)term << 1) | (role == kLeader ? 1u : 0u));
}

// GetState of the group's exported replica, fused into the tick
// (mraft_replicate_tick_export): commit and the GetState word.
struct Export {
  int32_t *commit, *term_leader;
  __device__ __forceinline__ void put(int g, int c, int t, int role) const {
    if (commit) {
      commit[g] = c;
      term_leader[g] = term_leader_word(t, role);
    }
  }
};

}  // namespace mraft
