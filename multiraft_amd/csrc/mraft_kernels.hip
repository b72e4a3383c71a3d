// mraft_kernels.hip — the small item-level gfx950 kernels behind the C ABI,
// a lane (or a wave) per item: Make, the slot claims, the AppendEntries gather,
// Start, the applier, snapshots, RequestVote and its tally, persistence and
// GetState (the per-message entry points of include/mraft.h).
// The AppendEntries handler lives in mraft_handle_ae.hip and
// mraft_handle_deferred.hip, the reply fold in mraft_fold.hip, the fused
// co-resident tick in mraft_tick.hip and mraft_tick_lite.hip.
#include "mraft_device.h"
#include "mraft_internal.h"
#include "mraft_rules.h"

namespace mraft {

namespace {

constexpr int kBlock = 256;

// Workgroups of the four kernels here whose threads grid-stride over the slots
// (k_init_state, k_collect_apply, k_collect_persist: at most 4,096;
// k_terms_sorted, a wave per slot: at most 65,536). MRAFT_STRIDED_GRID caps
// them further: the small-grid test library compiles this unit with 1, so the
// stride loops run their later passes on a small engine. Host code only.
#ifndef MRAFT_STRIDED_GRID
#define MRAFT_STRIDED_GRID (1 << 30)
#endif
int strided_grid(int64_t n, int cap = 4096) {
  return std::min(blocks_for(n, kBlock), std::min(cap, (int)MRAFT_STRIDED_GRID));
}

// ---------------------------------------------------------------- Make
__global__ void k_init_state(Dev s) {
  const int64_t gp = (int64_t)s.G * s.P;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < gp;
       i += (int64_t)gridDim.x * blockDim.x) {
    // raft.go:53-68,79-80: Follower, term 0, votedFor -1, logs = [dummy{0,0}],
    // commitIndex = lastApplied = dummyIndex.
    s.term[i] = 0; s.voted[i] = -1; s.role[i] = kFollower; s.commit[i] = 0; s.applied[i] = 0;
    s.dummy[i] = 0; s.last[i] = 0; s.votes[i] = 0; s.head[i] = 0; s.hsnap[i] = 0;
    s.srt[i] = 1;  // [dummy] only: nothing after the dummy to be out of order
    if (s.pdirty) s.pdirty[i] = 0;
  }
}

// ---------------------------------------------------------------- claims
__global__ void k_claim(const char *__restrict__ items, int64_t n, int stride, int slot_off,
                        const int64_t *__restrict__ seg_begin, int64_t gp, unsigned long long *__restrict__ claim,
                        uint32_t epoch, int32_t *__restrict__ err) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) claim_item(items, i, stride, slot_off, seg_begin, gp, claim, epoch, err);
}

__global__ void k_claim_check(const char *__restrict__ items, int64_t n, int stride, int slot_off,
                              const int64_t *__restrict__ seg_begin, const unsigned long long *__restrict__ claim,
                              uint32_t epoch, int32_t *__restrict__ err) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n || err[i]) return;
  if (claim_lost(items, i, stride, slot_off, seg_begin, claim, epoch)) err[i] = MRAFT_ITEM_DUP_SLOT;
}

// ---------------------------------------------------------------- a3
__global__ void k_gather_args(Dev s, const int32_t *__restrict__ slots,
                              const int32_t *__restrict__ peers, int64_t n,
                              mraft_ae_args *__restrict__ out, int32_t *__restrict__ err) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int P = s.P, L = s.L;
  const int64_t gp = (int64_t)s.G * P;
  mraft_ae_args a = {};
  int e = 0;
  const int slot = slots[i], peer = peers[i];
  if (slot < 0 || slot >= gp || peer < 0 || peer >= P || peer == slot % P) {
    e = MRAFT_ITEM_BAD_SLOT;
  } else {
    // every word that depends only on the slot in one round trip (the role
    // check does not gate the loads: one dependent round trip fewer)
    const int role = s.role[slot], dummy = s.dummy[slot], last = s.last[slot], head = s.head[slot];
    const int nxt = s.next[(int64_t)slot * P + peer], term = s.term[slot], commit = s.commit[slot];
    const int srt = s.srt[slot];
    const int prev = nxt - 1;                                          // :26
    if (role != kLeader) e = MRAFT_ITEM_BAD_STATE;                     // raft_append_entry.go:22-25
    else if (prev < dummy) e = MRAFT_ITEM_NEED_SNAPSHOT;               // :27
    else if (prev > last) e = MRAFT_ITEM_PREV_BEYOND_LAST;             // :41-43
    else {
      a.slot = (slot / P) * P + peer;
      a.leader_id = slot % P;
      a.term = term;
      a.prev_log_index = prev;
      a.prev_log_term = s.log[(int64_t)slot * L + ring(prev - dummy + head, L)];  // :49
      a.n_entries = last - prev;                                       // :50
      // prevLogTerm, entries: non-decreasing when the leader's terms after its
      // dummy are; prevLogTerm at the dummy itself is compared explicitly
      a.flags = (srt && (prev > dummy || prev == last ||
                         a.prev_log_term <= s.log[(int64_t)slot * L + ring(prev + 1 - dummy + head, L)]))
                    ? MRAFT_AE_ENTRIES_SORTED : 0;
      a.leader_commit = commit;                                        // :51
      a.entries_offset = (int64_t)slot * L + (prev + 1 - dummy);       // :54 (by reference: logical)
    }
  }
  out[i] = a;
  err[i] = e;
}

// ---------------------------------------------------------------- Start
// The duplicate-slot check (k_claim_check's) is done here, on the claim word
// k_claim left: one launch fewer per Start call.
__global__ void k_start(Dev s, const int32_t *__restrict__ slots, const int32_t *__restrict__ counts, int64_t n,
                        int32_t *__restrict__ oi, int32_t *__restrict__ ot, int32_t *__restrict__ ol,
                        int32_t *__restrict__ err, const unsigned long long *__restrict__ claim, uint32_t epoch) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  StartOutcome o{-1, -1, 0, 0};
  if (!err[i]) {
    const int k = counts ? counts[i] : 1;
    if (claim_lost((const char *)slots, i, sizeof(int32_t), 0, nullptr, claim, epoch)) o.err = MRAFT_ITEM_DUP_SLOT;
    else if (k < 1) o.err = MRAFT_ITEM_BAD_SLOT;
    else o = start_at(s, slots[i], k);
    if (o.err) err[i] = o.err;
  }
  oi[i] = o.index; ot[i] = o.term; ol[i] = o.is_leader;
}

// Start at every group's leader replica (mraft_start_and_tick on the full
// tick's path): slot g * P + leader_peer[g], counts[g] entries (0: none); a
// group whose leader_peer is out of range starts nothing
// (MRAFT_ITEM_BAD_SLOT when it asked for entries with leader_peer >= P).
__global__ void k_start_groups(Dev s, const int32_t *__restrict__ lpeer, StartIO sio) {
  const int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (g >= s.G) return;
  const int lp = lpeer[g], k = sio.counts[g];
  StartOutcome o{-1, -1, 0, 0};
  if (lp >= 0 && lp < s.P) {
    if (k < 0) o.err = MRAFT_ITEM_BAD_SLOT;
    else if (k > 0) o = start_at(s, g * s.P + lp, k);
  } else if (lp >= s.P && k != 0) {
    o.err = MRAFT_ITEM_BAD_SLOT;
  }
  sio.oi[g] = o.index; sio.ot[g] = o.term; sio.ol[g] = o.is_leader; sio.err[g] = o.err;
}

// ---------------------------------------------------------------- applier
__global__ void k_collect_apply(Dev s, int32_t *__restrict__ from, int32_t *__restrict__ to,
                                int32_t *__restrict__ snap_index, int32_t *__restrict__ snap_term) {
  const int64_t gp = (int64_t)s.G * s.P;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < gp;
       i += (int64_t)gridDim.x * blockDim.x) {
    const ApplyMsg m = apply_slot(s, i, snap_index ? s.hsnap[i] : 0, s.applied[i], s.commit[i]);
    if (snap_index) { snap_index[i] = m.snap_index; snap_term[i] = m.snap_term; }
    from[i] = m.from; to[i] = m.to;
  }
}

// Compacted applier: slots with a message to send, ascending, in three
// launches (mraft_device.h "ordered compaction", one list). `snaps`: the
// caller takes SnapshotValid messages (hasSnapshot counts and is cleared);
// without, only commitIndex > lastApplied counts and hasSnapshot is left for
// a later call that takes them (as mraft_collect_apply does).
__global__ __launch_bounds__(kCompactBlock) void k_apply_count(Dev s, int32_t *__restrict__ bcnt, int snaps) {
  const int64_t gp = (int64_t)s.G * s.P;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const bool pend[1] = {i < gp && apply_pending(snaps ? s.hsnap[i] : 0, s.applied[i], s.commit[i])};
  compact_count<1>(pend, bcnt, gridDim.x);
}

// The scan of every compaction: workgroup k scans list k's nb block counts in
// place (exclusive), 1,024 at a time with a carry, and writes the list's
// total (total0 for list 0, total1 for list 1).
__global__ __launch_bounds__(1024) void k_compact_scan(int32_t *__restrict__ bcnt, int64_t nb,
                                                       int64_t *__restrict__ total0, int64_t *__restrict__ total1) {
  __shared__ int64_t part[1024];
  int32_t *c = bcnt + blockIdx.x * nb;
  int64_t carry = 0;
  for (int64_t base = 0; base < nb; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const int64_t v = i < nb ? c[i] : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive Hillis-Steele scan
      const int64_t add = threadIdx.x >= (unsigned)o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < nb) c[i] = (int32_t)(carry + part[threadIdx.x] - v);  // exclusive offset
    const int64_t chunk = part[1023];
    __syncthreads();
    carry += chunk;
  }
  if (threadIdx.x == 0) *(blockIdx.x == 0 ? total0 : total1) = carry;
}

__global__ __launch_bounds__(kCompactBlock) void k_apply_emit(
    Dev s, const int32_t *__restrict__ boff, int64_t cap, int32_t *__restrict__ oslot, int32_t *__restrict__ osi,
    int32_t *__restrict__ ost, int32_t *__restrict__ ofrom, int32_t *__restrict__ oto) {
  const int64_t gp = (int64_t)s.G * s.P;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int la = 0, ci = 0, hs = 0;
  if (i < gp) { la = s.applied[i]; ci = s.commit[i]; hs = osi ? s.hsnap[i] : 0; }
  const bool pend[1] = {i < gp && apply_pending(hs, la, ci)};
  int64_t off[1];
  compact_offsets<1>(pend, boff, gridDim.x, off);
  if (pend[0] && off[0] < cap) {
    const ApplyMsg m = apply_slot(s, i, hs, la, ci);
    oslot[off[0]] = (int32_t)i;
    if (osi) { osi[off[0]] = m.snap_index; ost[off[0]] = m.snap_term; }
    ofrom[off[0]] = m.from; oto[off[0]] = m.to;
  }
}

// ---------------------------------------------------------------- snapshots
// Snapshot (raft_snapshot.go:3-13), thread per item: setLogs(sliceFrom(index))
// (:10, raft_log.go:18-21, 75-77) is an O(1) rebase of the ring — the head
// moves to the entry at `index`, which becomes the dummy with its own term;
// no term moves.
__global__ __launch_bounds__(256) void k_snapshot(Dev s, const int32_t *__restrict__ slots,
                                                  const int32_t *__restrict__ index, int64_t n,
                                                  int32_t *__restrict__ err) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n || err[i]) return;
  const int sl = slots[i], x = index[i];
  const int d = s.dummy[sl], last = s.last[sl];
  if (x <= d) return;                                                  // :6-9
  if (x > last) {                                                      // sliceFrom panics
    err[i] = MRAFT_ITEM_PREV_BEYOND_LAST;
    return;
  }
  s.head[sl] = ring(s.head[sl] + (x - d), s.L);                        // :10
  s.dummy[sl] = x;
  mark_persist(s, sl, MRAFT_PERSIST_STATE | MRAFT_PERSIST_SNAPSHOT);    // :12
}

// appendOneRound's snapshot branch (raft_append_entry.go:27-34).
__global__ void k_gather_is(Dev s, const int32_t *__restrict__ slots, const int32_t *__restrict__ peers,
                            int64_t n, mraft_is_args *__restrict__ out, int32_t *__restrict__ err) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int P = s.P;
  const int64_t gp = (int64_t)s.G * P;
  mraft_is_args a = {-1, 0, 0, 0, 0};
  int e = 0;
  const int slot = slots[i], peer = peers[i];
  if (slot < 0 || slot >= gp || peer < 0 || peer >= P || peer == slot % P) {
    e = MRAFT_ITEM_BAD_SLOT;
  } else if (s.role[slot] != kLeader) {
    e = MRAFT_ITEM_BAD_STATE;
  } else if (s.next[(int64_t)slot * P + peer] - 1 < s.dummy[slot]) {
    a.slot = (slot / P) * P + peer;
    a.term = s.term[slot];                                             // :29
    a.leader_id = slot % P;                                            // :30
    a.last_included_index = s.dummy[slot];                             // :31
    a.last_included_term = s.log[(int64_t)slot * s.L + s.head[slot]];  // :32 dummyTerm
  }
  out[i] = a;
  err[i] = e;
}

// HandleInstallSnapshot (raft_snapshot.go:15-54), thread per item. Installing
// by sliceFrom(LastIncludedIndex) (:38-40) is an O(1) ring rebase.
__global__ __launch_bounds__(256) void k_handle_is(Dev s, const mraft_is_args *__restrict__ args, int64_t n,
                                                   mraft_is_reply *__restrict__ rep, int32_t *__restrict__ flags,
                                                   int32_t *__restrict__ err) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  // every exit: the reply's term, the flags and, for an item refused here, its error
  auto out = [&](int term, int fl, int e = 0) { rep[i] = mraft_is_reply{term, 0}; flags[i] = fl; if (e) err[i] = e; };
  if (err[i]) return out(0, 0);
  const mraft_is_args a = args[i];
  if (!index_in_domain(a.last_included_index)) return out(0, 0, MRAFT_ITEM_BAD_SLOT);  // malformed
  const int f = a.slot, fterm = s.term[f];
  if (a.term < fterm) return out(fterm, 0);                            // :20-22
  const int lii = a.last_included_index;
  const int fcommit = s.commit[f];
  const bool install = lii > fcommit;                                  // :31-33
  const int fd = s.dummy[f], flast = s.last[f], fh = s.head[f];
  if (install && lii <= flast && lii < fd) return out(0, 0, MRAFT_ITEM_BELOW_DUMMY);  // sliceFrom panics
  int fl = 0;
  if (a.term > fterm) { s.term[f] = a.term; s.voted[f] = -1; }         // :23-26
  s.role[f] = kFollower;                                               // :28
  if (install) {
    // :35-37 a new log [dummy] keeps its head; :38-40 sliceFrom moves it
    const int nh = lii > flast ? fh : ring(fh + (lii - fd), s.L);
    s.log[(int64_t)f * s.L + nh] = a.last_included_term;               // :44-45
    if (lii > flast) { s.last[f] = lii; s.srt[f] = 1; }                // [dummy] only
    else s.head[f] = nh;                                               // a suffix: terms_sorted unchanged
    s.hsnap[f] = 1;                                                    // :52 hasSnapshot
    s.dummy[f] = lii;
    s.commit[f] = lii;                                                 // :42
    s.applied[f] = lii;                                                // :43
    fl = MRAFT_F_SNAPSHOT_INSTALLED;
  }
  mark_persist(s, f, (a.term > fterm ? MRAFT_PERSIST_STATE : 0) |     // :26
                         (install ? MRAFT_PERSIST_STATE | MRAFT_PERSIST_SNAPSHOT : 0));  // :47
  out(a.term, fl);                                                     // deferred reply.Term
}

// processInstallSnapshotReply (raft_snapshot.go:56-69): lane per segment.
__global__ void k_process_is(Dev s, const mraft_is_result *__restrict__ items, const int64_t *__restrict__ seg_begin,
                             int64_t n_seg, const int32_t *__restrict__ seg_err, int32_t *__restrict__ flags,
                             int32_t *__restrict__ item_err) {
  const int64_t sg = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (sg >= n_seg) return;
  int64_t b, e;
  if (!segment_bounds(seg_begin, sg, b, e)) return;
  const int P = s.P;
  const int bad = segment_verdict(items, b, e, P, seg_err[sg], [](const mraft_is_result &it) {
    return index_in_domain(it.args_last_included_index);
  });
  if (bad) {
    segment_reject(b, e, bad, flags, item_err);
    return;
  }
  const int slot = items[b].slot;
  int term = s.term[slot], role = s.role[slot];
  const int t0 = term;
  for (int64_t i = b; i < e; ++i) {
    const mraft_is_result it = items[i];
    int fl = 0;
    if (it.reply_term > term) {                                        // :59-64
      term = it.reply_term;
      role = kFollower;
      fl = MRAFT_F_STEPPED_DOWN;
    } else if (role == kLeader && it.args_term == term) {              // :65-68
      s.match[(int64_t)slot * P + it.peer] = it.args_last_included_index;
      s.next[(int64_t)slot * P + it.peer] = it.args_last_included_index + 1;
      fl = MRAFT_F_APPLIED;
    }
    flags[i] = fl;
    item_err[i] = 0;
  }
  if (term != t0) {
    s.term[slot] = term; s.role[slot] = role; s.voted[slot] = -1;
    mark_persist(s, slot, MRAFT_PERSIST_STATE);                        // :64
  }
}

// ---------------------------------------------------------------- a6 part 1
__global__ void k_start_election(Dev s, const int32_t *__restrict__ slots, int64_t n,
                                 mraft_rv_args *__restrict__ out, int32_t *__restrict__ err) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  mraft_rv_args a = {};
  if (!err[i]) {
    const int sl = slots[i];
    const int t = s.term[sl] + 1;                                      // raft_election.go:7
    const int last = s.last[sl];
    s.role[sl] = kCandidate;                                           // :6
    s.term[sl] = t;
    s.voted[sl] = sl % s.P;                                            // :14
    s.votes[sl] = 1;                                                   // :17
    mark_persist(s, sl, MRAFT_PERSIST_STATE);                          // :15
    a.slot = sl;
    a.term = t;
    a.candidate_id = sl % s.P;
    a.last_log_index = last;                                           // :12
    a.last_log_term = term_at(s, sl, s.dummy[sl], s.head[sl], last);  // :13
  }
  out[i] = a;
}

// ---------------------------------------------------------------- a5
__global__ void k_handle_rv(Dev s, const mraft_rv_args *__restrict__ args, int64_t n,
                            mraft_rv_reply *__restrict__ rep, int32_t *__restrict__ err) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  mraft_rv_reply r = {0, 0};
  if (!err[i]) {
    const mraft_rv_args a = args[i];
    const int v = a.slot;
    int term = s.term[v], voted = s.voted[v], role = s.role[v];
    const int t0 = term, v0 = voted, r0 = role;
    mark_persist(s, v, MRAFT_PERSIST_STATE);                           // deferred :57
    if (a.term < term) {                                               // raft_election.go:59-62
      r.term = term;
    } else {
      if (a.term > term) { role = kFollower; term = a.term; voted = -1; }  // :63-66
      r.term = term;                                                   // :67
      const int mylast = s.last[v];
      const int mylt = term_at(s, v, s.dummy[v], s.head[v], mylast);
      const bool up = a.last_log_term > mylt ||                        // raft_log.go:99-104
                      (mylt == a.last_log_term && a.last_log_index >= mylast);
      if ((voted == -1 || voted == a.candidate_id) && up) {            // :69-74
        voted = a.candidate_id;
        r.vote_granted = 1;
      }
      if (term != t0) s.term[v] = term;
      if (voted != v0) s.voted[v] = voted;
      if (role != r0) s.role[v] = role;
    }
  }
  rep[i] = r;
}

// ---------------------------------------------------------------- a6 part 2
__global__ void k_tally(Dev s, const mraft_rv_result *__restrict__ items, const int64_t *__restrict__ seg_begin,
                        int64_t n_seg, const int32_t *__restrict__ seg_err, int32_t *__restrict__ flags,
                        int32_t *__restrict__ item_err) {
  const int64_t sg = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (sg >= n_seg) return;
  int64_t b, e;
  if (!segment_bounds(seg_begin, sg, b, e)) return;
  const int P = s.P;
  const int bad = segment_verdict(items, b, e, P, seg_err[sg], [](const mraft_rv_result &) { return true; });
  if (bad) {
    segment_reject(b, e, bad, flags, item_err);
    return;
  }
  const int c = items[b].slot;
  int term = s.term[c], role = s.role[c], votes = s.votes[c], voted = s.voted[c];
  const int t0 = term, r0 = role, vs0 = votes, vd0 = voted;
  bool lead = false, stepped = false;
  for (int64_t i = b; i < e; ++i) {
    const mraft_rv_result it = items[i];
    int fl = 0;
    if (term == it.args_term && role == kCandidate) {                  // raft_election.go:29
      if (it.vote_granted) {                                           // :30
        votes += 1;                                                    // :31
        if (votes > P / 2) {                                           // :32
          role = kLeader;                                              // :33
          lead = true;
          fl |= MRAFT_F_BECAME_LEADER;
        }
      } else if (it.reply_term > term) {                               // :42-45
        role = kFollower; term = it.reply_term; voted = -1;
        fl |= MRAFT_F_STEPPED_DOWN;
        stepped = true;
      }
    }
    flags[i] = fl;
    item_err[i] = 0;
  }
  if (term != t0) s.term[c] = term;
  if (role != r0) s.role[c] = role;
  if (votes != vs0) s.votes[c] = votes;
  if (voted != vd0) s.voted[c] = voted;
  if (stepped) mark_persist(s, c, MRAFT_PERSIST_STATE);                // :45
  if (lead) {                                                          // :34-38
    const int nx = s.last[c] + 1;
    for (int j = 0; j < P; ++j) { s.match[(int64_t)c * P + j] = 0; s.next[(int64_t)c * P + j] = nx; }
  }
}

// ---------------------------------------------------------------- persistence
// persist_dirty read-out (copy + clear): the slots the host must save.
__global__ void k_collect_persist(Dev s, int32_t *__restrict__ out) {
  const int64_t gp = (int64_t)s.G * s.P;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < gp;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int v = s.pdirty[i];
    out[i] = v;
    if (v) s.pdirty[i] = 0;
  }
}

// SaveState (raft.go:209-216), scalar part: lane per slot.
__global__ void k_read_persistent_hdr(Dev s, const int32_t *__restrict__ slots, int64_t n,
                                      mraft_persistent *__restrict__ out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int sl = slots[i];
  mraft_persistent r = {};
  r.slot = sl;
  r.current_term = s.term[sl];
  r.voted_for = s.voted[sl];
  r.dummy_index = s.dummy[sl];
  r.last_index = s.last[sl];
  out[i] = r;
}

// SaveState, log part: wave per slot streams terms[0 .. last-dummy] of its row.
__global__ __launch_bounds__(256) void k_read_persistent_terms(Dev s,
                                                               const mraft_persistent *__restrict__ hdr,
                                                               int64_t n, int32_t *__restrict__ out) {
  const int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (i >= n) return;
  const mraft_persistent r = hdr[i];
  wave_copy_from_ring(s.log + (int64_t)r.slot * s.L, r.dummy_index, s.head[r.slot], s.L, r.dummy_index,
                      out + r.terms_offset, r.last_index - r.dummy_index + 1);
}

// Make (raft.go:51-87) + readPersist (:217-235): wave per (validated) item.
__global__ __launch_bounds__(256) void k_restore(Dev s, const mraft_persistent *__restrict__ in,
                                                 int64_t n, const int32_t *__restrict__ terms,
                                                 const int32_t *__restrict__ err) {
  const int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (i >= n || err[i]) return;
  const mraft_persistent r = in[i];
  const int64_t sl = r.slot;
  wave_copy(terms + r.terms_offset, s.log + sl * s.L, r.last_index - r.dummy_index + 1);  // :233
  const bool srt = wave_terms_sorted(terms + r.terms_offset, 0, 0, INT32_MAX, 1, r.last_index - r.dummy_index);
  if (lane_id() == 0) {
    s.srt[sl] = srt ? 1 : 0;
    s.term[sl] = r.current_term;                                       // :231
    s.voted[sl] = r.voted_for;                                         // :232
    s.role[sl] = kFollower;                                            // :58
    s.dummy[sl] = r.dummy_index;
    s.head[sl] = 0;                                                    // a fresh raftLog
    s.hsnap[sl] = 0;                                                   // Make: no snapshot pending
    s.last[sl] = r.last_index;
    s.commit[sl] = r.dummy_index;                                      // :79
    s.applied[sl] = r.dummy_index;                                     // :80
    s.votes[sl] = 0;
    if (s.pdirty) s.pdirty[sl] = 0;
  }
  for (int j = lane_id(); j < s.P; j += 64) {                          // :64-65 make([]int, P)
    s.match[sl * s.P + j] = 0;
    s.next[sl * s.P + j] = 0;
  }
}

// crash1 (config.go:113) + Make + readPersist in place (mraft_crash): wave per
// item. The persistent fields are live in HBM already (the reference persists
// before every handler returns), so the Make half of k_restore is all there is:
// no log word moves, the ring keeps its head. ed / hd: the timer arrays, or
// null without timers (a down replica's deadlines are never due).
__global__ __launch_bounds__(256) void k_crash(Dev s, const int32_t *__restrict__ slots, int64_t n,
                                               int32_t *__restrict__ err, int32_t *__restrict__ ed,
                                               int32_t *__restrict__ hd) {
  const int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  if (i >= n) return;
  const int64_t sl = slots[i];
  int e = MRAFT_ITEM_OK, d = 0, last = 0;
  if (sl < 0 || sl >= (int64_t)s.G * s.P) {
    e = MRAFT_ITEM_BAD_SLOT;
  } else {
    d = s.dummy[sl]; last = s.last[sl];
    if ((int64_t)last - d < 0 || (int64_t)last - d >= s.L) e = MRAFT_ITEM_BAD_STATE;
  }
  if (err && lane_id() == 0) err[i] = e;
  if (e) return;
  // the proof is taken as it stands; without one, from the ring (a head outside
  // the ring proves nothing). Repeated slots write the same words.
  if (!s.srt[sl]) {
    const int h = s.head[sl];
    if (h >= 0 && h < s.L && wave_terms_sorted(s.log + sl * s.L, d, h, s.L, d + 1, last) && lane_id() == 0)
      s.srt[sl] = 1;
  }
  if (lane_id() == 0) {
    s.role[sl] = kFollower;                                            // raft.go:58
    s.commit[sl] = d;                                                  // :79
    s.applied[sl] = d;                                                 // :80
    s.votes[sl] = 0;
    s.hsnap[sl] = 0;                                                   // Make: no snapshot pending
    if (s.pdirty) s.pdirty[sl] = 0;
    if (ed) { ed[sl] = MRAFT_TIMER_NEVER; hd[sl] = MRAFT_TIMER_NEVER; }
  }
  for (int j = lane_id(); j < 2 * s.P; j += 64)                        // :64-65 make([]int, P)
    (j < s.P ? s.match[sl * s.P + j] : s.next[sl * s.P + j - s.P]) = 0;
}

// terms_sorted of every replica from its log (mraft_load_state): wave per slot.
__global__ __launch_bounds__(256) void k_terms_sorted(Dev s) {
  const int64_t gp = (int64_t)s.G * s.P;
  for (int64_t sl = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; sl < gp;
       sl += ((int64_t)gridDim.x * blockDim.x) >> 6) {
    const int d = s.dummy[sl], last = s.last[sl], h = s.head[sl];
    const bool ok = last - d < s.L && wave_terms_sorted(s.log + sl * s.L, d, h, s.L, d + 1, last);
    if (lane_id() == 0) s.srt[sl] = ok ? 1 : 0;
  }
}

// ---------------------------------------------------------------- GetState
__global__ void k_export(Dev s, const int32_t *__restrict__ lpeer, int32_t *__restrict__ commit,
                         int32_t *__restrict__ term_leader) {
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g >= s.G) return;
  int p = lpeer ? lpeer[g] : 0;
  if (p < 0 || p >= s.P) p = 0;
  const int64_t sl = (int64_t)g * s.P + p;
  commit[g] = s.commit[sl];
  term_leader[g] = term_leader_word(s.term[sl], s.role[sl]);
}

// Launchers. A thread per item in workgroups of B threads; nothing to do without items.
template <int B = kBlock, class K, class... A>
void launch_items(K k, int64_t n, hipStream_t st, A... a) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k, dim3(blocks_for(n, B)), dim3(B), 0, st, a...);
}

}  // namespace

void launch_terms_sorted(const Dev &s, hipStream_t st) {
  const int64_t gp = (int64_t)s.G * s.P;
  hipLaunchKernelGGL(k_terms_sorted, dim3(strided_grid(gp * 64, 65536)), dim3(kBlock), 0, st, s);
}

void launch_init_state(const Dev &s, hipStream_t st) {
  hipLaunchKernelGGL(k_init_state, dim3(strided_grid((int64_t)s.G * s.P)), dim3(kBlock), 0, st, s);
}

void launch_claim(const void *items, int64_t n, int stride, int slot_off, const int64_t *seg_begin, int64_t gp,
                  unsigned long long *claim, uint32_t epoch, int32_t *err, hipStream_t st) {
  launch_items(k_claim, n, st, (const char *)items, n, stride, slot_off, seg_begin, gp, claim, epoch, err);
  launch_items(k_claim_check, n, st, (const char *)items, n, stride, slot_off, seg_begin, claim, epoch, err);
}

void launch_gather_args(const Dev &s, const int32_t *slots, const int32_t *peers, int64_t n, mraft_ae_args *out,
                        int32_t *err, hipStream_t st) {
  launch_items<kMsgBlock>(k_gather_args, n, st, s, slots, peers, n, out, err);
}

void launch_start(const Dev &s, const int32_t *slots, const int32_t *counts, int64_t n, int32_t *oi, int32_t *ot,
                  int32_t *ol, int32_t *err, unsigned long long *claim, uint32_t epoch, hipStream_t st) {
  launch_items(k_claim, n, st, (const char *)slots, n, (int)sizeof(int32_t), 0, (const int64_t *)nullptr,
               (int64_t)s.G * s.P, claim, epoch, err);
  launch_items(k_start, n, st, s, slots, counts, n, oi, ot, ol, err, claim, epoch);
}

void launch_start_groups(const Dev &s, const int32_t *lpeer, const StartIO &sio, hipStream_t st) {
  launch_items(k_start_groups, s.G, st, s, lpeer, sio);
}

void launch_collect_apply(const Dev &s, int32_t *from, int32_t *to, int32_t *snap_index, int32_t *snap_term,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_collect_apply, dim3(strided_grid((int64_t)s.G * s.P)), dim3(kBlock), 0, st, s, from, to,
                     snap_index, snap_term);
}

void launch_compact_scan(int32_t *bcnt, int64_t nb, int lists, int64_t *total0, int64_t *total1, hipStream_t st) {
  hipLaunchKernelGGL(k_compact_scan, dim3(lists), dim3(1024), 0, st, bcnt, nb, total0, total1);
}

void launch_collect_apply_compact(const Dev &s, int32_t *scratch_bcnt, int64_t cap, int32_t *oslot,
                                  int32_t *osnap_index, int32_t *osnap_term, int32_t *ofrom, int32_t *oto,
                                  int64_t *total, hipStream_t st) {
  const int64_t nb = compact_blocks((int64_t)s.G * s.P);
  hipLaunchKernelGGL(k_apply_count, dim3((unsigned)nb), dim3(kCompactBlock), 0, st, s, scratch_bcnt,
                     osnap_index ? 1 : 0);
  launch_compact_scan(scratch_bcnt, nb, 1, total, nullptr, st);
  hipLaunchKernelGGL(k_apply_emit, dim3((unsigned)nb), dim3(kCompactBlock), 0, st, s, scratch_bcnt, cap, oslot,
                     osnap_index, osnap_term, ofrom, oto);
}

void launch_snapshot(const Dev &s, const int32_t *slots, const int32_t *index, int64_t n, int32_t *err,
                     hipStream_t st) {
  launch_items(k_snapshot, n, st, s, slots, index, n, err);
}

void launch_gather_is(const Dev &s, const int32_t *slots, const int32_t *peers, int64_t n, mraft_is_args *out,
                      int32_t *err, hipStream_t st) {
  launch_items(k_gather_is, n, st, s, slots, peers, n, out, err);
}

void launch_handle_is(const Dev &s, const mraft_is_args *args, int64_t n, mraft_is_reply *rep, int32_t *flags,
                      int32_t *err, hipStream_t st) {
  launch_items(k_handle_is, n, st, s, args, n, rep, flags, err);
}

void launch_process_is(const Dev &s, const mraft_is_result *items, const int64_t *seg_begin, int64_t n_seg,
                       int32_t *seg_err, int32_t *flags, int32_t *item_err, hipStream_t st) {
  launch_items<64>(k_process_is, n_seg, st, s, items, seg_begin, n_seg, seg_err, flags, item_err);
}

void launch_start_election(const Dev &s, const int32_t *slots, int64_t n, mraft_rv_args *out, int32_t *err,
                           hipStream_t st) {
  launch_items(k_start_election, n, st, s, slots, n, out, err);
}

void launch_handle_rv(const Dev &s, const mraft_rv_args *args, int64_t n, mraft_rv_reply *rep, int32_t *err,
                      hipStream_t st) {
  launch_items(k_handle_rv, n, st, s, args, n, rep, err);
}

void launch_tally(const Dev &s, const mraft_rv_result *items, const int64_t *seg_begin, int64_t n_seg,
                  int32_t *seg_err, int32_t *flags, int32_t *item_err, hipStream_t st) {
  launch_items<64>(k_tally, n_seg, st, s, items, seg_begin, n_seg, seg_err, flags, item_err);
}

void launch_collect_persist(const Dev &s, int32_t *out, hipStream_t st) {
  hipLaunchKernelGGL(k_collect_persist, dim3(strided_grid((int64_t)s.G * s.P)), dim3(kBlock), 0, st, s, out);
}

void launch_read_persistent_hdr(const Dev &s, const int32_t *slots, int64_t n, mraft_persistent *out, hipStream_t st) {
  launch_items(k_read_persistent_hdr, n, st, s, slots, n, out);
}

// (a wave per item: 64 threads each)
void launch_read_persistent_terms(const Dev &s, const mraft_persistent *hdr, int64_t n, int32_t *out, hipStream_t st) {
  launch_items(k_read_persistent_terms, n * 64, st, s, hdr, n, out);
}

void launch_restore(const Dev &s, const mraft_persistent *in, int64_t n, const int32_t *terms, const int32_t *err,
                    hipStream_t st) {
  launch_items(k_restore, n * 64, st, s, in, n, terms, err);
}

void launch_crash(const Dev &s, const int32_t *slots, int64_t n, int32_t *err, int32_t *ed, int32_t *hd,
                  hipStream_t st) {
  launch_items(k_crash, n * 64, st, s, slots, n, err, ed, hd);
}

void launch_export(const Dev &s, const int32_t *lpeer, int32_t *commit, int32_t *term_leader, hipStream_t st) {
  launch_items(k_export, s.G, st, s, lpeer, commit, term_leader);
}

}  // namespace mraft
