// mraft_fold.hip — the message-level AppendEntries reply fold ("a2 + a1",
// mraft_process_append_replies of include/mraft.h) for gfx950: the segment
// claims with the zeroed outputs (k_claim_zero), the fold of eight reply
// segments per wave (k_fold), and the long segments and open a1 scans
// (k_fold_tail).
#include "mraft_device.h"
#include "mraft_internal.h"
#include "mraft_rules.h"

namespace mraft {

namespace {

// A pointer the wave holds in SGPRs where it is used (a per-lane address
// hoisted out of a loop as a VGPR pair is what the register allocator spills).
template <class T>
__device__ __forceinline__ T *uni_ptr(T *p) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (T *)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

// The reply fold's claim (mraft_process_append_replies): k_claim over the
// segments, and the zeroing of the per-item outputs (items no segment covers
// keep flag 0, error 0) in the same launch; the duplicate check happens in
// k_fold itself (claim[slot] loads with the replica's state).
__global__ void k_claim_zero(const char *__restrict__ items, int64_t n, int stride, int slot_off,
                             const int64_t *__restrict__ seg_begin, int64_t gp,
                             unsigned long long *__restrict__ claim, uint32_t epoch,
                             int32_t *__restrict__ err, int64_t nz, int32_t *__restrict__ z0,
                             int32_t *__restrict__ z1, unsigned *__restrict__ zc, unsigned *__restrict__ zl) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < nz) {
    z0[i] = 0;
    z1[i] = 0;
  }
  if (i == 0 && zc) *zc = 0;  // no a1 range pending for k_fold_tail's scans yet
  if (i == 0 && zl) *zl = 0;  // no long segment for k_fold_tail yet
  if (i < n) claim_item(items, i, stride, slot_off, seg_begin, gp, claim, epoch, err);
}

// ---------------------------------------------------------------- a2 + a1
#ifndef MRAFT_FOLD_GRID
#define MRAFT_FOLD_GRID (1 << 30)  // workgroups of the reply fold (segments beyond: grid-stride)
#endif
// Grids of the launches enqueued blind (their work is counted on the device
// and is usually small: deferred items need two leaders of one group in a
// batch, long segments more replies than a lane group, a1 scans a range the
// top-term probe did not settle). Small grids: a launch that must find free
// wave slots beside another pipeline's handler finds them at once — two
// pipelines 0.366-0.369 -> 0.358 ms per step, three 0.363-0.365 -> 0.354
// (profiles/r5_g1; 512 / 256 / 2,048 workgroups before).
#ifndef MRAFT_FOLD_TAIL_NL
#define MRAFT_FOLD_TAIL_NL 16  // k_fold_tail workgroups for the long segments (grid-stride)
#endif
#ifndef MRAFT_FOLD_TAIL_NS
#define MRAFT_FOLD_TAIL_NS 256 // k_fold_tail workgroups for the pending a1 scans (grid-stride)
#endif
// The fold's shape (r3-r5 A/B runs, profiles/INDEX.md): eight reply segments
// per wave, 8 lanes each (four per wave measured 10 % slower; one per wave
// slower still), waves of one XCD on a contiguous segment range (r4_v18: fold
// call -8 %, reads 55 -> 46 MB); each segment's a1 ranges probed by their top
// word in k_fold and the open ones scanned in a second launch, k_fold_tail,
// which also folds the segments longer than a lane group on all 64 lanes
// (r4_v21: -4 % against separate launches; the scans back inside k_fold,
// r5_f1: no difference). Earlier variants live in git history.
constexpr int kFoldGroups = 8;              // reply segments per k_fold wave
constexpr int kFoldScanU = 4;               // long-segment a1 scan: dword loads per lane in flight (64·U terms)
constexpr int kFscanU = 8;                  // k_fold_tail scans: dword loads per lane in flight (4: +7 %)
constexpr int kFscanW = 4;                  // pending a1 ranges per k_fold_tail scan wave

// Appends the lanes' pending a1 ranges (pred) to k_fold_tail's compact list:
// one atomic per wave on the list's counter. Record: {lo, hi, slot,
// currentTerm}, {dummy, ring head, reply index, 0}. Wave-uniform call.
__device__ __forceinline__ void push_pending(int4 *__restrict__ pend, unsigned *__restrict__ pcount, bool pred,
                                             int4 ra, int4 rb) {
  const unsigned long long m = __ballot(pred);
  if (!m) return;
  const int l0 = first_lane(m);
  unsigned base = 0;
  if (lane_id() == l0) base = atomicAdd(pcount, (unsigned)__popcll(m));
  base = (unsigned)__shfl((int)base, l0, 64);
  if (pred) {
    const unsigned k = base + (unsigned)__popcll(m & ((1ull << lane_id()) - 1));
    pend[2 * (int64_t)k] = ra;
    pend[2 * (int64_t)k + 1] = rb;
  }
}

// Lane groups of GW lanes (the wave as 64 / GW groups; GW = 64: the wave).
template <int GW>
__device__ __forceinline__ int gw_base() { return (int)(lane_id() & ~(unsigned)(GW - 1)); }
template <int GW>
__device__ __forceinline__ auto gw_mask(bool pred) {  // this lane's group's ballot, bit k = its lane k
  if constexpr (GW == 64) return __ballot(pred);
  else return (unsigned)((__ballot(pred) >> gw_base<GW>()) & ((1ull << GW) - 1));
}
template <int GW>
__device__ __forceinline__ int gw_bcast(int v, int k) { return __shfl(v, gw_base<GW>() + k, 64); }
__device__ __forceinline__ int last_lane(unsigned m) { return 31 - __clz((int)m); }
__device__ __forceinline__ int last_lane(unsigned long long m) { return 63 - __builtin_clzll(m); }

// ---------------------------------------------------------------- the fold's rules
// processAppendEntriesReply + advanceCommitIndexForLeader
// (raft_append_entry.go:66-105) on one reply segment, each rule stated once
// for the fold's two paths (fold_segment, one segment per wave; fold_groupw,
// one per lane group). The lanes that share a segment hold its running values
// alike; "this lane's" values belong to the reply the lane owns.

// The item segment sg begins at (segment sg - 1 ends before it); without
// seg_begin every item is a segment of its own. segment_bounds (mraft_rules.h)
// by value, for the group path.
__device__ __forceinline__ int64_t segment_edge(const int64_t *__restrict__ seg_begin, int64_t sg) {
  return seg_begin ? seg_begin[sg] : sg;
}

// Whether segment sg owns the slot whose claim word is (cw_hi, cw_lo): items
// addressed to one replica slot in several segments, the lowest segment wins
// (k_claim_zero's atomicMax on the inverted index), the others are rejected
// before any state change. The same truth as claim_won(word, epoch, sg); on
// the halves, because the long path holds the low half wave-uniform and the
// high half is the epoch itself: two 32-bit compares, no 64-bit tag formed.
__device__ __forceinline__ bool claim_owned(uint32_t cw_lo, uint32_t cw_hi, uint32_t epoch, int64_t sg) {
  return cw_lo == (uint32_t)claim_tag(epoch, sg) && cw_hi == epoch;
}

// A reply that makes its segment malformed: another slot than the segment's,
// a peer outside the group or the replica itself, or a record outside the
// Index domain (include/mraft.h; the oracle's reply_index_ok): the
// acknowledged entries end at prevLogIndex + n <= 2^31 - 2 with n >= 0, so
// matchIndex and nextIndex stay int32.
template <int P>
__device__ __forceinline__ bool reply_malformed(const mraft_ae_result &r, int slot, int me) {
  return r.slot != slot || r.peer < 0 || r.peer >= P || r.peer == me || r.args_n_entries < 0 ||
         !index_in_domain((int64_t)r.args_prev_log_index + r.args_n_entries);
}

// The verdict on a segment before any state changes, in the order of
// include/mraft.h: the claim's error or a slot another segment owns (bad, on
// entry: the claim decides first), then a malformed reply, then a replica
// whose commitIndex lies below its dummy.
__device__ __forceinline__ int fold_verdict(int bad, bool malformed, int commit, int dummy) {
  if (bad) return bad;
  if (malformed) return MRAFT_ITEM_BAD_SLOT;
  return commit < dummy ? MRAFT_ITEM_BAD_STATE : 0;
}

// A reply's fields as the reply step reads them, r(&mraft_ae_result::field),
// each path in its own fetch order. LaneReply: reply k of the long path's
// batch sits in lane k, and a field is read there when the step needs it
// (success, the entry count and the conflict index only inside their branch).
// HeldReply: the group path has broadcast the whole record up front.
using ReplyField = int32_t mraft_ae_result::*;
struct LaneReply {
  const mraft_ae_result &it;
  int k;
  __device__ __forceinline__ int operator()(ReplyField f) const { return __builtin_amdgcn_readlane(it.*f, k); }
};
struct HeldReply {
  mraft_ae_result v;
  __device__ __forceinline__ int operator()(ReplyField f) const { return v.*f; }
};

// The reply step (:67-88) on the segment's running values; returns the
// reply's flags. a1 (:89-105) is evaluated after each successful reply exactly
// as :78 calls it, but its log reads are deferred: the fold never reads
// commitIndex, and while the replica stays leader its term is the segment's
// initial term, so every evaluation is "the highest index in (H, top] whose
// term is currentTerm", with H the largest top evaluated so far (an
// evaluation that scanned (commit, top] leaves no entry of that term above
// the new commit up to top). The lane that owns reply k (ln == k, ln the
// lane's position in its segment) keeps the range as (plo, phi); a segment's
// ranges are disjoint and ascending. (ln and k apart, not the bool ln == k:
// as a lane mask held across the step it costs both kernels scalar registers.)
template <int P, class Reply>
__device__ __forceinline__ int reply_step(const Reply &r, int ln, int k, int &term, int &role, int (&m)[8],
                                          int (&nx)[8], int &H, int last, int me, bool &touched_mn, int &plo,
                                          int &phi) {
  using R = mraft_ae_result;
  const int pr = r(&R::peer), rt = r(&R::reply_term), at = r(&R::args_term), ap = r(&R::args_prev_log_index);
  int fl = 0, nxp = 0;
#pragma unroll
  for (int j = 0; j < P; ++j) if (j == pr) nxp = nx[j];
  if (rt > term) {                                                       // :67-72
    term = rt; role = kFollower;
    fl |= MRAFT_F_STEPPED_DOWN;
  } else if (rt == term && role == kLeader && at == term && ap == nxp - 1) {  // :73-74
    fl |= MRAFT_F_APPLIED;
    touched_mn = true;
    if (r(&R::reply_success)) {
      const int mv = r(&R::args_n_entries) + ap;                         // :76
      nxp = mv + 1;                                                      // :77
#pragma unroll
      for (int j = 0; j < P; ++j) if (j == pr) m[j] = mv;
      const int top = min(quorum<P>(m, me), last);                       // a1, :78
      if (top > H) {
        if (ln == k) { plo = H + 1; phi = top; }
        H = top;
      }
    } else {
      nxp = r(&R::reply_conflict_index);                                 // :82
    }
#pragma unroll
    for (int j = 0; j < P; ++j) if (j == pr) nx[j] = nxp;
    if (nxp < last + 1) fl |= MRAFT_F_NEED_MORE;                         // :84-86
  }
  return fl;
}

// The top-word probe of this lane's a1 range (has: it holds one): on a log
// whose last entries carry the current term every range ends at its top.
// Returns phi when the top term is t0 (:98), else -1, and whether the range
// stays open for a scan of [plo, phi - 1]. With sorted terms (include/mraft.h
// MRAFT_TERMS_SORTED) a top term below currentTerm settles the range: no lower
// entry carries currentTerm.
__device__ __forceinline__ int a1_probe(bool has, const int32_t *__restrict__ lrow, int dummy, int head, int L,
                                        int plo, int phi, int t0, int srt, bool &open) {
  int x = -1;
  bool settled = false;
  if (has) {
    const int pv = lrow[ring(phi - dummy + head, L)];
    if (pv == t0) x = phi;
    else settled = srt && pv < t0;
  }
  open = has && plo < phi && x < 0 && !settled;
  return x;
}

// :99-100 for the ranges whose index x the probes (and the long path's scans)
// found: MRAFT_F_COMMITTED on the lane's reply, and commitIndex from the
// latest range of the GW-lane group that found one.
template <int GW>
__device__ __forceinline__ void a1_commit(int x, int &myfl, int &commit) {
  if (x >= 0) myfl |= MRAFT_F_COMMITTED;
  const auto fm = gw_mask<GW>(x >= 0);
  if (fm) commit = __shfl(x, gw_base<GW>() + last_lane(fm), 64);
}

// The segment's write-back: term, role, votedFor and the persist mark (:72)
// and commitIndex by the segment's first lane, the match / next rows by its
// peer lanes (pl: the lane's position among them).
template <int P>
__device__ __forceinline__ void fold_write_back(const Dev &s, int slot, int64_t mrow, bool first, bool peer_lane,
                                                int pl, int term, int role, int commit, int t0, int r0, int c0,
                                                bool touched_mn, const int (&m)[8], const int (&nx)[8]) {
  if (first && (term != t0 || role != r0)) {
    s.term[slot] = term; s.role[slot] = role; s.voted[slot] = -1;
    mark_persist(s, slot, MRAFT_PERSIST_STATE);                          // :72
  }
  if (first && commit != c0) s.commit[slot] = commit;
  if (touched_mn) {
    int om = 0, on = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) if (pl == j) { om = m[j]; on = nx[j]; }
    if (peer_lane) { s.match[mrow + pl] = om; s.next[mrow + pl] = on; }
  }
}

// a1's scans of the reply fold (raft_append_entry.go:89-105; the loop reads
// terms from the top of the range down to the first one equal to currentTerm),
// for the ranges k_fold's probes left open: wave per kFscanW replies, each
// pending range scanned with the whole wave from its top down, stopping at the
// first hit as Go does. Split from k_fold so the scans of every segment stream
// at once instead of behind each segment's chain of dependent loads (bounds ->
// replies -> replica state -> probe). A hit sets MRAFT_F_COMMITTED on its reply
// and raises the replica's commitIndex (atomicMax: several waves may hold
// ranges of one segment).
__device__ __forceinline__ void fold_scan_blocks(const Dev &s, const int4 *__restrict__ pend,
                                                 const unsigned *__restrict__ pcount, int32_t *__restrict__ flags,
                                                 int64_t bid, int64_t nblk) {
  const int lane = lane_id();
  const int64_t cnt = (int64_t)*pcount;  // k_fold's compact list: nothing pending, nothing to do
  const int L = s.L;
  for (int64_t b0 = bid * kFscanW; b0 < cnt; b0 += nblk * kFscanW) {
    const int64_t i = b0 + lane;
    // the record in one round trip: {lo, hi, slot, currentTerm}, {dummy,
    // head, reply index}
    int4 ra = make_int4(0, -1, 0, 0), rb = make_int4(0, 0, 0, 0);
    if (lane < kFscanW && i < cnt) {
      ra = pend[2 * i];
      rb = pend[2 * i + 1];
    }
    const int lo = ra.x, hi = ra.y;
    for (unsigned long long m = __ballot(hi >= lo); m; m &= m - 1) {
      const int k = first_lane(m);
      const int klo = __builtin_amdgcn_readlane(lo, k), khi = __builtin_amdgcn_readlane(hi, k);
      const int kslot = __builtin_amdgcn_readlane(ra.z, k), kt0 = __builtin_amdgcn_readlane(ra.w, k);
      const int kd = __builtin_amdgcn_readlane(rb.x, k), kh = __builtin_amdgcn_readlane(rb.y, k);
      const int x = wave_scan_down_eq<kFscanU>(s.log + (int64_t)kslot * L, kd, kh, L, klo, khi,
                                                                     kt0);  // klo - 1 if none
      if (lane == k && x >= klo) {
        flags[rb.z] |= MRAFT_F_COMMITTED;                                // :99-100
        atomicMax(&s.commit[kslot], x);
      }
    }
  }
}

// The long path (a segment of more replies than a lane group: k_fold_tail),
// one segment per wave on wave-uniform values. Its own: the replica's state in
// one load per lane over lanes 0..22; the replies in 64-reply batches, lane k
// loading reply k of a batch, so a batch arrives in one round trip; and each
// batch's open a1 ranges scanned in place, wave-cooperatively, at its end.
template <int P>
__device__ __forceinline__ void fold_segment(const Dev &s, const mraft_ae_result *__restrict__ items,
                                             const int64_t *__restrict__ seg_begin, int64_t sg,
                                             const int32_t *__restrict__ seg_err,
                                             const unsigned long long *__restrict__ claim, uint32_t epoch,
                                             int32_t *__restrict__ flags, int32_t *__restrict__ item_err) {
  const int lane = lane_id();
  int64_t b, e;
  const bool any = segment_bounds(seg_begin, sg, b, e);
  int bad = uni(seg_err[sg]);  // the claim verdict: a bad segment's slot may be out of range
  if (!any) return;
  const int64_t cnt = e - b;
  mraft_ae_result it{};
  if (lane < cnt) it = items[b + lane];
  const int slot = __builtin_amdgcn_readfirstlane(it.slot);
  const int me = slot % P;
  const int64_t mrow = (int64_t)slot * P;
  // lanes 0..P-1 matchIndex, 8..8+P-1 nextIndex, 16..22 the scalars
  const int32_t *src = nullptr;
  int64_t si = slot;
  if (lane < P) { src = s.match; si = mrow + lane; }
  else if (lane >= 8 && lane < 8 + P) { src = s.next; si = mrow + lane - 8; }
  else if (lane == 16) src = s.term;
  else if (lane == 17) src = s.role;
  else if (lane == 18) src = s.commit;
  else if (lane == 19) src = s.last;
  else if (lane == 20) src = s.dummy;
  else if (lane == 21) src = s.head;
  else if (lane == 22) src = s.srt;
  const int vs = (src && !bad) ? src[si] : 0;
  const unsigned long long cw = !bad ? claim[slot] : 0ull;  // loaded beside the state
  if (!bad && !claim_owned((uint32_t)uni((int)(uint32_t)cw), (uint32_t)(cw >> 32), epoch, sg)) bad = MRAFT_ITEM_DUP_SLOT;
  int term = __builtin_amdgcn_readlane(vs, 16), role = __builtin_amdgcn_readlane(vs, 17),
      commit = __builtin_amdgcn_readlane(vs, 18);
  const int last = __builtin_amdgcn_readlane(vs, 19), dummy = __builtin_amdgcn_readlane(vs, 20),
            head = __builtin_amdgcn_readlane(vs, 21), srt = __builtin_amdgcn_readlane(vs, 22);
  bool malformed = false;
  for (int64_t base = 0; base < cnt; base += 64) {
    const int64_t i = base + lane;
    if (__ballot(i < cnt && reply_malformed<P>(base > 0 ? items[b + i] : it, slot, me))) malformed = true;
  }
  bad = fold_verdict(bad, malformed, commit, dummy);
  if (bad) {
    for (int64_t i = lane; i < cnt; i += 64) { item_err[b + i] = bad; flags[b + i] = 0; }
    return;
  }
  int m[8], nx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = j < P ? __builtin_amdgcn_readlane(vs, j) : 0;
    nx[j] = j < P ? __builtin_amdgcn_readlane(vs, 8 + j) : 0;
  }
  const int c0 = commit, t0 = term, r0 = role;
  const int32_t *lrow = s.log + (int64_t)slot * s.L;
  bool touched_mn = false;
  int H = commit;
  for (int64_t base = 0; base < cnt; base += 64) {
    if (base > 0 && base + lane < cnt) it = items[b + base + lane];
    const int nb = (int)min((int64_t)64, cnt - base);
    int myfl = 0, plo = 1, phi = 0;  // this lane's reply: flags and a1 range
    for (int k = 0; k < nb; ++k) {
      const int fl = reply_step<P>(LaneReply{it, k}, lane, k, term, role, m, nx, H, last, me, touched_mn, plo, phi);
      if (lane == k) myfl = fl;
    }
    // The batch's a1 ranges: probe every top word at once, scan the rest.
    bool open;
    int x = a1_probe(plo <= phi, lrow, dummy, head, s.L, plo, phi, t0, srt, open);
    for (unsigned long long pend = __ballot(open); pend; pend &= pend - 1) {
      const int src = first_lane(pend);
      const int lo = __shfl(plo, src, 64), hi = __shfl(phi, src, 64) - 1;
      const int r = wave_scan_down_eq<kFoldScanU>(lrow, dummy, head, s.L, lo, hi, t0);  // lo - 1 if none
      if (lane == src && r >= lo) x = r;
    }
    a1_commit<64>(x, myfl, commit);
    if (lane < nb) {
      flags[b + base + lane] = myfl;
      item_err[b + base + lane] = 0;
    }
  }
  fold_write_back<P>(s, slot, mrow, lane == 0, lane < P, lane, term, role, commit, t0, r0, c0, touched_mn, m, nx);
}

// The group path: 64 / GW segments at once, one per GW-lane group, on
// per-group (not wave-uniform) values, so the segments' chains of dependent
// loads (bounds -> replies -> replica state -> probes) overlap in one wave.
// Its own: the replica's state in three loads per lane; no batches (only
// segments of at most GW replies: a longer one goes to the long-segment list,
// the open a1 ranges to the pending list by push_pending, both for
// k_fold_tail); and the replies' address formed from an SGPR base (uni_ptr).
template <int P, int GW>
__device__ __forceinline__ void fold_groupw(const Dev &s, const mraft_ae_result *__restrict__ items,
                                            int64_t n_items, const int64_t *__restrict__ seg_begin, int64_t sg0,
                                            int64_t n_seg, const int32_t *__restrict__ seg_err,
                                            const unsigned long long *__restrict__ claim, uint32_t epoch,
                                            int32_t *__restrict__ flags, int32_t *__restrict__ item_err,
                                            int4 *__restrict__ pend, unsigned *__restrict__ pcount,
                                            unsigned *__restrict__ lcount, int64_t *__restrict__ llist) {
  static_assert(GW >= P && GW >= 7, "a group holds the replica's match / next rows and seven scalars");
  const int lane = lane_id(), gl = lane & (GW - 1);
  const int64_t sg = sg0 + lane / GW;
  const bool live = sg < n_seg;
  int64_t b = 0, e = 0;
  int bad = 0;
  if (live) {
    // (segment_bounds' two edges by value: through its reference arguments
    // k_fold takes up to three more VGPRs and, for 7 and 8 peers, spills)
    b = segment_edge(seg_begin, sg);
    e = segment_edge(seg_begin, sg + 1);
    bad = seg_err[sg];  // the claim verdict: a bad segment's slot may be out of range
  }
  int cnt = (int)(e > b ? min(e - b, (int64_t)(GW + 1)) : 0);  // 0: nothing to fold (empty or inverted)
  {
    // a segment longer than a group goes to the long-segment list (the 64-lane
    // path, k_fold_tail: this kernel stays at 8 waves per SIMD); its group
    // folds nothing here
    const unsigned long long lm = __ballot(gl == 0 && cnt > GW);
    if (lm) {
      const int l0 = first_lane(lm);
      unsigned base = 0;
      if (lane == l0) base = atomicAdd(lcount, (unsigned)__popcll(lm));
      base = (unsigned)__shfl((int)base, l0, 64);
      if (gl == 0 && cnt > GW) llist[base + (unsigned)__popcll(lm & ((1ull << lane) - 1))] = sg;
    }
    if (cnt > GW) cnt = 0;
  }
  (void)n_items;
  mraft_ae_result it{};
  if (gl < cnt) {
    // 32-bit lane offset from an SGPR base, formed here (see uni_ptr)
    const int64_t b0 = (int64_t)(((uint64_t)(uint32_t)uni((int)((uint64_t)b >> 32)) << 32) |
                                 (uint32_t)uni((int)(uint32_t)(uint64_t)b));  // lane 0's b
    int64_t off = b - b0 + gl;
    asm volatile("" : "+v"(off));
    it = uni_ptr(items + b0)[off];
  }
  const int slot = gw_bcast<GW>(it.slot, 0);
  const int me = cnt ? slot % P : 0;
  const int64_t mrow = (int64_t)slot * P;
  // lanes 0..P-1 of the group matchIndex and nextIndex, lanes 0..6 the scalars
  int va = 0, vn = 0, vb = 0;
  if (cnt && !bad) {
    if (gl < P) {
      va = s.match[mrow + gl];
      vn = s.next[mrow + gl];
    }
    const int32_t *src = gl == 0 ? s.term : gl == 1 ? s.role : gl == 2 ? s.commit : gl == 3 ? s.last
                         : gl == 4 ? s.dummy : gl == 5 ? s.head : gl == 6 ? s.srt : nullptr;
    if (src) vb = src[slot];
  }
  const unsigned long long cw = (cnt && !bad) ? claim[slot] : 0ull;  // loaded beside the state
  if (cnt && !bad && !claim_owned((uint32_t)cw, (uint32_t)(cw >> 32), epoch, sg)) bad = MRAFT_ITEM_DUP_SLOT;
  int term = gw_bcast<GW>(vb, 0), role = gw_bcast<GW>(vb, 1), commit = gw_bcast<GW>(vb, 2);
  const int last = gw_bcast<GW>(vb, 3), dummy = gw_bcast<GW>(vb, 4), head = gw_bcast<GW>(vb, 5);
  const int srt = gw_bcast<GW>(vb, 6);
  const bool malformed = gw_mask<GW>(gl < cnt && reply_malformed<P>(it, slot, me)) != 0;
  bad = fold_verdict(bad, malformed, commit, dummy);
  if (bad) {
    if (gl < cnt) { item_err[b + gl] = bad; flags[b + gl] = 0; }
  }
  const bool go = cnt && !bad;
  int m[8], nx[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    m[j] = j < P ? gw_bcast<GW>(va, j) : 0;
    nx[j] = j < P ? gw_bcast<GW>(vn, j) : 0;
  }
  const int c0 = commit, t0 = term, r0 = role;
  const int32_t *lrow = s.log + (int64_t)slot * s.L;
  bool touched_mn = false;
  int H = commit;
  int nmax = 0;
  for (int k = 0; k < GW; ++k)
    if (__ballot(go && k < cnt)) nmax = k + 1;
  int myfl = 0, plo = 1, phi = 0;  // this lane's reply: flags and a1 range
  for (int k = 0; k < nmax; ++k) {
    HeldReply r{};  // reply k of each group
    r.v.peer = gw_bcast<GW>(it.peer, k), r.v.reply_term = gw_bcast<GW>(it.reply_term, k);
    r.v.args_term = gw_bcast<GW>(it.args_term, k), r.v.args_prev_log_index = gw_bcast<GW>(it.args_prev_log_index, k);
    r.v.reply_success = gw_bcast<GW>(it.reply_success, k), r.v.args_n_entries = gw_bcast<GW>(it.args_n_entries, k);
    r.v.reply_conflict_index = gw_bcast<GW>(it.reply_conflict_index, k);
    if (go && k < cnt) {
      const int fl = reply_step<P>(r, gl, k, term, role, m, nx, H, last, me, touched_mn, plo, phi);
      if (gl == k) myfl = fl;
    }
  }
  // a1's ranges of each group: every top word probed at once. The ranges
  // whose top word differs are scanned by k_fold_tail, after this launch: it
  // ORs MRAFT_F_COMMITTED into the reply's flags and raises the replica's
  // commitIndex to the highest index it finds (the ranges of a segment are
  // disjoint and ascending, so "the latest range that found one" is the
  // maximum over all of them, probes included).
  bool open;
  const int x = a1_probe(go && plo <= phi, lrow, dummy, head, s.L, plo, phi, t0, srt, open);
  push_pending(pend, pcount, open, make_int4(plo, phi - 1, slot, t0), make_int4(dummy, head, (int)(b + gl), 0));
  a1_commit<GW>(x, myfl, commit);
  if (go && gl < cnt) {
    flags[b + gl] = myfl;
    item_err[b + gl] = 0;
  }
  fold_write_back<P>(s, slot, mrow, go && gl == 0, go && gl < P, gl, term, role, commit, t0, r0, c0, touched_mn, m, nx);
}

template <int P>
__global__ __launch_bounds__(64, 8) void k_fold(Dev s, const mraft_ae_result *__restrict__ items,
                                                int64_t n_items, const int64_t *__restrict__ seg_begin, int64_t n_seg,
                                                const int32_t *__restrict__ seg_err,
                                                const unsigned long long *__restrict__ claim, uint32_t epoch,
                                                int32_t *__restrict__ flags, int32_t *__restrict__ item_err,
                                                int4 *__restrict__ pend, unsigned *__restrict__ pcount,
                                                unsigned *__restrict__ lcount, int64_t *__restrict__ llist) {
  // lane groups of GW lanes, one segment each (fold_groupw)
  constexpr int NG = kFoldGroups, GW = 64 / NG;
  if ((int64_t)gridDim.x * NG >= n_seg) {
    // each XCD a contiguous range of waves: neighbouring waves' segments
    // share the lines of the replica arrays in one L2
    // (xcd_contiguous(b, nb) written out: the call compiles to other code here)
    const int64_t nb = gridDim.x, b = blockIdx.x, x = b & 7, per = nb >> 3, rem = nb & 7;
    const int64_t wb = x * per + min(x, rem) + (b >> 3);
    fold_groupw<P, GW>(s, items, n_items, seg_begin, NG * wb, n_seg, seg_err, claim, epoch, flags, item_err, pend,
                       pcount, lcount, llist);
    return;
  }
  for (int64_t sg0 = NG * (int64_t)blockIdx.x; sg0 < n_seg; sg0 += NG * (int64_t)gridDim.x)
    fold_groupw<P, GW>(s, items, n_items, seg_begin, sg0, n_seg, seg_err, claim, epoch, flags, item_err, pend,
                       pcount, lcount, llist);
}

// The fold's second launch: the first n_long workgroups fold the segments
// k_fold left for the 64-lane path (longer than a lane group), scanning their
// own ranges, the rest scan the ranges k_fold's probes left open. The two
// halves touch different replicas (one segment per replica slot, the
// claim), so they need no order between them: one kernel boundary fewer per
// fold call.
template <int P>
__global__ __launch_bounds__(64, 8) void k_fold_tail(Dev s, const mraft_ae_result *__restrict__ items,
                                                     const int64_t *__restrict__ seg_begin,
                                                     const int32_t *__restrict__ seg_err,
                                                     const unsigned long long *__restrict__ claim, uint32_t epoch,
                                                     int32_t *__restrict__ flags, int32_t *__restrict__ item_err,
                                                     const int4 *__restrict__ pend, const unsigned *__restrict__ pcount,
                                                     const unsigned *__restrict__ lcount,
                                                     const int64_t *__restrict__ llist, int n_long) {
  if ((int)blockIdx.x < n_long) {
    const int64_t cnt = (int64_t)*lcount;
    for (int64_t k = blockIdx.x; k < cnt; k += n_long)
      fold_segment<P>(s, items, seg_begin, llist[k], seg_err, claim, epoch, flags, item_err);
  } else {
    fold_scan_blocks(s, pend, pcount, flags, (int64_t)blockIdx.x - n_long, (int64_t)gridDim.x - n_long);
  }
}


}  // namespace

void launch_fold(const Dev &s, const mraft_ae_result *items, int64_t n, const int64_t *seg_begin,
                 int64_t n_seg, int64_t gp, unsigned long long *claim, uint32_t epoch, int32_t *seg_err,
                 int32_t *flags, int32_t *item_err, void *scan_buf, hipStream_t st) {
  // one launch for the claims and the zeroed outputs, one for the fold, one
  // for the long segments and the a1 scans the fold's probes left open
  // (scan_buf: fold_scan_bytes(n, n_seg) of scratch)
  const int64_t nt = max(n_seg, n);
  if (nt <= 0 || !scan_buf) return;
  // scan_buf: pend [2 int4 per reply] | pcount | lcount | llist [n_seg int64]
  int4 *pend = (int4 *)scan_buf;                                      // 2 int4 per pending reply
  unsigned *pcount = (unsigned *)(pend + 2 * n);                      // the a1 list's length
  unsigned *lcount = pcount + 1;                                      // the long-segment list's length
  int64_t *llist = (int64_t *)(pend + 2 * n + 1);
  hipLaunchKernelGGL(k_claim_zero, dim3(blocks_for(nt, kMsgBlock)), dim3(kMsgBlock), 0, st, (const char *)items, n_seg,
                     (int)sizeof(mraft_ae_result), (int)offsetof(mraft_ae_result, slot), seg_begin, gp, claim,
                     epoch, seg_err, n, flags, item_err, pcount, lcount);
  if (n_seg <= 0) return;
  const int64_t waves = (n_seg + kFoldGroups - 1) / kFoldGroups;
  const dim3 gr((unsigned)min(waves, (int64_t)MRAFT_FOLD_GRID)), bl(64);
  // the tail's grids: both halves grid-stride over lists whose lengths are
  // read on the device
  const int nl = (int)min(n_seg, (int64_t)MRAFT_FOLD_TAIL_NL);
  const int64_t ns = min((n + kFscanW - 1) / kFscanW, (int64_t)MRAFT_FOLD_TAIL_NS);
  with_peers<1>(s.P, [&](auto pc) {
    constexpr int PP = decltype(pc)::value;
    hipLaunchKernelGGL(k_fold<PP>, gr, bl, 0, st, s, items, n, seg_begin, n_seg, seg_err, claim, epoch, flags,
                       item_err, pend, pcount, lcount, llist);
    hipLaunchKernelGGL(k_fold_tail<PP>, dim3((unsigned)(nl + ns)), bl, 0, st, s, items, seg_begin, seg_err, claim,
                       epoch, flags, item_err, pend, pcount, lcount, llist, nl);
  });
}

size_t fold_scan_bytes(int64_t n, int64_t n_seg) {
  // pend records, two counters, the long-segment list
  return 2 * sizeof(int4) * (size_t)(n > 0 ? n : 0) + sizeof(int4) + sizeof(int64_t) * (size_t)(n_seg > 0 ? n_seg : 1);
}

}  // namespace mraft
