// mraft_clock.hip — the device-resident timers (include/mraft.h "timers") for
// gfx950: ticker() (raft.go:106-125) over two deadline arrays in HBM, the
// reference's seven timer-reset sites, and the clock step of co-resident
// groups.
//
// The clock step's first launch (k_clock_round) uses the election storm's
// layout (mraft_elect.hip): one lane per replica, eight lanes per group, so a
// group's eight deadlines and roles are one segment's registers; the ticker
// (A), one election round (B, the storm's round body included as text from
// mraft_elect_round.inc) and the choice of the sender (C) run on them with
// HBM touched once on entry and once on exit. The tick (D) is the existing
// launch; k_clock_resets (E) follows it with the same layout.
//
// Occupancy: the kernels here declare __launch_bounds__(256) and nothing
// more: the compiler's resource remarks give every kernel 8 waves per SIMD
// with no scratch. k_clock_round<P> takes 35 (P = 1) to 64 (P = 8) VGPRs,
// the last exactly the 64 that 8 waves per SIMD leave each, and 2,560 B of
// LDS per workgroup (DESIGN.md §8d records the figures). Instantiated with
// the reachability pack (k_clock_round<P, uint8_t>, k_clock_resets<uint8_t>;
// mraft_device.h) they hold one more word per lane:
// k_clock_round<8, uint8_t> takes 66 VGPRs, which leaves 7 waves per SIMD;
// P <= 7 keeps 8.
#include "mraft_device.h"
#include "mraft_internal.h"
#include "mraft_timer_draw.h"

namespace mraft {

namespace {

// "Election reset at now" / "heartbeat reset" (include/mraft.h).
__device__ __forceinline__ int election_deadline(const TimerDev &t, int64_t slot, int now) {
  return now + timer_draw(t.cfg, (uint32_t)slot, (uint32_t)now);
}
__device__ __forceinline__ int heartbeat_deadline(const TimerDev &t, int now) { return now + t.cfg.heartbeat; }

// Make's two NewTimer calls (raft.go:66-67) for every slot.
__global__ __launch_bounds__(256) void k_timers_arm_all(TimerDev t, int64_t gp, int now) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= gp) return;
  t.ed[i] = election_deadline(t, i, now);
  t.hd[i] = heartbeat_deadline(t, now);
}

// ... and for the listed slots (restarted replicas); out-of-range slots skipped.
__global__ __launch_bounds__(256) void k_timers_arm(TimerDev t, const int32_t *__restrict__ slots, int64_t n,
                                                    int64_t gp, int now) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t sl = slots[i];
  if (sl < 0 || sl >= gp) return;
  t.ed[sl] = election_deadline(t, sl, now);
  t.hd[sl] = heartbeat_deadline(t, now);
}

// ---------------------------------------------------------------- ticker
// ticker() for every slot, its two lists compacted in ascending slot order
// (mraft_device.h "ordered compaction": list 0 the election timeouts of
// non-leaders, raft.go:112-114, list 1 the leaders' heartbeats, :119-121).
struct TickerLane { bool edue, hdue, list[2]; };
__device__ __forceinline__ TickerLane ticker_lane(const Dev &s, const TimerDev &t, int64_t i, int64_t gp, int now) {
  TickerLane l{false, false, {false, false}};
  if (i < gp) {
    const bool leader = s.role[i] == kLeader;
    l.edue = t.ed[i] <= now;
    l.hdue = t.hd[i] <= now;
    l.list[0] = l.edue && !leader;
    l.list[1] = l.hdue && leader;
  }
  return l;
}

__global__ __launch_bounds__(kCompactBlock) void k_ticker_count(Dev s, TimerDev t, int now,
                                                                int32_t *__restrict__ bcnt) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const TickerLane l = ticker_lane(s, t, i, (int64_t)s.G * s.P, now);
  compact_count<2>(l.list, bcnt, gridDim.x);
}

__global__ __launch_bounds__(kCompactBlock) void k_ticker_emit(
    Dev s, TimerDev t, int now, const int32_t *__restrict__ boff, int64_t cap_e, int64_t cap_h,
    int32_t *__restrict__ oe, int32_t *__restrict__ oh) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const TickerLane l = ticker_lane(s, t, i, (int64_t)s.G * s.P, now);
  int64_t off[2];
  compact_offsets<2>(l.list, boff, gridDim.x, off);
  // A listed slot whose entry does not fit keeps its due timer (the caller
  // calls again for the rest); every other due timer is reset (:111, :118).
  if (l.edue) {
    const bool fits = off[0] < cap_e;
    if (l.list[0] && fits) oe[off[0]] = (int32_t)i;
    if (!l.list[0] || fits) t.ed[i] = election_deadline(t, i, now);
  }
  if (l.hdue) {
    const bool fits = off[1] < cap_h;
    if (l.list[1] && fits) oh[off[1]] = (int32_t)i;
    if (!l.list[1] || fits) t.hd[i] = heartbeat_deadline(t, now);
  }
}

// ---------------------------------------------------------------- reset sites
// The resets that follow a message-path call, from the arrays it returned
// (include/mraft.h mraft_timers_note): one lane per item. Items that repeat a
// slot write the same deadline (the draw depends on slot and now only).
__global__ __launch_bounds__(256) void k_timers_note(TimerDev t, int kind, const void *__restrict__ records,
                                                     const void *__restrict__ outcome,
                                                     const int32_t *__restrict__ item_err, int64_t n,
                                                     int64_t gp, int now) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (item_err && item_err[i] != 0) return;
  int64_t slot = -1;
  bool hit = false;
  switch (kind) {
    case MRAFT_NOTE_AE_HANDLED: {                                      // raft_append_entry.go:121
      const mraft_ae_args *a = (const mraft_ae_args *)records + i;
      slot = a->slot;
      hit = ((const mraft_ae_reply *)outcome)[i].term <= a->term;
      break;
    }
    case MRAFT_NOTE_IS_HANDLED: {                                      // raft_snapshot.go:30
      const mraft_is_args *a = (const mraft_is_args *)records + i;
      slot = a->slot;
      hit = ((const mraft_is_reply *)outcome)[i].term <= a->term;
      break;
    }
    case MRAFT_NOTE_RV_HANDLED:                                        // raft_election.go:72
      slot = ((const mraft_rv_args *)records)[i].slot;
      hit = ((const mraft_rv_reply *)outcome)[i].vote_granted != 0;
      break;
    case MRAFT_NOTE_AE_FOLDED:                                         // raft_append_entry.go:71
      slot = ((const mraft_ae_result *)records)[i].slot;
      hit = (((const int32_t *)outcome)[i] & MRAFT_F_STEPPED_DOWN) != 0;
      break;
    case MRAFT_NOTE_IS_FOLDED:                                         // raft_snapshot.go:63
      slot = ((const mraft_is_result *)records)[i].slot;
      hit = (((const int32_t *)outcome)[i] & MRAFT_F_STEPPED_DOWN) != 0;
      break;
    case MRAFT_NOTE_RV_FOLDED:                                         // raft_election.go:39
      slot = ((const mraft_rv_result *)records)[i].slot;
      hit = (((const int32_t *)outcome)[i] & MRAFT_F_BECAME_LEADER) != 0;
      break;
    default: break;
  }
  if (!hit || slot < 0 || slot >= gp) return;
  if (kind == MRAFT_NOTE_RV_FOLDED)
    t.hd[slot] = heartbeat_deadline(t, now);
  else
    t.ed[slot] = election_deadline(t, slot, now);
}

// ---------------------------------------------------------------- clock step
// A (ticker), B (one election round) and C (the sender) of mraft_clock_step
// for eight groups per wave. The state registers, the LDS words and the round
// body are k_election_rounds' (mraft_elect.hip); this kernel adds the two
// deadlines per lane, the per-voter grant (gm, left in scope by the round
// body) and the sender's choice by segment shuffles.
// Under the reachability pack (mraft_device.h) A (timeouts) and C (the sender)
// are local and take no notice of the mask; B's round does
// (mraft_elect_round.inc), and the reset of a voter that "granted another
// replica" follows the deliveries through gm.
template <int P, class... M>
__global__ __launch_bounds__(256) void k_clock_round(Dev s, TimerDev t, int now, unsigned flags,
                                                     uint8_t *__restrict__ cand, int32_t *__restrict__ lpeer,
                                                     int32_t *__restrict__ tg, int32_t *__restrict__ gflags,
                                                     const M *__restrict__... reach) {
  constexpr bool REACH = reach_given<M...>();  // false: rmask is the constant all-ones
  const int tid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int g = tid >> 3, p = tid & 7;
  const bool grp = g < s.G;  // uniform over the segment
  const bool act = grp && p < P;
  const int rmask = grp ? reach_byte(g, reach...) : -1;  // bit q: replica q is connected
  const long long sl = (long long)g * P + p;
  int term = 0, voted = -1, role = kFollower, votes = 0, last = 0, lterm = 0;
  int ed = INT32_MAX, hd = INT32_MAX;
  if (act) {
    term = s.term[sl];
    voted = s.voted[sl];
    role = s.role[sl];
    votes = s.votes[sl];
    last = s.last[sl];
    lterm = term_at(s, sl, s.dummy[sl], s.head[sl], last);             // lastEntry, raft_log.go:50-53
    ed = t.ed[sl];
    hd = t.hd[sl];
  }
  constexpr int kVJunk = 0x100;  // votedFor outside [-1, P): as in k_election_rounds
  const int pb = 1 << p;
  int vb = voted == -1 ? 0 : ((unsigned)voted < (unsigned)P ? 1 << voted : kVJunk);
  int upm = 0;  // bit c: candidate c's log is up to date for this voter (raft_log.go:99-104)
#pragma unroll
  for (int c = 0; c < P; ++c) {
    const int clt = __shfl(lterm, c, 8), clast = __shfl(last, c, 8);
    upm |= (int)(clt > lterm || (clt == lterm && clast >= last)) << c;
  }
  __shared__ int lds_cx[256];
  __shared__ __attribute__((aligned(8))) uint8_t lds_gm[256];
  __shared__ int lds_rt[256];
  __shared__ __attribute__((aligned(8))) uint8_t lds_rc[256];
  const int seg = (int)(threadIdx.x & 63) & ~7;
  int fl = 0, became = 0, pd = 0;

  // A. ticker (raft.go:106-125). Every reset of this replica in this step
  // happens at `now`, so they all set the same deadline.
  const int ed_new = act ? election_deadline(t, sl, now) : 0;
  const int hd_new = heartbeat_deadline(t, now);
  const bool edue = act && ed <= now, hdue = act && hd <= now;
  ed = edue ? ed_new : ed;                                             // :111
  const bool fired = hdue && role == kLeader;                          // :119-121; its reset comes in C
  hd = (hdue && role != kLeader) ? hd_new : hd;                        // :118
  const int m = (int)((__ballot(edue) >> seg) & 0xffull);              // the round's timeouts (:112-114)

  // B. one election round
#include "mraft_elect_round.inc"
  ed = (act && (gm & ~pb) != 0) ? ed_new : ed;                         // granted another replica, raft_election.go:72
  hd = became ? hd_new : hd;                                           // :39

  // C. the sender: highest currentTerm, lowest peer on a tie
  const int elig = act && role == kLeader && (fired || became || (flags & MRAFT_CLOCK_SEND_ALL));
  int bp = -1, bt = 0;
#pragma unroll
  for (int c = 0; c < P; ++c) {
    const int ce = __shfl(elig, c, 8), ct = __shfl(term, c, 8);
    const bool take = ce && (bp < 0 || ct > bt);
    bt = take ? ct : bt;
    bp = take ? c : bp;
  }
  hd = (act && p == bp) ? hd_new : hd;

  const unsigned long long el = __ballot(fl & MRAFT_G_ELECTED), sd = __ballot(fl & MRAFT_G_STEPPED_DOWN);
  if (grp && p == 0) {
    if (cand) cand[g] = (uint8_t)cm;
    lpeer[g] = bp;
    tg[g] = bt;
    if (gflags)
      gflags[g] = (((el >> seg) & 0xffull) ? MRAFT_G_ELECTED : 0) |
                  (((sd >> seg) & 0xffull) ? MRAFT_G_STEPPED_DOWN : 0);
  }
  if (!act) return;
  s.term[sl] = term;
  s.voted[sl] = (vb & kVJunk) ? voted : (vb ? __builtin_ctz(vb) : -1);
  s.role[sl] = role;
  s.votes[sl] = votes;
  t.ed[sl] = ed;
  t.hd[sl] = hd;
  if (pd) mark_persist(s, sl, MRAFT_PERSIST_STATE);
  if (became) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      s.match[sl * P + j] = 0;
      s.next[sl * P + j] = last + 1;
    }
  }
}

// E. the resets of the tick, from its group flags and the terms it left: a
// follower whose term equals the sender's pre-tick term passed the term gate
// of its handler (raft_append_entry.go:121, raft_snapshot.go:30); a sender
// that stepped down reset its own timer (:71, raft_snapshot.go:63).
// Under the reachability pack a non-sender heard the sender only when its bit
// and the sender's are both set; without it the word is all-ones and `heard`
// compiles to true. (A sender that is cut off folds no reply, so it never
// carries STEPPED_DOWN.)
template <class... M>
__global__ __launch_bounds__(256) void k_clock_resets(Dev s, TimerDev t, int now,
                                                      const int32_t *__restrict__ gflags,
                                                      const int32_t *__restrict__ lpeer,
                                                      const int32_t *__restrict__ tg,
                                                      const M *__restrict__... reach) {
  static_assert(sizeof...(M) <= 1, "the reachability pack holds no pointer or one");
  const int tid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int g = tid >> 3, p = tid & 7;
  if (g >= s.G || p >= s.P) return;
  const int gf = gflags[g];
  if (!(gf & MRAFT_G_ACTIVE) || (gf & MRAFT_G_ERROR)) return;
  const long long sl = (long long)g * s.P + p;
  const int lp = lpeer[g], rmask = reach_byte(g, reach...);
  const bool heard = ((rmask >> p) & 1) && ((rmask >> (lp & 7)) & 1);
  const bool hit = p != lp ? heard && s.term[sl] == tg[g] : (gf & MRAFT_G_STEPPED_DOWN) != 0;
  if (hit) t.ed[sl] = election_deadline(t, sl, now);
}

}  // namespace

void launch_timers_arm_all(const TimerDev &t, int64_t gp, int32_t now, hipStream_t st) {
  hipLaunchKernelGGL(k_timers_arm_all, dim3(blocks_for(gp)), dim3(256), 0, st, t, gp, now);
}

void launch_timers_arm(const TimerDev &t, const int32_t *slots, int64_t n, int64_t gp, int32_t now,
                       hipStream_t st) {
  hipLaunchKernelGGL(k_timers_arm, dim3(blocks_for(n)), dim3(256), 0, st, t, slots, n, gp, now);
}

void launch_ticker(const Dev &s, const TimerDev &t, int32_t now, int32_t *bcnt, int32_t *oe, int64_t cap_e,
                   int64_t *n_e, int32_t *oh, int64_t cap_h, int64_t *n_h, hipStream_t st) {
  const int64_t nb = ticker_blocks((int64_t)s.G * s.P);
  hipLaunchKernelGGL(k_ticker_count, dim3((unsigned)nb), dim3(kCompactBlock), 0, st, s, t, now, bcnt);
  launch_compact_scan(bcnt, nb, 2, n_e, n_h, st);
  hipLaunchKernelGGL(k_ticker_emit, dim3((unsigned)nb), dim3(kCompactBlock), 0, st, s, t, now, bcnt, cap_e, cap_h,
                     oe, oh);
}

void launch_timers_note(const TimerDev &t, int kind, const void *records, const void *outcome,
                        const int32_t *item_err, int64_t n, int64_t gp, int32_t now, hipStream_t st) {
  hipLaunchKernelGGL(k_timers_note, dim3(blocks_for(n)), dim3(256), 0, st, t, kind, records, outcome, item_err, n,
                     gp, now);
}

void launch_clock_round(const Dev &s, const TimerDev &t, int32_t now, uint32_t flags, uint8_t *cand,
                        int32_t *lpeer, int32_t *tg, int32_t *eflags, const uint8_t *reach, hipStream_t st) {
  const dim3 gr(blocks_for((int64_t)s.G * 8)), bl(256);
  with_peers<1>(s.P, [&](auto pc) {
    constexpr int P = decltype(pc)::value;
    if (reach)
      hipLaunchKernelGGL((k_clock_round<P, uint8_t>), gr, bl, 0, st, s, t, now, flags, cand, lpeer, tg, eflags, reach);
    else
      hipLaunchKernelGGL(k_clock_round<P>, gr, bl, 0, st, s, t, now, flags, cand, lpeer, tg, eflags);
  });
}

void launch_clock_resets(const Dev &s, const TimerDev &t, int32_t now, const int32_t *gflags,
                         const int32_t *lpeer, const int32_t *tg, const uint8_t *reach, hipStream_t st) {
  const dim3 gr(blocks_for((int64_t)s.G * 8)), bl(256);
  if (reach)
    hipLaunchKernelGGL(k_clock_resets<uint8_t>, gr, bl, 0, st, s, t, now, gflags, lpeer, tg, reach);
  else
    hipLaunchKernelGGL(k_clock_resets<>, gr, bl, 0, st, s, t, now, gflags, lpeer, tg);
}

}  // namespace mraft
