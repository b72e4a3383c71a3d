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
// LDS per workgroup (DESIGN.md §8d records the figures). Their counterparts
// under a reachability mask (k_clock_round_reach, k_clock_resets_reach;
// DESIGN.md §8e) hold one more word per lane: k_clock_round_reach<8> takes 66
// VGPRs, which leaves 7 waves per SIMD; P <= 7 keeps 8.
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
template <int P>
__global__ __launch_bounds__(256) void k_clock_round(Dev s, TimerDev t, int now, unsigned flags,
                                                     uint8_t *__restrict__ cand, int32_t *__restrict__ lpeer,
                                                     int32_t *__restrict__ tg, int32_t *__restrict__ gflags) {
  constexpr bool REACH = false;  // no reachability mask: rmask is the constant all-ones
  constexpr const uint8_t *reach = nullptr;
#include "mraft_clock_round_kernel.inc"
}

// k_clock_round under a reachability mask (mraft_set_reachable): launched only
// while a mask is set.
template <int P>
__global__ __launch_bounds__(256) void k_clock_round_reach(Dev s, TimerDev t, int now, unsigned flags,
                                                           uint8_t *__restrict__ cand, int32_t *__restrict__ lpeer,
                                                           int32_t *__restrict__ tg, int32_t *__restrict__ gflags,
                                                           const uint8_t *__restrict__ reach) {
  constexpr bool REACH = true;
#include "mraft_clock_round_kernel.inc"
}

// E. the resets of the tick, from its group flags and the terms it left: a
// follower whose term equals the sender's pre-tick term passed the term gate
// of its handler (raft_append_entry.go:121, raft_snapshot.go:30); a sender
// that stepped down reset its own timer (:71, raft_snapshot.go:63).
__global__ __launch_bounds__(256) void k_clock_resets(Dev s, TimerDev t, int now,
                                                      const int32_t *__restrict__ gflags,
                                                      const int32_t *__restrict__ lpeer,
                                                      const int32_t *__restrict__ tg) {
  const int tid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int g = tid >> 3, p = tid & 7;
  if (g >= s.G || p >= s.P) return;
  const int gf = gflags[g];
  if (!(gf & MRAFT_G_ACTIVE) || (gf & MRAFT_G_ERROR)) return;
  const long long sl = (long long)g * s.P + p;
  const bool hit = p != lpeer[g] ? s.term[sl] == tg[g] : (gf & MRAFT_G_STEPPED_DOWN) != 0;
  if (hit) t.ed[sl] = election_deadline(t, sl, now);
}

// E under a reachability mask: a non-sender heard the sender only when its bit
// and the sender's are both set; the rest of the rule is k_clock_resets'. (A
// sender that is cut off folds no reply, so it never carries STEPPED_DOWN.)
__global__ __launch_bounds__(256) void k_clock_resets_reach(Dev s, TimerDev t, int now,
                                                            const int32_t *__restrict__ gflags,
                                                            const int32_t *__restrict__ lpeer,
                                                            const int32_t *__restrict__ tg,
                                                            const uint8_t *__restrict__ reach) {
  const int tid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int g = tid >> 3, p = tid & 7;
  if (g >= s.G || p >= s.P) return;
  const int gf = gflags[g];
  if (!(gf & MRAFT_G_ACTIVE) || (gf & MRAFT_G_ERROR)) return;
  const long long sl = (long long)g * s.P + p;
  const int lp = lpeer[g], rmask = (int)reach[g];
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
  if (reach) {
    with_peers<1>(s.P, [&](auto pc) {
      hipLaunchKernelGGL(k_clock_round_reach<decltype(pc)::value>, gr, bl, 0, st, s, t, now, flags, cand, lpeer, tg,
                         eflags, reach);
    });
    return;
  }
  with_peers<1>(s.P, [&](auto pc) {
    hipLaunchKernelGGL(k_clock_round<decltype(pc)::value>, gr, bl, 0, st, s, t, now, flags, cand, lpeer, tg, eflags);
  });
}

void launch_clock_resets(const Dev &s, const TimerDev &t, int32_t now, const int32_t *gflags,
                         const int32_t *lpeer, const int32_t *tg, const uint8_t *reach, hipStream_t st) {
  if (reach) {
    hipLaunchKernelGGL(k_clock_resets_reach, dim3(blocks_for((int64_t)s.G * 8)), dim3(256), 0, st, s, t, now, gflags,
                       lpeer, tg, reach);
    return;
  }
  hipLaunchKernelGGL(k_clock_resets, dim3(blocks_for((int64_t)s.G * 8)), dim3(256), 0, st, s, t, now, gflags, lpeer,
                     tg);
}

}  // namespace mraft
