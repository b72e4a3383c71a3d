// mraft_tick_lite.hip — the light tick's first launch (k_tick_lite) for gfx950;
// its fallback launch, k_tick_list, is the full tick of mraft_tick.hip.
//
// MRAFT_TICK_LIGHT (mraft_set_tick_mode). The tick of a running deployment —
// every follower caught up to its nextIndex, a heartbeat or a few appended
// entries — is a handful of dependent word loads per group and almost no
// streaming, so a wave per group spends its life waiting on them
// (secondary.steady_state_config3: 0.117 ms per 65,536-group tick, 285 GB/s).
// k_tick_lite gives each group eight lanes (eight Raft groups per wave, lane j
// = peer j), so eight groups' chains overlap in one wave. It settles a group
// only when every follower's reply is a success that needs no compare:
// prevLogTerm matches and either n = 0 (heartbeat, IC_HB) or the follower's
// log ends at prev (a pure append: IC_MERGE with an empty compare range, so
// the first mismatch is prev + 1), the append fits the ring, the leader's
// entries to send span at most kLiteSpan Indexes, and a1 settles at its top:
// with every follower at `last`, min(M*, last) = last (the order statistic of
// the last evaluation is `last`), and log[last] is currentTerm, or below it
// under the leader's terms_sorted proof. Every other group (stale or
// adopting-with-conflict replies, snapshots, conflicts, merges that compare,
// Figure-8 scans, capacity) is recognised before any store and appended to a
// device list that k_tick_list runs through the full tick
// (mraft_tick_body.inc). Per group the stores are the full tick's.
// The kernel's body is mraft_tick_lite_body.inc, included by k_tick_lite and by
// k_tick_lite_reach, which runs while a reachability mask is set
// (mraft_set_reachable) and also lists every group with a replica cut off.
#include "mraft_device.h"
#include "mraft_internal.h"
#include "mraft_rules.h"

namespace mraft {

namespace {

constexpr int kLiteSpan = 64;
constexpr int kLiteWaves = 4;  // waves per light workgroup: 32 groups, one list reservation
static_assert(kLiteWaves * 8 == kLiteBlockGroups, "the groups of a light workgroup (mraft_internal.h)");

// START (mraft_start_and_tick): Start (raft.go:90-104) of counts[g] entries at
// the group's leader replica first, inside this launch: the leader lane
// appends them (start_fits, then terms_sorted, lastIndex and the persist bit
// as start_at does, mraft_rules.h: here spread over lanes and round trips) and the
// tick runs on the result — the new entries' terms are currentTerm, known
// without a load (the followers' copies and a1's probe of the new last).
// Groups that fall back carry their Start's stores into the full tick.
template <int P, bool START>
__global__ __launch_bounds__(64 * kLiteWaves, 8) void k_tick_lite(Dev s, const int32_t *__restrict__ leader_peer,
                                                               int32_t *__restrict__ gflags, Export ex,
                                                               int32_t *__restrict__ fb_list,
                                                               unsigned *__restrict__ fb_count, int cap,
                                                               StartIO sio) {
  constexpr bool REACH = false;  // no reachability mask
  constexpr const uint8_t *reach = nullptr;
#include "mraft_tick_lite_body.inc"
}

// k_tick_lite under a reachability mask (mraft_set_reachable): launched only
// while a mask is set.
template <int P, bool START>
__global__ __launch_bounds__(64 * kLiteWaves, 8) void k_tick_lite_reach(Dev s, const int32_t *__restrict__ leader_peer,
                                                                     int32_t *__restrict__ gflags, Export ex,
                                                                     int32_t *__restrict__ fb_list,
                                                                     unsigned *__restrict__ fb_count, int cap,
                                                                     StartIO sio, const uint8_t *__restrict__ reach) {
  constexpr bool REACH = true;
#include "mraft_tick_lite_body.inc"
}

template <int P>
void launch_tick_lite_p(const Dev &s, const int32_t *lpeer, int32_t *gflags, Export ex, const LiteBufs &lb,
                        const StartIO *sio, const uint8_t *reach, hipStream_t st) {
  if (reach) {
    if (sio)
      hipLaunchKernelGGL((k_tick_lite_reach<P, true>), dim3((unsigned)lite_blocks(s.G)), dim3(64 * kLiteWaves), 0, st,
                         s, lpeer, gflags, ex, lb.list, lb.cnt, lite_cap(s.G), *sio, reach);
    else
      hipLaunchKernelGGL((k_tick_lite_reach<P, false>), dim3((unsigned)lite_blocks(s.G)), dim3(64 * kLiteWaves), 0, st,
                         s, lpeer, gflags, ex, lb.list, lb.cnt, lite_cap(s.G), StartIO{}, reach);
    return;
  }
  if (sio)
    hipLaunchKernelGGL((k_tick_lite<P, true>), dim3((unsigned)lite_blocks(s.G)), dim3(64 * kLiteWaves), 0, st, s,
                       lpeer, gflags, ex, lb.list, lb.cnt, lite_cap(s.G), *sio);
  else
    hipLaunchKernelGGL((k_tick_lite<P, false>), dim3((unsigned)lite_blocks(s.G)), dim3(64 * kLiteWaves), 0, st, s,
                       lpeer, gflags, ex, lb.list, lb.cnt, lite_cap(s.G), StartIO{});
}

}  // namespace

void launch_replicate_tick_light(const Dev &s, const int32_t *lpeer, int32_t *gflags, int32_t *exp_commit,
                                 int32_t *exp_term_leader, const LiteBufs &lb, const StartIO *sio,
                                 const uint8_t *reach, hipStream_t st) {
  if (with_peers<2>(s.P, [&](auto pc) {
        launch_tick_lite_p<decltype(pc)::value>(s, lpeer, gflags, Export{exp_commit, exp_term_leader}, lb, sio, reach,
                                                st);
      })) {
    launch_tick_list(s, lpeer, gflags, exp_commit, exp_term_leader, lb, reach, st);
  } else {  // P == 1: the full tick's k_tick_p1 is a lane per group already
    if (sio) launch_start_groups(s, lpeer, *sio, st);
    launch_replicate_tick(s, lpeer, gflags, exp_commit, exp_term_leader, reach, st);
  }
}

}  // namespace mraft
