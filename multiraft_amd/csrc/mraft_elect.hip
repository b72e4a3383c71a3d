// mraft_elect.hip — the election storm (SURVEY.md §8a rows a5-a6, §8d
// config #5) for gfx950: one lane per replica, eight lanes per group (eight
// groups per wave); each replica's election state (term, votedFor, role,
// grantedVotes, last index/term) lives in registers for all R rounds of one
// launch, so HBM is touched once on entry and once on exit. Per round: timeouts -> StartElection (raft_election.go:4-15) in peer
// order, every RequestVote delivered voter by voter in candidate order
// (HandleRequestVote :54-77 with isLogUpToDate, raft_log.go:99-104), every
// candidate's tally in voter order (closure :22-47).
//
// Round 5 (profiles/r5_e1 README): one lane per group, two lanes per group,
// a dense voter loop, a branch-free vote-key loop and LDS-staged round masks
// were all measured (parity green) and all slower; this layout hides its
// dependent chains with 8 waves per SIMD. Round 6 (profiles/r6_e1): the
// instruction account of the round body matched the counters exactly (84 VALU
// + 19 SALU per wave-round plus 29 + 13 per candidate, 3.0 candidates per
// wave-round), fewer instructions per candidate alone changed nothing, and
// taking the per-candidate LDS round trip out of the delivery loop's
// dependent chain (candidates ranked once per round, held in registers) took
// the storm 9 % down; the loop's conditions as bitwise ops (no exec-mask
// region per candidate: 126 -> 77 SALU per round body) 1.5 % more
// (profiles/r6_d1).
//
// The kernel's body is mraft_elect_kernel.inc, included by k_election_rounds
// here and by k_election_rounds_reach (mraft_elect_reach.hip), which runs while
// a reachability mask is set (mraft_set_reachable): a RequestVote and its reply
// then pass only between two connected replicas (mraft_elect_round.inc).
#include "mraft_device.h"
#include "mraft_internal.h"

namespace mraft {

namespace {

template <int P>
__global__ __launch_bounds__(256) void k_election_rounds(Dev s, const uint8_t *__restrict__ cand,
                                                         int R, int32_t *__restrict__ gflags) {
  constexpr bool REACH = false;  // no reachability mask: rmask is the constant all-ones
  constexpr const uint8_t *reach = nullptr;
#include "mraft_elect_kernel.inc"
}

}  // namespace

void launch_election_rounds(const Dev &s, const uint8_t *cand, int R, int32_t *gflags, const uint8_t *reach,
                            hipStream_t st) {
  const dim3 gr((unsigned)blocks_for((int64_t)s.G * 8)), bl(256);
  if (reach) {  // under a reachability mask: mraft_elect_reach.hip
    launch_election_rounds_reach(s, cand, R, gflags, reach, st);
    return;
  }
  with_peers<1>(s.P, [&](auto pc) {
    hipLaunchKernelGGL(k_election_rounds<decltype(pc)::value>, gr, bl, 0, st, s, cand, R, gflags);
  });
}

}  // namespace mraft
