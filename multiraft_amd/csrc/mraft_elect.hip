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
// While a reachability mask is set (mraft_set_reachable, include/mraft.h) the
// host launches k_election_rounds with the reachability pack (mraft_device.h),
// which compiles the mask's tests in: candidate c's RequestVote reaches voter
// v, and v's reply reaches c, iff both their bits are set
// (mraft_elect_round.inc).
#include "mraft_device.h"
#include "mraft_internal.h"

namespace mraft {

namespace {

template <int P, class... M>
__global__ __launch_bounds__(256) void k_election_rounds(Dev s, const uint8_t *__restrict__ cand,
                                                         int R, int32_t *__restrict__ gflags,
                                                         const M *__restrict__... reach) {
  constexpr bool REACH = reach_given<M...>();  // false: rmask is the constant all-ones
  // Lane p of an 8-lane segment holds replica p of group g (P <= 8): voters
  // and candidates work in parallel, candidate data is broadcast inside the
  // segment (__shfl width 8).
  const int tid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int g = tid >> 3, p = tid & 7;
  const bool grp = g < s.G;  // uniform over the segment
  const bool act = grp && p < P;
  const int rmask = grp ? reach_byte(g, reach...) : -1;  // bit q: replica q is connected
  const long long sl = (long long)g * P + p;
  int term = 0, voted = -1, role = kFollower, votes = 0, last = 0, lterm = 0;
  if (act) {
    term = s.term[sl];
    voted = s.voted[sl];
    role = s.role[sl];
    votes = s.votes[sl];
    last = s.last[sl];
    lterm = term_at(s, sl, s.dummy[sl], s.head[sl], last);             // lastEntry, raft_log.go:50-53
  }
  // votedFor as a bit: 1 << votedFor, 0 for -1, kVJunk for a value outside
  // [-1, P) (no candidate ever equals it, as in Go's compare at :69-74)
  constexpr int kVJunk = 0x100;
  const int pb = 1 << p;
  int vb = voted == -1 ? 0 : ((unsigned)voted < (unsigned)P ? 1 << voted : kVJunk);
  // The logs do not change during an election storm, so isLogUpToDate of
  // every candidate's (lastTerm, lastIndex) against this voter's
  // (raft_log.go:99-104) is fixed for the launch: bit c of upm.
  int upm = 0;
#pragma unroll
  for (int c = 0; c < P; ++c) {
    const int clt = __shfl(lterm, c, 8), clast = __shfl(last, c, 8);
    upm |= (int)(clt > lterm || (clt == lterm && clast >= last)) << c;
  }
  __shared__ int lds_cx[256];
  __shared__ __attribute__((aligned(8))) uint8_t lds_gm[256];
  __shared__ int lds_rt[256];                                  // rank k's args.Term, per segment
  __shared__ __attribute__((aligned(8))) uint8_t lds_rc[256];  // rank k's peer index
  const int seg = (int)(threadIdx.x & 63) & ~7;
  int fl = 0, became = 0, pd = 0;  // pd: persist() ran (StartElection :15, HandleRequestVote :57, :45)
  // The round's timeout mask, loaded one round ahead. (Staging 64 rounds of
  // masks through LDS per cooperative load measured 1 % slower, r5_c1 / r5_e3.)
  int mnext = (grp && R > 0) ? (int)cand[g] : 0;
  for (int r = 0; r < R; ++r) {
    const int m = mnext;
    if (grp && r + 1 < R) mnext = (int)cand[(long long)(r + 1) * s.G + g];
    // the round body, shared as text with the clock step (mraft_clock.hip)
#include "mraft_elect_round.inc"
  }
  const unsigned long long el = __ballot(fl & MRAFT_G_ELECTED), sd = __ballot(fl & MRAFT_G_STEPPED_DOWN);
  if (grp && p == 0 && gflags) {
    gflags[g] = (((el >> seg) & 0xffull) ? MRAFT_G_ELECTED : 0) |
                (((sd >> seg) & 0xffull) ? MRAFT_G_STEPPED_DOWN : 0);
  }
  if (!act) return;
  s.term[sl] = term;
  s.voted[sl] = (vb & kVJunk) ? voted : (vb ? __builtin_ctz(vb) : -1);
  s.role[sl] = role;
  s.votes[sl] = votes;
  if (pd) mark_persist(s, sl, MRAFT_PERSIST_STATE);
  if (became) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      s.match[sl * P + j] = 0;
      s.next[sl * P + j] = last + 1;
    }
  }
}

}  // namespace

void launch_election_rounds(const Dev &s, const uint8_t *cand, int R, int32_t *gflags, const uint8_t *reach,
                            hipStream_t st) {
  const dim3 gr((unsigned)blocks_for((int64_t)s.G * 8)), bl(256);
  with_peers<1>(s.P, [&](auto pc) {
    constexpr int P = decltype(pc)::value;
    if (reach)
      hipLaunchKernelGGL((k_election_rounds<P, uint8_t>), gr, bl, 0, st, s, cand, R, gflags, reach);
    else
      hipLaunchKernelGGL(k_election_rounds<P>, gr, bl, 0, st, s, cand, R, gflags);
  });
}

}  // namespace mraft
