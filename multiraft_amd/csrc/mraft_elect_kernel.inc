// mraft_elect_kernel.inc — the body of the election storm's kernel
// (described in mraft_elect.hip), included textually by k_election_rounds and
// by its counterpart under a reachability mask, k_election_rounds_reach, so
// both compile the same statements. Expects P, the kernel's arguments s, cand,
// R, gflags in scope, and REACH (constexpr bool) with reach, the groups'
// reachability bytes (mraft_set_reachable).
  // Lane p of an 8-lane segment holds replica p of group g (P <= 8): voters
  // and candidates work in parallel, candidate data is broadcast inside the
  // segment (__shfl width 8).
  const int tid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int g = tid >> 3, p = tid & 7;
  const bool grp = g < s.G;  // uniform over the segment
  const bool act = grp && p < P;
  const int rmask = (REACH && grp) ? (int)reach[g] : -1;  // bit q: replica q is connected
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
