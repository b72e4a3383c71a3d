// mraft_clock_round_kernel.inc — the body of the clock step's first launch
// (A, B and C; described in mraft_clock.hip), included textually by
// k_clock_round and by its counterpart under a reachability mask,
// k_clock_round_reach, so both compile the same statements. Expects P, the
// kernel's arguments s, t, now, flags, cand, lpeer, tg, gflags in scope, and
// REACH (constexpr bool) with reach, the groups' reachability bytes
// (mraft_set_reachable). A (timeouts) and C (the sender) are local and take no
// notice of the mask; B's round does (mraft_elect_round.inc), and the reset of
// a voter that "granted another replica" follows the deliveries through gm.
  const int tid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int g = tid >> 3, p = tid & 7;
  const bool grp = g < s.G;  // uniform over the segment
  const bool act = grp && p < P;
  const int rmask = (REACH && grp) ? (int)reach[g] : -1;  // bit q: replica q is connected
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
