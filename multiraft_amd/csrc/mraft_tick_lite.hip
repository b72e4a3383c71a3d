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
// While a reachability mask is set (mraft_set_reachable) k_tick_lite runs with
// the reachability pack (mraft_device.h) and also lists every group with a
// replica cut off.
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
template <int P, bool START, class... M>
__global__ __launch_bounds__(64 * kLiteWaves, 8) void k_tick_lite(Dev s, const int32_t *__restrict__ leader_peer,
                                                               int32_t *__restrict__ gflags, Export ex,
                                                               int32_t *__restrict__ fb_list,
                                                               unsigned *__restrict__ fb_count, int cap,
                                                               StartIO sio, const M *__restrict__... reach) {
  constexpr bool REACH = reach_given<M...>();  // false: no statement of the mask remains
  __shared__ unsigned sh_cnt, sh_base;
  const int lane = lane_id(), j = lane & 7, gbase = lane & ~7, wv = (int)(threadIdx.x >> 6);
  const int xcd = (int)(blockIdx.x & 7);
  const int wb = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);  // as k_tick_group
  if (threadIdx.x == 0) sh_cnt = 0;
  const int g = (wb * kLiteWaves + wv) * 8 + (lane >> 3);
  const bool live = g < s.G;
  const int L = s.L;
  // Round trip 1: everything that does not depend on which peer leads. Lane
  // j < P of the group: replica j's scalars, its persist bits and column j of
  // the group's P x P nextIndex block (every candidate leader's view of j).
  const long long r = (long long)g * P + j;
  const bool rl = live && j < P;
  int lpv = -1, rrole = 0, rterm = 0, rcommit = 0, rlast = 0, rdummy = 0, rhead = 0, rsrt = 0, rpd = 0;
  int nx[P];
#pragma unroll
  for (int x = 0; x < P; ++x) nx[x] = 0;
  int kcnt = 0;  // START: entries to append at the leader
  if (live) lpv = leader_peer[g];
  if (START && live) kcnt = sio.counts[g];
  if (rl) {
    rrole = s.role[r]; rterm = s.term[r]; rcommit = s.commit[r]; rlast = s.last[r];
    rdummy = s.dummy[r]; rhead = s.head[r]; rsrt = s.srt[r];
    if (s.pdirty) rpd = s.pdirty[r];
#pragma unroll
    for (int x = 0; x < P; ++x) nx[x] = s.next[((long long)g * P + x) * P + j];
  }
  auto bc = [&](int v, int k) { return __shfl(v, gbase + k, 64); };
  {
    const int c_0 = bc(rcommit, 0), t_0 = bc(rterm, 0), r_0 = bc(rrole, 0);
    if (live && (lpv < 0 || lpv >= P) && j == 0) {
      if (gflags) gflags[g] = lpv >= P ? MRAFT_G_ERROR : 0;
      ex.put(g, c_0, t_0, r_0);  // mraft_export_group_status: replica 0
    }
  }
  bool go = live && lpv >= 0 && lpv < P;
  const int lp = go ? lpv : 0;
  const int role = bc(rrole, lp), T = bc(rterm, lp), c0 = bc(rcommit, lp), last0 = bc(rlast, lp),
            ldummy = bc(rdummy, lp), lhead = bc(rhead, lp), lsrt0 = bc(rsrt, lp);
  // START: mraft_start's decision (k_start_groups' preamble, start_fits) for the group's leader replica
  bool started = false;
  int serr = 0;
  if (START && live) {
    if (lpv >= 0 && lpv < P) {
      if (kcnt < 0) {
        serr = MRAFT_ITEM_BAD_SLOT;
      } else if (kcnt > 0 && role == kLeader) {                          // raft.go:93-95
        started = start_fits(last0, kcnt, ldummy, L);
        if (!started) serr = MRAFT_ITEM_LOG_FULL;
      }
    } else if (lpv >= P && kcnt != 0) {
      serr = MRAFT_ITEM_BAD_SLOT;
    }
    if (j == 0) {
      sio.oi[g] = started ? last0 + 1 : -1;                              // :103
      sio.ot[g] = started ? T : -1;
      sio.ol[g] = started ? 1 : 0;
      sio.err[g] = serr;
    }
  }
  const int last = started ? last0 + kcnt : last0;                       // :96-100
  if (go && (role != kLeader || c0 < ldummy)) {  // appendOneRound returns (:22-25) / MRAFT_ITEM_BAD_STATE
    if (j == 0) {
      if (gflags) gflags[g] = role != kLeader ? 0 : MRAFT_G_ERROR;
      ex.put(g, c0, T, role);
    }
    go = false;
  }
  int nj = 0;
#pragma unroll
  for (int x = 0; x < P; ++x) if (x == lp) nj = nx[x];
  const long long lrow = ((long long)g * P + lp) * L, f = r;
  const int lb = lhead - ldummy;
  const bool isf = go && j < P && j != lp;
  const int fterm = rterm, fdummy = rdummy, flast = rlast, fcommit = rcommit, fhead = rhead;
  const int prev = nj - 1, n = last - prev;                              // :26, :50
  // decided by round trip 1: snapshot, panic, stale, below / beyond the
  // follower's log, a merge that would compare (the follower holds entries
  // past prev) or run past the ring's capacity -> the full tick
  // IC_BELOW (prev below the follower's dummy, :123-127): Go returns before
  // setting reply.Term, so with currentTerm > 0 the leader's gate (:73-74)
  // drops the reply — the follower's own words only (role, term adoption,
  // persist), settled here too
  const bool bel = isf && prev >= ldummy && prev <= last && T >= fterm && prev < fdummy && T > 0;
  bool fb = isf && !bel && (prev < ldummy || prev > last || T < fterm || prev < fdummy || prev > flast ||
                            (n > 0 && (flast != prev || n > kLiteSpan || (long long)last - fdummy > (long long)L - 1)));
  const bool mrg = isf && !fb && !bel && n > 0;
  // successful replies: with at least P/2 of them the last evaluation of a1's
  // order statistic is `last` (so top = min(M*, last) = last); with none, a1
  // never runs; in between (few) a1 runs on an order statistic that still
  // holds older matchIndex words, settled below when it cannot pass commitIndex
  const bool succ = isf && !fb && !bel;
  const int nsucc = __popcll(__ballot(succ) >> gbase & 0xffull);
  const bool few = nsucc > 0 && nsucc < P / 2;
  bool gfb = ((__ballot(fb) >> gbase) & 0xffull) != 0;
  // REACH: a group with a replica cut off (its mask not all-ones over its P
  // replicas) is not settled here: it goes to the list, after its Start, and
  // k_tick_list runs it under the mask. A fully connected group settles
  // exactly as without a mask.
  if (REACH) {
    const int rmask = live ? reach_byte(g, reach...) : -1;
    gfb = gfb || (rmask & ((1 << P) - 1)) != (1 << P) - 1;
  }
  // Round trip 2 (groups still settling here): prevLogTerm at leader and
  // follower, a1's probe log[last] and each merging follower's first four
  // entries to append (its own lane loads the leader's words).
  const bool t2 = go && !gfb;
  int pt = 0, ft = 0, probe = 0, mj = 0;
  int e4[4] = {0, 0, 0, 0};
  // (START: Indexes above last0 are the entries Start appends, currentTerm)
  if (t2) {
    if (few && isf) mj = s.match[((long long)g * P + lp) * P + j];     // the leader's matchIndex[j]
    if (isf && !bel) {
      pt = (START && prev > last0) ? T : s.log[lrow + ring(prev + lb, L)];  // :49
      ft = s.log[f * L + ring(prev - fdummy + fhead, L)];                // :128
    }
    if (mrg) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < n) e4[u] = (START && prev + 1 + u > last0) ? T : s.log[lrow + ring(prev + 1 + u + lb, L)];
    }
  }
  // a1's probe (:98) of the pre-Start last: the tick's top when nothing was
  // appended, and Start's terms_sorted rule (k_start) when something was
  if ((t2 || started) && j == lp) probe = s.log[lrow + ring(last0 + lb, L)];
  if (t2 && isf && !bel && ft != pt) fb = true;                          // a conflict: the full tick
  const int pr0 = bc(probe, lp);
  const int t = started ? T : pr0;  // log[last]: an appended entry's term when Start appended
  // the leader's terms_sorted after Start: cleared when an older entry above
  // the dummy carries a term above currentTerm
  const bool sclr = started && last0 > ldummy && pr0 > T;
  const int lsrt = sclr ? 0 : lsrt0;
  if (START && started && j == lp) {
    const long long sl = (long long)g * P + lp;
    if (sclr) s.srt[sl] = 0;
    for (int u = 1; u <= kcnt; ++u) s.log[lrow + ring(last0 + u + lb, L)] = T;
    s.last[sl] = last;
    if (s.pdirty) s.pdirty[sl] = rpd | MRAFT_PERSIST_STATE;             // :101
  }
  int commit = c0, ftop = 0, pq = 0;
  gfb = gfb || ((__ballot(fb) >> gbase) & 0xffull) != 0;
  if (__ballot(t2 && few)) {
    // few successes (fewer than P/2): a1 runs after each of them (:78) on
    // quorum_rt's order statistic — the (P/2)-th largest follower matchIndex —
    // over words each success raises to `last`, the others' older words kept.
    // With no success lowering its word (old <= last) the evaluations' tops
    // rise to the last one's, so a1's ranges cover (commitIndex, top] and its
    // probe of log[top] settles it as for top = last below; otherwise, over
    // each follower's larger word, a bound on every evaluation's top that at
    // or below commitIndex means a1 changes nothing. Else the full tick.
    const int mm = isf ? (succ ? max(mj, last) : mj) : INT32_MIN;
    int c = 0;
#pragma unroll
    for (int q = 0; q < P; ++q) c += (bc((int)isf, q) && bc(mm, q) >= mm) ? 1 : 0;  // followers at or above mine
    int qv = (isf && c >= P / 2) ? mm : INT32_MIN;
#pragma unroll
    for (int q = 0; q < P; ++q) qv = max(qv, bc(qv, q));
    const bool mono = ((__ballot(succ && mj > last) >> gbase) & 0xffull) == 0;
    ftop = min(qv, last);
    if (go && few && ftop > c0) {
      if (!mono) gfb = true;
      else if (j == lp) pq = (START && ftop > last0) ? T : s.log[lrow + ring(ftop + lb, L)];  // :98
    }
    const int pqv = bc(pq, lp);
    if (go && few && !gfb && ftop > c0) {
      if (pqv == T) commit = ftop;                                       // :98-100
      else if (!(lsrt && pqv < T)) gfb = true;                           // a scan: the full tick
    }
  }
  if (go && !gfb && nsucc > 0 && !few && last > c0) {                    // top = last (above)
    if (t == T) commit = last;                                           // :98-100
    else if (!(lsrt && t < T)) gfb = true;                               // a Figure-8 scan: the full tick
  }
  const bool w = go && !gfb;
  // the appended entries, Indexes prev + 1 .. last, by the follower's own lane
  // (:149-155; the compare range is empty); past the first four, four at a time
  if (w && mrg) {
    const long long frow = f * L;
    const int fb0 = prev + 1 - fdummy + fhead;  // ring position of Index prev + 1, before the wrap
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (u < n) s.log[frow + ring(fb0 + u, L)] = e4[u];
    for (int c = 4; c < n; c += 4) {
      int x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        x[u] = c + u >= n ? 0 : (START && prev + 1 + c + u > last0) ? T : s.log[lrow + ring(prev + 1 + c + u + lb, L)];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (c + u < n) s.log[frow + ring(fb0 + c + u, L)] = x[u];
    }
  }
  bool fcadv = false;
  if (w && isf) {
    if (s.pdirty) s.pdirty[f] = rpd | MRAFT_PERSIST_STATE;              // :111 (mark_persist)
    if (T > fterm) { s.term[f] = T; s.voted[f] = -1; }                   // :116-118
    s.role[f] = kFollower;                                               // :120
  }
  if (w && isf && !bel) {
    int newlast = flast;
    if (n > 0) {
      newlast = last;                                                    // prev + n
      s.last[f] = newlast;
      // terms_sorted after appending from prev + 1 (the tick's rule, mk = 0)
      const bool fl = lsrt != 0 && (prev != ldummy || pt <= e4[0]);  // e4[0]: the entry at prev + 1
      const int sw = !fl ? 0 : prev == fdummy ? 1 : -1;
      if (sw >= 0) s.srt[f] = sw;
    }
    if (c0 > fcommit) {                                                  // :157-160
      s.commit[f] = min(c0, newlast);
      fcadv = true;
    }
    s.next[((long long)g * P + lp) * P + j] = last + 1;                  // :76-77
    s.match[((long long)g * P + lp) * P + j] = last;
  }
  const bool anyadv = ((__ballot(fcadv) >> gbase) & 0xffull) != 0;
  if (w && j == 0) {
    if (commit != c0) s.commit[(long long)g * P + lp] = commit;
    if (gflags)
      gflags[g] = MRAFT_G_ACTIVE | (commit != c0 ? MRAFT_G_COMMITTED : 0) | (anyadv ? MRAFT_G_FOLLOWER_COMMIT : 0);
    ex.put(g, commit, T, kLeader);
  }
  // The groups for the full tick: one LDS count per wave, one global atomic
  // per workgroup on its XCD's counter (one device-wide counter hit by every
  // wave serialised the launch: 72 us for 65,536 groups, profiles/r6_l4), the
  // list entries in the XCD's region of cap groups.
  const bool push = go && gfb && j == 0;
  const unsigned long long pmask = __ballot(push);
  unsigned woff = 0;
  if (pmask && lane == first_lane(pmask)) woff = atomicAdd(&sh_cnt, (unsigned)__popcll(pmask));
  woff = (unsigned)__shfl((int)woff, pmask ? first_lane(pmask) : 0, 64);
  __syncthreads();
  if (threadIdx.x == 0) sh_base = sh_cnt ? atomicAdd(&fb_count[xcd * kLiteCntStride], sh_cnt) : 0u;
  __syncthreads();
  if (push) fb_list[(long long)xcd * cap + sh_base + woff + (unsigned)__popcll(pmask & ((1ull << lane) - 1))] = g;
}

template <int P>
void launch_tick_lite_p(const Dev &s, const int32_t *lpeer, int32_t *gflags, Export ex, const LiteBufs &lb,
                        const StartIO *sio, const uint8_t *reach, hipStream_t st) {
  const dim3 gr((unsigned)lite_blocks(s.G)), bl(64 * kLiteWaves);
  const int cap = lite_cap(s.G);
  if (reach) {
    if (sio)
      hipLaunchKernelGGL((k_tick_lite<P, true, uint8_t>), gr, bl, 0, st, s, lpeer, gflags, ex, lb.list, lb.cnt, cap,
                         *sio, reach);
    else
      hipLaunchKernelGGL((k_tick_lite<P, false, uint8_t>), gr, bl, 0, st, s, lpeer, gflags, ex, lb.list, lb.cnt, cap,
                         StartIO{}, reach);
  } else if (sio) {
    hipLaunchKernelGGL((k_tick_lite<P, true>), gr, bl, 0, st, s, lpeer, gflags, ex, lb.list, lb.cnt, cap, *sio);
  } else {
    hipLaunchKernelGGL((k_tick_lite<P, false>), gr, bl, 0, st, s, lpeer, gflags, ex, lb.list, lb.cnt, cap, StartIO{});
  }
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
