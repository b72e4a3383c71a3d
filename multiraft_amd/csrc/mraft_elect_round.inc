// mraft_elect_round.inc — one election round of an 8-lane group segment: the
// body of k_election_rounds' round loop (mraft_elect.hip) and of the clock
// step's election round (mraft_clock.hip), included as text so both compile
// the same statements.
//
// The including scope provides, per lane (replica p of group g):
//   P (constexpr), p, pb = 1 << p, act, seg, m (the round's timeout mask),
//   upm (isLogUpToDate bits), the replica's registers term, vb, role, votes,
//   the accumulators fl, became, pd, and the __shared__ arrays lds_cx, lds_gm,
//   lds_rt, lds_rc (256 entries each);
//   REACH (constexpr bool) and rmask, the group's reachability word
//   (mraft_set_reachable, bit q: replica q is connected). A kernel without the
//   reachability pack (mraft_device.h) has REACH = false with rmask the
//   constant all-ones, and every test of it compiles away. Under a mask candidate c's RequestVote reaches voter v, and
//   v's reply reaches c, iff both their bits are set; timeouts and
//   StartElection are local and happen either way.
// It leaves in scope: isc (this lane ran StartElection), gm (bit c: this voter
// granted candidate c's RequestVote; a candidate's own bit is set by its
// delivery to itself, so "granted another replica" is (gm & ~pb) != 0).
    const int isc = act && ((m >> p) & 1) && role != kLeader;
    if (isc) {                                                         // StartElection :6-17
      role = kCandidate;
      term += 1;
      vb = pb;
      votes = 1;
      pd = 1;
    }
    const int at = term;  // args.Term of this lane's RequestVote (when isc); voter's term before RVs
    int cx[8];
    // One broadcast per replica per round, through this wave's LDS words: its
    // term with the candidate bit on top.
    const int mycx = at;
    lds_cx[threadIdx.x] = mycx;
    __builtin_amdgcn_wave_barrier();
    {
      const int4 a = *reinterpret_cast<const int4 *>(&lds_cx[threadIdx.x & ~7u]);
      const int4 b = *reinterpret_cast<const int4 *>(&lds_cx[(threadIdx.x & ~7u) + 4]);
      cx[0] = a.x; cx[1] = a.y; cx[2] = a.z; cx[3] = a.w;
      cx[4] = b.x; cx[5] = b.y; cx[6] = b.z; cx[7] = b.w;
    }
    // RequestVote deliveries: voter p handles the candidates in peer order
    // (HandleRequestVote :54-77). pmx = max args.Term over candidates c <= p,
    // which with the voter's own pre-delivery term gives every reply.Term the
    // tally below needs (a voter's term after handling c is the max of the
    // two, the stale branch included).
    int gm = 0, pmx = INT32_MIN;
    // The segment's candidate mask (ascending peer order is the delivery order).
    const unsigned long long cb = __ballot(isc);
    const int cm = (int)((cb >> seg) & 0xffull);
    // the candidates whose RequestVote this replica receives
    const int conn = REACH ? (rmask >> p) & 1 : 1;
    const int cmv = REACH ? (conn ? cm & rmask : 0) : cm;
    pd |= (int)(act && (cmv & ~(1 << p)) != 0);                        // :57, every RV this voter handles
    // The segment's candidates ranked in peer order: rank k's args.Term and
    // peer index staged through LDS once per round and held in registers, so
    // the delivery loop has no LDS round trip per candidate and a compile-time
    // register index per iteration (round 6: 0.164 -> 0.149 ms per storm;
    // round 5's loop walked the candidate mask with a ds_bpermute per
    // candidate in its dependent chain, profiles/r6_e1)
    {
      // every lane writes one rank slot: a candidate its rank (args.Term, its
      // bit), the others the slots past the segment's candidates (INT_MIN, bit
      // 0: a delivery that changes nothing), so the loop needs no validity test
      const int ncand = __builtin_popcount(cm);
      const int rk = __builtin_popcount(cm & (pb - 1));
      const int pos = isc ? rk : ncand + p - rk;
      lds_rt[(threadIdx.x & ~7u) + pos] = isc ? at : INT32_MIN;
      lds_rc[(threadIdx.x & ~7u) + pos] = (uint8_t)(isc ? pb : 0);
      __builtin_amdgcn_wave_barrier();
      const int4 ra = *reinterpret_cast<const int4 *>(&lds_rt[threadIdx.x & ~7u]);
      const int4 rb = *reinterpret_cast<const int4 *>(&lds_rt[(threadIdx.x & ~7u) + 4]);
      const unsigned long long rcs = *reinterpret_cast<const unsigned long long *>(&lds_rc[threadIdx.x & ~7u]);
      __builtin_amdgcn_wave_barrier();
      const int rt[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
      // A candidate's delivery to itself (cb == pb) changes nothing: its term
      // is at >= cat, and at term == at its vote is already its own; the grant
      // bit it sets in gm is masked out of its tally (om). So no c != p test.
#pragma unroll
      for (int k = 0; k < P; ++k) {
        if (!__ballot(k < ncand)) break;
        int cb = (int)((rcs >> (8 * k)) & 0xffull);
        int cat = rt[k];
        if (REACH && !(cb & cmv)) {  // not delivered: the slot past the candidates, which changes nothing
          cb = 0;
          cat = INT32_MIN;
        }
        pmx = cb <= pb ? max(pmx, cat) : pmx;                          // c <= p
        const bool gt = cat > term;                                    // :63-66
        const bool ge = cat >= term;                                   // :59-62 (stale: no change)
        term = gt ? cat : term;
        vb = gt ? 0 : vb;
        const bool grant = ge & (((vb & ~cb) | (cb & ~upm)) == 0);     // :69-74
        vb = grant ? cb : vb;
        gm |= grant ? cb : 0;
      }
      role = term > at ? kFollower : role;                             // :63-66 (some RV carried a higher term)
    }
    // Grants transposed through LDS: byte v of the segment's word = voter v's
    // grant mask; bit v of mine = voter v granted this lane.
    int mine = 0;
    {
      lds_gm[threadIdx.x] = (uint8_t)gm;
      __builtin_amdgcn_wave_barrier();
      const unsigned long long gw = *reinterpret_cast<const unsigned long long *>(&lds_gm[threadIdx.x & ~7u]);
      mine = (int)((((gw >> p) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
      __builtin_amdgcn_wave_barrier();
    }
    // Tally (closure :22-47): candidate p folds its replies in voter order.
    // The guard (:29) can only flip at the first event, becoming leader at the
    // grant that makes a majority (:32-38) or stepping down at the first
    // refusal whose reply.Term exceeds args.Term (:42-45), so the fold is
    // closed-form: whichever of the two positions comes first in voter order.
    // Under a mask the same holds inside the connected set: a connected
    // candidate receives every other connected candidate's RequestVote, as
    // every connected voter does, so pmx on its lane is the pmx of each voter
    // whose reply it gets; its grants (mine) can only come from voters its
    // RequestVote reached, its refusals (smask) are restricted to them, and
    // the majority stays P/2 grants of all P. A candidate that is cut off
    // hears no reply: it skips the tally and stays Candidate with its own vote.
    {
      bool ok0 = isc && term == at && role == kCandidate;
      if (REACH) ok0 = ok0 && conn;
      const int om = ((1 << P) - 1) & ~(1 << p);
      int gt = 0, tv = 0;
#pragma unroll
      for (int v = 0; v < P; ++v) gt |= (int)((cx[v]) > at) << v;
      // reply.Term = max(voter's own term, pmx) > at: every refusal when pmx > at.
      const int smask = om & ~mine & (pmx > at ? om : gt) & (REACH ? rmask : -1);
      int mm = mine & om;
#pragma unroll
      for (int k = 1; k < (P / 2 > 1 ? P / 2 : 1); ++k) mm &= mm - 1;  // the (P/2)-th grant
      const int lpos = mm ? __builtin_ctz(mm) : 32;
      const int spos = smask ? __builtin_ctz(smask) : 32;
      tv = lds_cx[(threadIdx.x & ~7u) + min(spos, 7)];  // used only when spos < P
      const bool lead = ok0 && lpos < spos;
      const bool sd = ok0 && spos < lpos;
      const int upos = lead ? lpos + 1 : spos;                          // < 32 when lead | sd
      const int upto = (lead | sd) ? (int)((1u << (upos & 31)) - 1u) : -1;
      votes += ok0 ? __builtin_popcount(mine & om & upto) : 0;                // :31
      role = lead ? kLeader : sd ? kFollower : role;
      became |= (int)lead;
      fl |= lead ? MRAFT_G_ELECTED : 0;
      term = sd ? max(tv, pmx) : term;
      vb = sd ? 0 : vb;
      fl |= sd ? MRAFT_G_STEPPED_DOWN : 0;
    }
