// mraft_tick.hip — the fused co-resident replication tick (SURVEY.md §8a rows
// a1-a4) for gfx950: one 64-lane wave per Raft group, one group per 64-thread
// workgroup (a wave's slot is released the moment its group is done; with
// 4-wave workgroups a finished wave held its slot until its siblings ended,
// idling ~18 % of the slots — tools/trace_tick.py).
//
// Per group (wave):
//   header   wave-uniform scalar loads of the leader replica (role, term,
//            commit, last, dummy);
//   phase A  lane per follower: appendOneRound's args gather
//            (raft_append_entry.go:20-54) and HandleAppendEntries up to
//            matchLog (:108-133): term check/adoption, prev < dummy,
//            prev > last, prev-term match;
//   phase B  wave-cooperative: the ConflictIndex backward scans (:136-142) and
//            ONE streaming pass over the leader's log tail that serves every
//            follower's entry merge at once (:149-155): each 256-entry chunk of
//            the leader log is loaded once (dwordx4 per lane) and compared
//            against / copied into every follower whose range covers it, the
//            first mismatch of each follower found by ballot. The reference
//            copies the tail into every follower's args (:50-54); here the
//            leader's entries cross HBM once per group;
//   phase C  lane per follower: follower state write-back, follower commit
//            (:157-160);
//   phase D  wave-uniform fold of the replies in peer order
//            (processAppendEntriesReply, :66-88) with the quorum order
//            statistic over matchIndex in registers, and the current-term gate
//            of advanceCommitIndexForLeader (:89-105): one probe of
//            log[min(M*, last)], a wave-cooperative downward scan only when it
//            misses (Figure-8 groups).
//
// COUNT=true runs the same decisions with no state store and accumulates the
// algorithmic word count of DESIGN.md §4 (reads, writes, active groups).
//
// Every kernel that runs the tick's body (mraft_tick_body.inc) is here:
// k_tick_group and k_tick_list, the light tick's fallback launch over the
// groups that k_tick_lite (mraft_tick_lite.hip) lists.
#include "mraft_device.h"
#include "mraft_internal.h"
#include "mraft_pass.h"
#include "mraft_rules.h"

namespace mraft {

namespace {

enum : int {
  IC_NONE = 0,  // no AppendEntries for this item
  IC_SNAP,      // prev < leader dummy: InstallSnapshot path
  IC_PANIC,     // prev > leader last: Go panics
  IC_GO,        // args gathered
  IC_STALE,     // args.Term < currentTerm
  IC_BELOW,     // prev < follower dummy
  IC_BEYOND,    // prev > follower last
  IC_MISMATCH,  // term(prev) differs, ConflictIndex known without a scan
  IC_SCAN,      // term(prev) differs, ConflictIndex needs the backward scan
  IC_MERGE,     // prefix matches, n > 0 entries to merge
  IC_HB,        // prefix matches, heartbeat
  IC_FULL,      // merge would exceed capacity L: rejected
  IC_IS_STALE,  // InstallSnapshot, args.Term < currentTerm (raft_snapshot.go:20-22)
  IC_IS_OLD,    // InstallSnapshot, outdated snapshot (:31-33)
  IC_IS_INSTALL,// InstallSnapshot installed (:35-50)
  IC_IS_PANIC   // InstallSnapshot whose sliceFrom would panic: dropped
};

__device__ __forceinline__ long long interval_len(long long a, long long b) {
  return b >= a ? b - a + 1 : 0;
}

// The state pointers again, read afresh from the kernel-argument segment (the
// tick's first argument is the Dev struct). Phase C/D use this copy, so the
// entry copy of the ~14 array pointers dies after the header instead of being
// held (and spilled) across the streaming pass; the segment pointer is passed
// through an empty asm so the loads are new scalar loads, not the entry ones.
__device__ __forceinline__ Dev reload_dev() {
  const __attribute__((address_space(4))) Dev *kp =
      (const __attribute__((address_space(4))) Dev *)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  Dev d;
  d.term = kp->term; d.voted = kp->voted; d.role = kp->role; d.commit = kp->commit;
  d.applied = kp->applied; d.dummy = kp->dummy; d.last = kp->last; d.votes = kp->votes;
  d.log = kp->log; d.match = kp->match; d.next = kp->next; d.pdirty = kp->pdirty;
  d.head = kp->head; d.hsnap = kp->hsnap; d.srt = kp->srt; d.G = kp->G; d.P = kp->P; d.L = kp->L;
  return d;
}

// Reply fold of one group (processAppendEntriesReply, :66-88, in peer order),
// wave-uniform. Inputs per follower slot q come from lane q. The fold keeps
// only what the rest of the tick needs (bit q of gate_m: the reply passed the
// term/state/prev gate; of rs_m: it set matchIndex), so little wave-uniform
// state stays live across the streaming pass; phase D recomputes each lane's
// nextIndex / matchIndex from its own item. COUNT keeps the per-reply arrays
// the algorithmic word count reads.
// (The rule this restates in ballot-mask form: reply_step, mraft_fold.hip.)
template <int P, bool COUNT>
struct Fold {
  static constexpr int NI = P - 1;
  static constexpr int NA = COUNT ? NI : 1;
  int term, stepped, any, mstar, gate_m, rs_m;
  int rp[NA], ic[NA];

  // is_m: followers whose reply is an InstallSnapshot reply
  // (processInstallSnapshotReply, raft_snapshot.go:56-69) for
  // LastIncludedIndex lii; their (prev, n) read (lii, 0).
  __device__ __forceinline__ void run(int T, int lp, int (&mm)[P], int have_m, int succ_m, int is_m, int lii,
                                      int rterm, int prev, int n, int rci, int icls) {
    term = T;
    stepped = 0;
    any = 0;
    mstar = INT32_MIN;
    gate_m = 0;
    rs_m = 0;
    int role = kLeader;
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      const int pq = q < lp ? q : q + 1;
      int qrp = uni(__shfl(prev, q, 64)), qrn = uni(__shfl(n, q, 64));
      const int qic = uni(__shfl(icls, q, 64));
      if (qic >= IC_IS_STALE) {
        qrp = lii;
        qrn = 0;
      }
      if (COUNT) {
        rp[q < NA ? q : 0] = qrp;
        ic[q < NA ? q : 0] = qic;
      }
      const int rt = uni(__shfl(rterm, q, 64));
      if (!((have_m >> q) & 1)) continue;
      if (rt > term) {                                                   // :67-72, snapshot :59-64
        term = rt;
        role = kFollower;
        stepped = 1;
      } else if ((is_m >> q) & 1) {
        if (role == kLeader && T == term) {                              // snapshot :65-67
          gate_m |= 1 << q;
          rs_m |= 1 << q;
#pragma unroll
          for (int j = 0; j < P; ++j)
            if (j == pq) mm[j] = lii;
        }
      } else if (rt == term && role == kLeader && T == term) {           // :73-74 (prev gate holds)
        gate_m |= 1 << q;
        if ((succ_m >> q) & 1) {
          rs_m |= 1 << q;
#pragma unroll
          for (int j = 0; j < P; ++j)
            if (j == pq) mm[j] = qrp + qrn;                              // :76
          mstar = max(mstar, quorum<P>(mm, lp));                   // :78 -> a1
          any = 1;
        }
      }
    }
  }
};

#ifndef MRAFT_TICK_MINW
#define MRAFT_TICK_MINW 8  // __launch_bounds__ minimum waves per SIMD
#endif
#ifndef MRAFT_TICK_ALIGN
#define MRAFT_TICK_ALIGN 32  // pass chunks start on this many entries (32 = one 128-B line)
#endif
#ifndef MRAFT_TICK_TRACE
#define MRAFT_TICK_TRACE 0  // diagnostic build: s_memrealtime stamps per group (tools/trace_tick.py)
#endif
#if MRAFT_TICK_TRACE
__device__ unsigned long long g_tick_trace[65536 * 4];
// the XCD (XCC) this wave runs on, kept in the top bits of the entry stamp
__device__ __forceinline__ unsigned long long tick_xcc() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return (unsigned long long)(v & 15);
}
#define TICK_STAMP(k)                                                                        \
  do {                                                                                       \
    if (!COUNT && g < 65536 && lane == 0) g_tick_trace[g * 4 + (k)] = __builtin_amdgcn_s_memrealtime() | ((k) == 0 ? tick_xcc() << 60 : 0ull); \
  } while (0)
#else
#define TICK_STAMP(k) do {} while (0)
#endif
#ifndef MRAFT_TICK_SCANU
#define MRAFT_TICK_SCANU 1  // ConflictIndex scans past the probe: 64 * SCANU terms per round trip
#endif
#ifndef MRAFT_TICK_CMP_EPL
#define MRAFT_TICK_CMP_EPL 4  // compare chunk: 64 * EPL entries (4: dwordx4 per lane, 2: dwordx2)
#endif
// One wave (group) per 64-thread workgroup: each wave's slot frees as soon as
// its group ends (four per workgroup, the group order without the XCD mapping,
// the compare chunks without software pipelining, two dwordx4 per lane per
// chunk and the state pointers held across the pass all measured slower; git
// history keeps them).
//
// With the reachability pack (mraft_device.h; mraft_set_reachable) the body
// runs with REACH, reach[g] one more wave-uniform byte of its header. Launched
// so only while a mask is set, and never with COUNT
// (mraft_replicate_tick_count is defined for the full network only).
template <int P, bool COUNT, class... M>
__global__ __launch_bounds__(64, MRAFT_TICK_MINW) void k_tick_group(Dev s, const int32_t *__restrict__ leader_peer,
                                                    int32_t *__restrict__ gflags,
                                                    unsigned long long *__restrict__ counts, Export ex,
                                                    const M *__restrict__... reach) {
  constexpr int NI = P - 1;
  constexpr bool REACH = reach_given<M...>();
  const int lane = lane_id();
  // Each XCD a contiguous range of groups, so the scalar SoA lines
  // neighbouring groups share stay in one XCD's L2. Speed only; any placement
  // gives the same results.
  const int gb = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
  // (threadIdx.x >> 6 is 0 in a one-wave workgroup; without the term the
  // compiler assigns this kernel's registers differently, so the measured
  // code is kept instruction-for-instruction)
  const int g = uni(gb + (int)(threadIdx.x >> 6));
  if (g >= s.G) return;
#define TICK_EXIT return
#include "mraft_tick_body.inc"
#undef TICK_EXIT
}

// P == 1: no peers, so no AppendEntries and no reply ever reaches a1.
__global__ void k_tick_p1(Dev s, const int32_t *__restrict__ leader_peer,
                          int32_t *__restrict__ gflags, unsigned long long *__restrict__ counts,
                          int count, Export ex) {
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g >= s.G) return;
  const int lp = leader_peer[g];
  int fl = 0;
  unsigned long long R = 0, A = 0;
  if (lp >= 1) {
    fl = MRAFT_G_ERROR;
  } else if (lp == 0) {
    R = 1;
    if (s.role[g] == kLeader) {
      R = 5;
      if (s.commit[g] < s.dummy[g]) fl = MRAFT_G_ERROR;
      else { fl = MRAFT_G_ACTIVE; A = 1; R = 6; }  // + terms_sorted (DESIGN.md §4 header words)
    }
  }
  if (count) {
    atomicAdd(&counts[kCountWords * (blockIdx.x & (kCountStripes - 1)) + 0], R);
    atomicAdd(&counts[kCountWords * (blockIdx.x & (kCountStripes - 1)) + 2], A);
  } else {
    if (gflags) gflags[g] = fl;
    ex.put(g, s.commit[g], s.term[g], s.role[g]);
  }
}

// The light tick's fallback: the groups k_tick_lite (mraft_tick_lite.hip)
// listed (eight XCD lists of cap entries, their counts kLiteCntStride words
// apart), each through the full tick
// (one wave per group, grid-stride over the device counts, so any grid is
// exact; the host sizes it from the previous tick's count). The first
// workgroup zeroes the counters the next light tick uses and publishes this
// tick's count to the host's pinned word.
// Under a reachability pack the walk is the same and the body runs with
// REACH: the masked light launch (mraft_tick_lite.hip) lists every group whose
// mask is incomplete, so this is where a partitioned group's tick runs in
// light mode.
template <int P, class... M>
__global__ __launch_bounds__(64, MRAFT_TICK_MINW) void k_tick_list(Dev s, const int32_t *__restrict__ leader_peer,
                                                   int32_t *__restrict__ gflags,
                                                   unsigned long long *__restrict__ counts, Export ex,
                                                   const int32_t *__restrict__ list, const unsigned *__restrict__ cnt,
                                                   unsigned *__restrict__ cnt_next, long long *__restrict__ hint,
                                                   int cap, const M *__restrict__... reach) {
  constexpr bool COUNT = false, REACH = reach_given<M...>();
  constexpr int NI = P - 1;
  const int lane = lane_id();
  unsigned c8[8], nl = 0;
#pragma unroll
  for (int x = 0; x < 8; ++x) {
    c8[x] = (unsigned)uni((int)cnt[x * kLiteCntStride]);
    nl += c8[x];
  }
  if (blockIdx.x == 0) {
    if (lane < 8) cnt_next[lane * kLiteCntStride] = 0;
    if (lane == 0 && hint) __hip_atomic_store(hint, (long long)nl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  for (unsigned k = blockIdx.x; k < nl; k += gridDim.x) {
    unsigned base = 0;
    int x = 0;
#pragma unroll
    for (int y = 0; y < 7; ++y)
      if (x == y && k >= base + c8[y]) { base += c8[y]; x = y + 1; }
    const int g = uni(list[(long long)x * cap + (k - base)]);
#define TICK_EXIT continue
#include "mraft_tick_body.inc"
#undef TICK_EXIT
  }
}

template <int P, bool COUNT>
void launch_tick_p(const Dev &s, const int32_t *lpeer, int32_t *gflags, unsigned long long *counts,
                   Export ex, hipStream_t st) {
  hipLaunchKernelGGL((k_tick_group<P, COUNT>), dim3(s.G), dim3(64), 0, st, s, lpeer, gflags, counts, ex);
}

template <bool COUNT>
void launch_tick_c(const Dev &s, const int32_t *lpeer, int32_t *gflags, unsigned long long *counts,
                   Export ex, hipStream_t st) {
  if (!with_peers<2>(s.P, [&](auto pc) {
        launch_tick_p<decltype(pc)::value, COUNT>(s, lpeer, gflags, counts, ex, st);
      }))
    hipLaunchKernelGGL(k_tick_p1, dim3(blocks_for(s.G)), dim3(256), 0, st, s, lpeer, gflags, counts, COUNT ? 1 : 0,
                       ex);
}

}  // namespace

#if MRAFT_TICK_TRACE
extern "C" int mraft_debug_tick_trace(void *dst, long long nbytes) {
  if (nbytes > (long long)sizeof(g_tick_trace)) nbytes = sizeof(g_tick_trace);
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_tick_trace), (size_t)nbytes, 0, hipMemcpyDeviceToHost) ==
                 hipSuccess ? 0 : -3;
}
#endif

void launch_replicate_tick(const Dev &s, const int32_t *lpeer, int32_t *gflags, int32_t *exp_commit,
                           int32_t *exp_term_leader, const uint8_t *reach, hipStream_t st) {
  const Export ex{exp_commit, exp_term_leader};
  // P == 1 sends nothing: its kernel is the same with and without a mask
  if (!reach || !with_peers<2>(s.P, [&](auto pc) {
        hipLaunchKernelGGL((k_tick_group<decltype(pc)::value, false, uint8_t>), dim3(s.G), dim3(64), 0, st, s, lpeer,
                           gflags, (unsigned long long *)nullptr, ex, reach);
      }))
    launch_tick_c<false>(s, lpeer, gflags, nullptr, ex, st);
}

void launch_tick_list(const Dev &s, const int32_t *lpeer, int32_t *gflags, int32_t *exp_commit,
                      int32_t *exp_term_leader, const LiteBufs &lb, const uint8_t *reach, hipStream_t st) {
  with_peers<2>(s.P, [&](auto pc) {
    constexpr int P = decltype(pc)::value;
    const dim3 gr((unsigned)lb.grid), bl(64);
    const Export ex{exp_commit, exp_term_leader};
    if (reach)
      hipLaunchKernelGGL((k_tick_list<P, uint8_t>), gr, bl, 0, st, s, lpeer, gflags, nullptr, ex, lb.list, lb.cnt,
                         lb.cnt_next, lb.hint, lite_cap(s.G), reach);
    else
      hipLaunchKernelGGL((k_tick_list<P>), gr, bl, 0, st, s, lpeer, gflags, nullptr, ex, lb.list, lb.cnt,
                         lb.cnt_next, lb.hint, lite_cap(s.G));
  });
}

void launch_replicate_tick_count(const Dev &s, const int32_t *lpeer, unsigned long long *counts,
                                 hipStream_t st) {
  launch_tick_c<true>(s, lpeer, nullptr, counts, Export{nullptr, nullptr}, st);
}

}  // namespace mraft

MRAFT_BOUNDS_READER(mraft_debug_bounds_tick)
