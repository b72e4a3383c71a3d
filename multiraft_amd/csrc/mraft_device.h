// mraft_device.h — device-side building blocks shared by the gfx950 kernels.
//
// The replica state every kernel takes (Dev), the log ring (ring, term_at),
// mark_persist, and the 64-lane wave's helpers (lane_id, first_lane, uni,
// wave_sum), then its wave-cooperative primitives over a ring row:
//  * wave_scan_down (wave_scan_down_ne / wave_scan_down_eq) — the highest
//    Index of a range whose term differs from / equals a value, 64·U terms
//    per iteration (U coalesced dword loads per lane in flight), found by
//    ballot + find-first-set (the ConflictIndex scan; the term gate of
//    advanceCommitIndexForLeader, raft_append_entry.go:89-105);
//  * wave_conflict_scan — the ConflictIndex backward scan of :136-142;
//  * wave_copy — a streaming copy into a replica's log (restore);
//  * wave_copy_from_ring — a ring row unrolled into a flat buffer
//    (persistence read-out, staged entries);
//  * wave_terms_sorted — whether a row's terms never decrease;
// the optional reachability mask of a kernel (reach_given, reach_byte),
// and for whole grids xcd_contiguous (each XCD a contiguous range of the
// workgroups) and compact_count / compact_offsets, the in-block part of an
// ordered compaction of K lists (the compacted applier, the ticker). The
// rules of single items (claims, Start, the Index domain) are in mraft_rules.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mraft {

constexpr int kLeader = 1, kCandidate = 2, kFollower = 3;  // raft_rpc.go:8-12
constexpr int kWave = 64;
constexpr int kUnroll = 4;                 // loads in flight per lane per stream
constexpr int kChunk = kWave * kUnroll;    // terms per wave iteration

struct Dev {
  int32_t *term, *voted, *role, *commit, *applied, *dummy, *last, *votes;
  int32_t *log, *match, *next;
  int32_t *pdirty;  // persist_dirty (include/mraft.h MRAFT_PERSIST_*); may be null
  int32_t *head;    // log_head: ring position of each replica's dummy entry
  int32_t *hsnap;   // has_snapshot (raft.go:158): set by an installing InstallSnapshot
  int32_t *srt;     // terms_sorted (include/mraft.h MRAFT_TERMS_SORTED): the terms after the dummy never decrease
  int32_t G, P, L;
};

// The log ring (include/mraft.h): Index i of a replica with dummy d and head h
// lives at row + ring(i - d + h, L). Valid for arguments in [-L, 2L): live
// entries have i - d in [0, L), and the pass's masked-out lanes stay within
// one row length of them.
__device__ __forceinline__ int ring(int k, int L) {
  k = k >= L ? k - L : k;
  return k < 0 ? k + L : k;
}

// Term of Index i of replica `slot` (dummy d, head h).
__device__ __forceinline__ int term_at(const Dev &s, int64_t slot, int d, int h, int i) {
  return s.log[slot * s.L + ring(i - d + h, s.L)];
}

// Records a persist() / SaveStateAndSnapshot() call site of the reference for
// replica `slot` (one writer per slot per launch).
__device__ __forceinline__ void mark_persist(const Dev &s, int64_t slot, int bits) {
  if (s.pdirty && bits) s.pdirty[slot] |= bits;
}

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

__device__ __forceinline__ int first_lane(unsigned long long m) { return __ffsll((long long)m) - 1; }

// A value every lane of the wave holds alike, in an SGPR.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The downward term scan: the largest idx in [lo, hi] whose term equals a
// (EQ) or differs from it (!EQ), in a ring row whose Index `base` (the dummy)
// sits at `head` (row length L); lo - 1 when no term of the range does.
// 64·U terms per iteration (U coalesced dword loads per lane in flight),
// found by ballot + find-first-set. Wave-uniform arguments; the term of lo
// must be readable when lo <= hi (lanes past lo re-read it).
template <bool EQ, int U>
__device__ __forceinline__ int wave_scan_down(const int32_t *__restrict__ row, int base, int head, int L,
                                              int lo, int hi, int a) {
  const int lane = lane_id();
  for (int top = hi; top >= lo; top -= kWave * U) {
    int v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = top - lane - kWave * u;
      const int w = row[ring(max(idx, lo) - base + head, L)];  // unconditional: the U loads issue back to back
      v[u] = idx >= lo ? w : EQ ? a + 1 : a;                   // past lo: a term that does not count
    }
    // Every ballot, no exit per vector (which lets the compiler sink each load
    // behind the previous compare: one round trip per 64 terms).
    int r = lo - 1;
#pragma unroll
    for (int u = U - 1; u >= 0; --u) {
      const unsigned long long m = __ballot(EQ ? v[u] == a : v[u] != a);
      r = m ? top - kWave * u - first_lane(m) : r;
    }
    if (r >= lo) return r;
  }
  return lo - 1;
}

// Its two uses by name: the ConflictIndex scan (term differs), and the term
// gate of advanceCommitIndexForLeader (term equals; a1 of the reply fold).
template <int U = kUnroll>
__device__ __forceinline__ int wave_scan_down_ne(const int32_t *__restrict__ row, int base, int head,
                                                 int L, int lo, int hi, int a) {
  return wave_scan_down<false, U>(row, base, head, L, lo, hi, a);
}
template <int U = kUnroll>
__device__ __forceinline__ int wave_scan_down_eq(const int32_t *__restrict__ row, int base, int head,
                                                 int L, int lo, int hi, int a) {
  return wave_scan_down<true, U>(row, base, head, L, lo, hi, a);
}

// ConflictIndex of raft_append_entry.go:136-142 for prev > dummy + 1, where
// a = term(prev): the largest index in [dummy+2, prev-1] whose term differs
// from a, else dummy + 1. The first probe reads one term per lane (64 terms:
// most runs end there), then 256-term iterations.
__device__ __forceinline__ int wave_conflict_scan(const int32_t *__restrict__ frow, int fdummy, int fhead,
                                                  int L, int prev, int a) {
  const int lo = fdummy + 2, hi = prev - 1;
  const int idx = hi - lane_id();
  const int v = idx >= lo ? frow[ring(idx - fdummy + fhead, L)] : a;
  const unsigned long long m = __ballot(v != a);
  if (m) return hi - first_lane(m);
  if (hi - 64 < lo) return fdummy + 1;
  const int r = wave_scan_down_ne(frow, fdummy, fhead, L, lo, hi - 64, a);
  return r < lo ? fdummy + 1 : r;
}

// F[k] = E[k] for k in [0, cnt).
__device__ __forceinline__ void wave_copy(const int32_t *__restrict__ E, int32_t *__restrict__ F,
                                          int cnt) {
  const int lane = lane_id();
  for (int base = 0; base < cnt; base += kChunk) {
    int v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      int k = base + lane + kWave * u;
      v[u] = k < cnt ? E[k] : 0;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      int k = base + lane + kWave * u;
      if (k < cnt) F[k] = v[u];
    }
  }
}

// n terms of a ring row from Index `from` (dummy `base` at `head`) into dst,
// in order: the ring unrolled (persistence read-out, staged entries).
__device__ __forceinline__ void wave_copy_from_ring(const int32_t *__restrict__ row, int base, int head,
                                                    int L, int from, int32_t *__restrict__ dst, int cnt) {
  const int lane = lane_id();
  for (int b = 0; b < cnt; b += kChunk) {
    int v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int k = b + lane + kWave * u;
      v[u] = k < cnt ? row[ring(from + k - base + head, L)] : 0;
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int k = b + lane + kWave * u;
      if (k < cnt) dst[k] = v[u];
    }
  }
}

// Whether the terms of Index [lo, hi] of a ring row (dummy `base` at `head`)
// never decrease (wave-cooperative; terms_sorted, include/mraft.h). Not on a
// hot path: load_state and restore only.
__device__ __forceinline__ bool wave_terms_sorted(const int32_t *__restrict__ row, int base, int head, int L,
                                                  int lo, int hi) {
  // (offsets from lo: an Index loop `b += 64` would overflow int32 within 64
  // of 2^31 - 1, include/mraft.h's Index domain)
  for (int d = 0; d < hi - lo; d += kWave) {
    const int k = d + lane_id();  // Index lo + k
    const bool bad = k < hi - lo && row[ring(lo + k - base + head, L)] > row[ring(lo + k + 1 - base + head, L)];
    if (__ballot(bad)) return false;
  }
  return true;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Workgroups are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md
// §Workgroup dispatch). The index workgroup b of nb takes so that each XCD
// serves one contiguous range (the first nb % 8 XCDs one workgroup more): a
// permutation of [0, nb), for speed only.
template <typename T>
__device__ __forceinline__ T xcd_contiguous(T b, T nb) {
  const T x = b & 7, per = nb >> 3, rem = nb & 7;
  return x * per + min(x, rem) + (b >> 3);
}

// ---------------------------------------------------------------- reachability mask
// Convention: a kernel that can run under a reachability mask
// (mraft_set_reachable) takes as its last parameter a pack of no pointer or
// one, `const M *__restrict__... reach`: empty, the kernel is the unmasked one;
// M = uint8_t, it reads the groups' reachability bytes.
template <class... M>
constexpr bool reach_given() {
  static_assert(sizeof...(M) <= 1, "the reachability pack holds no pointer or one");
  return sizeof...(M) == 1;
}

// Group g's reachability word (bit p: replica p is connected): the constant
// all-ones without a mask, so every test of it compiles away.
__device__ __forceinline__ int reach_byte(int) { return -1; }
__device__ __forceinline__ int reach_byte(int g, const uint8_t *m) { return (int)m[g]; }

// ---------------------------------------------------------------- ordered compaction
// K lists of the items that satisfy K predicates, each in ascending item
// order, from workgroups of kCompactBlock threads, a thread per item: a count
// launch (compact_count), an exclusive scan of the block counts
// (launch_compact_scan, mraft_internal.h), an emit launch (compact_offsets).
// List k's block counts, then offsets, are bcnt[k * nb + block].
constexpr int kCompactBlock = 256, kCompactWaves = kCompactBlock / kWave;

// The wave's ballots m and, after a barrier, every wave's counts wc.
template <int K>
__device__ __forceinline__ void compact_ballots(const bool (&pred)[K], unsigned long long (&m)[K],
                                                int (&wc)[K][kCompactWaves]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    m[k] = __ballot(pred[k]);
    if (lane_id() == 0) wc[k][threadIdx.x >> 6] = __popcll(m[k]);
  }
  __syncthreads();
}

// Count launch, every thread: the workgroup's count of each list.
template <int K>
__device__ __forceinline__ void compact_count(const bool (&pred)[K], int32_t *__restrict__ bcnt, int64_t nb) {
  __shared__ int wc[K][kCompactWaves];
  unsigned long long m[K];
  compact_ballots<K>(pred, m, wc);
  const int k = threadIdx.x;
  if (k < K) bcnt[k * nb + blockIdx.x] = wc[k][0] + wc[k][1] + wc[k][2] + wc[k][3];
}

// Emit launch, every thread: off[k] = its position in list k where pred[k]
// holds (the scanned block offset, the waves below, the lanes below).
template <int K>
__device__ __forceinline__ void compact_offsets(const bool (&pred)[K], const int32_t *__restrict__ boff, int64_t nb,
                                                int64_t (&off)[K]) {
  __shared__ int wc[K][kCompactWaves];
  unsigned long long m[K];
  compact_ballots<K>(pred, m, wc);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    off[k] = boff[k * nb + blockIdx.x] + __popcll(m[k] & ((1ull << lane_id()) - 1));
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off[k] += wc[k][w];
  }
}

}  // namespace mraft
