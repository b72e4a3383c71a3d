// mraft_handle_deferred.hip — the deferred launch of the message-level
// AppendEntries handler (k_handle_deferred: the `written` items of
// mraft_handle_ae.h "a4", after the main launch of mraft_handle_ae.hip) for
// gfx950, with its ordered fallback.
#include "mraft_handle_ae.h"

namespace mraft {

namespace {

// ---- The deferred launch's fallback: the staged words exceed the stage
// capacity, so deferred items that are also `read` have no staged copy and
// must run in an order (round 6; rounds 4-5 ran the whole fallback on one
// wave). Edge x -> wr[x]: x reads the row its writer wr[x] rewrites, so x runs
// first. Each item has one writer at most, so the graph is trees feeding
// chains that end at an item with no writer or at a cycle. Every workgroup
// takes deferred items grid-stride and nothing ever waits:
//  * an item no deferred item reads (kin 0) starts a chain: it runs, then
//    counts itself at its writer (arr); the reader that completes the
//    writer's count (arr == kin) runs the writer next, and so on;
//  * a cycle of at most kCycWalk items (found by walking wr) runs as a unit
//    on one wave, once every tree feeding it has run: its smallest item's
//    entries are copied to the wave's cycle buffer first, then the members
//    run around the cycle from its writer, that item last from the copy.
//    Readiness is one counter at that item (cpend): each member whose other
//    readers have all run adds 1 (the reader whose arrival leaves only the
//    cycle predecessor missing, arr == kin - 1), and the smallest item's own
//    visit adds kBig - F (F: members with such readers): the add that brings
//    it to kBig runs the cycle;
//  * what is left — cycles longer than the walk, or completed on a workgroup
//    with no cycle buffer — the last workgroup to finish runs one cycle at a
//    time through the L-word buffer (every tree has run by then).
// Nothing another item reads is written before that item has read it; items
// of a chain share no row they both read and write, so the hand-offs need no
// fence beyond the counters' atomics (the runs of a cycle are ordered on one
// wave). Same results as the staged path (tests/test_handler_async.py,
// tests/test_deferred_graphs_gpu.py).
constexpr int kCycWalk = 32;
constexpr unsigned kCycBig = 1u << 30;  // > kCycWalk: the count cannot reach it early

__device__ __forceinline__ int32_t &fb_dn(const HsArgs &k, int64_t x) { return reinterpret_cast<int32_t *>(k.fb + x)[2]; }

// One deferred item in the fallback: its entries in place (buf null) or from
// buf (its copy); then marked run.
__device__ __forceinline__ void fb_run(const HsArgs &k, int64_t x, int32_t *buf) {
  HsArgs kx = k;
  kx.stage = buf;
  kx.stage_cap = k.s.L;
  handle_one<1, HM_ORDER>(kx, x, 1, buf ? 0 : -2);
  if (lane_id() == 0) at_store(&fb_dn(k, x), 1);
}

// x's writer: the claimant of the row x reads when that claimant is a
// well-formed reference (then its slot, read by x, made it deferred too).
__device__ __forceinline__ int64_t fb_writer(const HsArgs &k, int64_t x) {
  const int w = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int32_t *>(k.fb + x)[0]);
  if (w < 0 || (int64_t)w >= k.n) return -1;
  const int L = k.s.L;
  return ae_ref_ok(k.args[w], (int64_t)k.s.G * k.s.P * L, L) ? (int64_t)w : -1;
}

// Whether y lies on a cycle of at most kCycWalk items; then its smallest item
// and length.
__device__ __forceinline__ bool fb_short_cycle(const HsArgs &k, int64_t y, int64_t *least, int *len) {
  int64_t z = y, m = y;
  for (int st = 1; st <= kCycWalk; ++st) {
    z = fb_writer(k, z);
    if (z < 0) return false;
    if (z == y) {
      *least = m;
      *len = st;
      return true;
    }
    m = min(m, z);
  }
  return false;
}

// A cycle whose feeding trees have all run, from its smallest item b: b's
// entries (the pristine row of its writer) copied first, then the members
// from b's writer round to b. With no cycle buffer for this workgroup the
// cycle is left to the last workgroup.
__device__ __forceinline__ void fb_run_cycle(const HsArgs &k, int64_t b) {
  if ((int)blockIdx.x >= k.nslot) return;
  int32_t *buf = k.cslot + (int64_t)blockIdx.x * k.s.L;
  const mraft_ae_args a = k.args[b];
  const int L = k.s.L;
  const int64_t row = a.entries_offset / L;
  wave_copy_from_ring(k.s.log + row * L, 0, k.s.head[row], L, (int)(a.entries_offset % L), buf, a.n_entries);
  wave_fence();  // this wave reads the copy back: a workgroup-scope fence (r6_v9: an agent-scope one per cycle, an L2 write-back each, cost 5 ms per 32k cycles)
  int64_t z = fb_writer(k, b);
  for (int st = 0; z >= 0 && z != b && st < kCycWalk; ++st, z = fb_writer(k, z)) fb_run(k, z, nullptr);
  fb_run(k, b, buf);
}

__device__ __forceinline__ void fb_cycle_add(const HsArgs &k, int64_t b, unsigned add) {
  unsigned old = 0;
  if (lane_id() == 0) old = atomicAdd(reinterpret_cast<unsigned *>(k.fb + b) + 3, add);
  old = (unsigned)__builtin_amdgcn_readfirstlane((int)old);
  if (old + add == kCycBig) fb_run_cycle(k, b);
}

// x, then every writer whose readers x's run completes.
__device__ __forceinline__ void fb_chain(const HsArgs &k, int64_t x) {
  x = ((int64_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
  for (;;) {
    fb_run(k, x, nullptr);
    const int64_t w = fb_writer(k, x);
    if (w < 0) return;
    unsigned a = 0;
    if (lane_id() == 0) a = atomicAdd(reinterpret_cast<unsigned *>(k.fb + w) + 1, 1u) + 1u;
    a = (unsigned)__builtin_amdgcn_readfirstlane((int)a);
    const unsigned kw = (unsigned)tag_count(&k.kin[w], k.epoch);
    if (a == kw) {
      x = w;
      continue;
    }
    int64_t b;
    int len;
    if (a + 1 == kw && fb_short_cycle(k, w, &b, &len)) fb_cycle_add(k, b, 1);
    return;
  }
}

// The deferred items as one sequence j = 0 .. nd - 1 over the stripes' lists
// (stripe x's count d[x], its list at defer[x * n]); wave-uniform counts.
struct DeferSeq {
  int64_t d[kStripes];
  __device__ __forceinline__ int64_t at(const HsArgs &k, int64_t j) const {
    int x = 0;
#pragma unroll
    for (int y = 0; y < kStripes - 1; ++y)
      if (x == y && j >= d[y]) { j -= d[y]; x = y + 1; }
    return k.defer[x * k.n + j];
  }
};

// The last workgroup: every item not yet run lies on a cycle whose feeding
// trees have run; each such cycle runs from one member x through the L-word
// buffer.
__device__ __forceinline__ void fb_leftover(const HsArgs &k, int64_t nd, const DeferSeq &ds) {
  const int lane = lane_id();
  const int L = k.s.L;
  for (int64_t j0 = 0; j0 < nd; j0 += 64) {
    const int64_t j = j0 + lane;
    const int64_t y = j < nd ? ds.at(k, j) : -1;
    for (unsigned long long m = __ballot(y >= 0 && at_load(&fb_dn(k, y)) == 0); m; m &= m - 1) {
      const int q = first_lane(m);
      const int64_t x = ((int64_t)__builtin_amdgcn_readlane((int)(y >> 32), q) << 32) |
                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)y, q);
      if (__builtin_amdgcn_readfirstlane(at_load(&fb_dn(k, x)))) continue;  // run with an earlier one's cycle
      const mraft_ae_args a = k.args[x];
      const int64_t row = a.entries_offset / L;
      if (a.n_entries > 0) wave_copy_from_ring(k.s.log + row * L, 0, k.s.head[row], L, (int)(a.entries_offset % L),
                                               k.cyc, a.n_entries);
      wave_fence();
      int64_t z = fb_writer(k, x);
      for (int64_t st = 0; z >= 0 && z != x && st < nd; ++st) {
        fb_run(k, z, nullptr);
        z = fb_writer(k, z);
      }
      fb_run(k, x, k.cyc);
    }
  }
}

__device__ __forceinline__ void defer_fallback(const HsArgs &k, int64_t nd, const DeferSeq &ds) {
  // only workgroups with a cycle buffer take items (any of them may complete
  // a cycle and must run it: r6_v6 ran 28k of 32k 2-cycles on the last
  // workgroup when the grid was 16x the buffers); the others only count out
  const int64_t nb = min((int64_t)gridDim.x, (int64_t)max(k.nslot, 1));
  if ((int64_t)blockIdx.x >= nb) return;  // (not counted below either)
  for (int64_t j = blockIdx.x; j < nd; j += nb) {
    const int64_t x = ds.at(k, j);
    if (tag_count(&k.kin[x], k.epoch) == 0) {
      fb_chain(k, x);  // no deferred item reads x's row: a chain starts here
    } else {
      int64_t b;
      int len;
      if (fb_short_cycle(k, x, &b, &len) && b == x) {
        // x is its short cycle's smallest item: its visit's share of the count
        int F = 0;
        int64_t z = x;
        for (int st = 0; st < len; ++st) {
          F += tag_count(&k.kin[z], k.epoch) > 1 ? 1 : 0;
          z = fb_writer(k, z);
        }
        fb_cycle_add(k, x, kCycBig - (unsigned)F);
      }
    }
  }
  // the last workgroup to finish runs what is left (it sees every other
  // workgroup's runs: release before each count, acquire after it). Counted
  // in two levels, per stripe (blockIdx % 8, its own line) and then the
  // stripes: one counter taking every workgroup's atomic serialised them
  // (the 2-cycle-heavy batch's fallback, r6_d1)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  int last = 0;
  if (lane_id() == 0) {
    const int64_t x = blockIdx.x & (kStripes - 1);
    const unsigned long long in_x = (unsigned long long)((nb - 1 - x) / kStripes + 1);  // workgroups b < nb, b % 8 == x
    if (atomicAdd(&k.total[kAeCntFbStripeDone + kAeCntStripe * x], 1ull) == in_x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
      last = atomicAdd(&k.total[kAeCntFbDone], 1ull) == (unsigned long long)min(nb, (int64_t)kStripes) - 1;
    }
  }
  if (!__builtin_amdgcn_readfirstlane(last)) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  fb_leftover(k, nd, ds);
}

// The deferred launch: every deferred item (a set of one), grid-stride; the
// counts are read on the device (the host enqueues this launch blind: with no
// deferred item, every workgroup exits at once). Its grid is the host's choice
// from the last call's deferred count, which workgroup 0 publishes to a pinned
// host word when it changes (kAeCntPublished keeps the published value).
__global__ __launch_bounds__(64, MRAFT_AE_DMINW) void k_handle_deferred(HsArgs ka) {
  DeferSeq ds;
  int64_t nd = 0;
  long long smax = 0;  // the largest stripe's staged words
#pragma unroll
  for (int x = 0; x < kStripes; ++x) {
    ds.d[x] = (int64_t)ka.total[kAeCntDeferred + kAeCntStripe * x];
    nd += ds.d[x];
    smax = max(smax, (long long)ka.total[kAeCntStaged + kAeCntStripe * x]);
  }
  const long long cap8 = ka.stage_cap / kStripes;
  // the need, as a stage whose every stripe holds the largest one's words
  const long long staged = smax > cap8 ? smax * kStripes : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && ka.hint && ka.total[kAeCntPublished] != (unsigned long long)nd) {
    ka.total[kAeCntPublished] = (unsigned long long)nd;
    __hip_atomic_store(ka.hint, (long long)nd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // a batch whose staged words exceed the stage: the need, for the host's
  // next call (the stage grows to it under MRAFT_STAGE_AUTO, mraft_abi_msg.hip)
  if (blockIdx.x == 0 && threadIdx.x == 0 && ka.hint && smax > cap8)
    __hip_atomic_store(ka.hint + 1, staged, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (nd == 0) return;
  if (smax <= cap8) {
    for (int64_t j = blockIdx.x; j < nd; j += gridDim.x) handle_one<1, HM_DEFER>(ka, ds.at(ka, j), 1);
  } else {
    defer_fallback(ka, nd, ds);
  }
}

}  // namespace

// Enqueued blind (its counts are on the device), on the host's grid (from the
// last call's deferred count) that grid-strides over the deferred items.
void launch_handle_deferred(const HsArgs &ka, int grid, hipStream_t st) {
  const int64_t g = max((int64_t)1, min(ka.n, (int64_t)grid));
  hipLaunchKernelGGL(k_handle_deferred, dim3((unsigned)g), dim3(64), 0, st, ka);
}

}  // namespace mraft

MRAFT_BOUNDS_READER(mraft_debug_bounds_deferred)
