// mraft_handle_ae.hip — the message-level AppendEntries handler ("a4",
// mraft_handle_append_entries of include/mraft.h) for gfx950: the claims and
// set heads (k_claim_ae) and the main launch (k_handle_set, one set of messages
// per wave through handle_one of mraft_handle_ae.h, where the rules are). The
// deferred launch is mraft_handle_deferred.hip.
#include "mraft_handle_ae.h"

namespace mraft {

namespace {

// The claims of AppendEntries by reference and the set heads, one launch
// (rounds 2-4: a claim kernel, then a plan kernel that classified every item
// and compacted set and deferral lists through contended atomics). Per item:
// the slot check and the claim (atomicMax: the lowest item wins), srcmark of
// the row it reads, and sethd[i] = the size of the set item i heads, else 0
// (keys of the neighbours within kAeHalo from LDS, the halo loaded by the
// wave's edge lanes). Its first threads also arm the counters the main and
// the deferred launch add into (mraft_internal.h kAeCnt*); the previous call's
// deferred launch has read them (stream order).
constexpr int kAeHalo = 7;

__global__ __launch_bounds__(64) void k_claim_ae(const mraft_ae_args *__restrict__ args, int64_t n, int64_t n_log,
                                                 int L, int64_t gp, int ni, unsigned long long *__restrict__ claim,
                                                 uint32_t *__restrict__ srcmark, uint32_t epoch,
                                                 int32_t *__restrict__ err, uint8_t *__restrict__ sethd,
                                                 unsigned long long *__restrict__ total) {
  __shared__ long long kr[64 + 2 * kAeHalo];
  __shared__ int kb[64 + 2 * kAeHalo], ke[64 + 2 * kAeHalo];
  const int t = (int)threadIdx.x;
  const int64_t i = blockIdx.x * (int64_t)64 + t;
  if (i == 0) total[kAeCntFbDone] = 0;
  if (i < kStripes) {
    total[kAeCntDeferred + kAeCntStripe * i] = 0;
    total[kAeCntFbStripeDone + kAeCntStripe * i] = 0;
    total[kAeCntStaged + kAeCntStripe * i] = 0;
  }
  AeKey k{-1, 0, 0};
  if (i < n) {
    const mraft_ae_args a = args[i];
    if (a.slot < 0 || a.slot >= gp) {
      err[i] = MRAFT_ITEM_BAD_SLOT;
    } else {
      err[i] = 0;
      atomicMax(&claim[a.slot], claim_tag(epoch, i));
      k = ae_key(a, gp, n_log, L);
      if (a.n_entries > 0 && k.row >= 0) srcmark[k.row] = epoch;
    }
  }
  kr[kAeHalo + t] = k.row; kb[kAeHalo + t] = k.base; ke[kAeHalo + t] = k.end;
  if (t < kAeHalo || t >= 64 - kAeHalo) {  // the halo: kAeHalo neighbours on either side of the wave
    const int64_t j = t < kAeHalo ? i - kAeHalo : i + kAeHalo;
    AeKey h{-1, 0, 0};
    if (j >= 0 && j < n) h = ae_key(args[j], gp, n_log, L);
    const int slot = t < kAeHalo ? t : t + 2 * kAeHalo;
    kr[slot] = h.row; kb[slot] = h.base; ke[slot] = h.end;
  }
  __syncthreads();
  if (i >= n) return;
  int hd = 0;
  const int c = kAeHalo + t;
  int pos = 0;  // this item's place in its run of same-entry messages (up to ni back)
  if (k.row >= 0)
    for (int d = 1; d <= ni && same_key(k, AeKey{kr[c - d], kb[c - d], ke[c - d]}); ++d) ++pos;
  if (k.row < 0 || pos >= ni) {
    hd = 1;
  } else if (pos == 0) {
    hd = 1;  // the set's size (up to ni forward)
    for (int d = 1; d < ni && same_key(k, AeKey{kr[c + d], kb[c + d], ke[c + d]}); ++d) ++hd;
  }
  sethd[i] = (uint8_t)hd;
}

// The main launch: wave v serves the sets whose heads lie in items
// [v*NI, (v+1)*NI) (one set for a gathered batch), each XCD a contiguous
// range of waves (neighbouring sets share one L2 for the leaders' entries).
// HM_HOST: wave v serves message v.
template <int NI, int MODE>
__global__ __launch_bounds__(64, MRAFT_AE_MINW) void k_handle_set(HsArgs ka) {
  const int64_t nb = MODE == HM_HOST ? ka.n : (ka.n + NI - 1) / NI;
  int64_t v = blockIdx.x;
  {
    const int64_t x = v & 7, per = nb >> 3, rem = nb & 7;
    if ((v >> 3) >= per + (x < rem ? 1 : 0)) return;
    v = xcd_contiguous(v, nb);
  }
  if (MODE == HM_HOST) {
    handle_one<NI, HM_HOST>(ka, v, 1);
    return;
  }
  const int lane = lane_id();
  const int64_t c0 = v * NI;
  const int hd = (lane < NI && c0 + lane < ka.n) ? (int)ka.sethd[c0 + lane] : 0;
  for (unsigned long long m = __ballot(hd > 0); m; m &= m - 1) {
    const int q = first_lane(m);
    handle_one<NI, HM_MAIN>(ka, c0 + q, __builtin_amdgcn_readlane(hd, q));
  }
}

}  // namespace

void launch_claim_ae(const mraft_ae_args *args, int64_t n, int64_t n_log, int L, int64_t gp, int ni,
                     unsigned long long *claim, uint32_t *srcmark, uint32_t epoch, int32_t *err, uint8_t *sethd,
                     unsigned long long *total, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_claim_ae, dim3(blocks_for(n, 64)), dim3(64), 0, st, args, n, n_log, L, gp,
                     ni < 1 ? 1 : ni > kAeHalo ? kAeHalo : ni, claim, srcmark, epoch, err, sethd, total);
}

// grid for k_handle_set: nb waves, each XCD a contiguous range (k_handle_set)
template <int NI, int MODE>
static void launch_set(const HsArgs &ka, int64_t nb, hipStream_t st) {
  hipLaunchKernelGGL((k_handle_set<NI, MODE>), dim3((unsigned)nb), dim3(64), 0, st, ka);
}

template <int NI>
static void launch_main(const HsArgs &ka, hipStream_t st) {
  launch_set<NI, HM_MAIN>(ka, (ka.n + NI - 1) / NI, st);
}

void launch_handle_ae_ref(const HsArgs &ka, int ni, int grid, hipStream_t st) {
  if (ka.n <= 0) return;
  switch (ni) {
    case 1: launch_main<1>(ka, st); break;
    case 2: launch_main<2>(ka, st); break;
    case 3: launch_main<3>(ka, st); break;
    case 4: launch_main<4>(ka, st); break;
    case 5: launch_main<5>(ka, st); break;
    case 6: launch_main<6>(ka, st); break;
    default: launch_main<7>(ka, st);
  }
  launch_handle_deferred(ka, grid, st);
}

void launch_handle_ae_host(const Dev &s, const mraft_ae_args *args, int64_t n, const int32_t *ent, int64_t n_ent,
                           mraft_ae_reply *rep, int32_t *err, mraft_ae_result *res, hipStream_t st) {
  if (n <= 0) return;
  HsArgs ka{};
  ka.s = s; ka.args = args; ka.n = n; ka.ent0 = ent; ka.n_ent0 = n_ent; ka.rep = rep; ka.err = err; ka.res = res;
  launch_set<1, HM_HOST>(ka, n, st);
}

}  // namespace mraft

MRAFT_BOUNDS_READER(mraft_debug_bounds_kernels)
