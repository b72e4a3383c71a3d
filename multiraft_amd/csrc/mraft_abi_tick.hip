// mraft_abi_tick.hip — the tick's entry points (include/mraft.h) and its
// launch policy: full, light or automatic per shard, one launch on the engine
// stream or one per tick shard on the shard's own queue.
#include "mraft_engine.h"

using namespace mraft::host;

namespace {

int32_t *off(int32_t *p, int64_t k) { return p ? p + k : nullptr; }

// The light tick's buffers (MRAFT_TICK_LIGHT), allocated on first use,
// stream-ordered, counters zeroed.
int ensure_lite(mraft_engine *h) {
  if (h->lite_list) return MRAFT_OK;
  TRY(alloc_async(h, &h->lite_list, (size_t)mraft::lite_list_alloc_words(h->G, kMaxShards), "light tick list"));
  TRY(alloc_async(h, &h->lite_cnt, (size_t)2 * kMaxShards * mraft::kLiteCntWords, "light tick counters", true));
  for (int s = 0; s < kMaxShards; ++s) h->lite_par[s] = 0;
  return MRAFT_OK;
}

// MRAFT_TICK_AUTO's choice for shard s of G_s groups: the light tick while
// the last completed light tick sent at most a quarter of the groups to the
// full tick (or none has completed yet); otherwise the full tick, with a
// light tick every kAutoProbe-th tick to measure again.
bool auto_light(mraft_engine *h, int s, int32_t gs) {
  const long long last = hint(h, kHintLite + s);
  if (last < 0 || 4 * last <= (long long)gs) {
    h->auto_since[s] = 0;
    return true;
  }
  if (++h->auto_since[s] >= kAutoProbe) {
    h->auto_since[s] = 0;
    return true;
  }
  return false;
}

// One tick launch over groups [g0, g0 + d.G) as shard s on stream st: the full
// tick, or the light tick's pair of launches.
// sio (mraft_start_and_tick): Start at the range's leaders first — inside the
// light launch, or as its own launch before the full tick.
void tick_range(mraft_engine *h, const mraft::Dev &d, int s, int32_t g0, const int32_t *lp, int32_t *gf,
                int32_t *ec, int32_t *et, hipStream_t st, const mraft::StartIO *sio = nullptr) {
  const bool light = h->P >= 2 && (h->tick_mode == MRAFT_TICK_LIGHT ||
                                   (h->tick_mode == MRAFT_TICK_AUTO && auto_light(h, s, d.G)));
  // the reachability mask (mraft_set_reachable), when one is set: the range's bytes
  const uint8_t *reach = h->reach ? h->reach + g0 : nullptr;
  mraft::StartIO so{};
  if (sio) so = {sio->counts + g0, sio->oi + g0, sio->ot + g0, sio->ol + g0, sio->err + g0};
  if (!light) {
    if (sio) mraft::launch_start_groups(d, lp + g0, so, st);
    mraft::launch_replicate_tick(d, lp + g0, off(gf, g0), off(ec, g0), off(et, g0), reach, st);
    return;
  }
  mraft::LiteBufs lb;
  const int par = h->lite_par[s];
  h->lite_par[s] ^= 1;
  lb.list = h->lite_list + mraft::lite_list_begin(g0, s);
  lb.cnt = h->lite_cnt + (2 * s + par) * mraft::kLiteCntWords;
  lb.cnt_next = h->lite_cnt + (2 * s + (par ^ 1)) * mraft::kLiteCntWords;
  lb.hint = h->dhint_dev + kHintLite + s;
  const long long prev = hint(h, kHintLite + s);
  // no completed light tick yet (e.g. the first ticks enqueued back to back):
  // one wave per SIMD slot, grid-stride
  const long long gr = prev < 0 ? kLiteGridUnknown : std::max(kLiteGridMin, 2 * prev);
  lb.grid = (int)std::max(1ll, std::min(gr, (long long)d.G));
  mraft::launch_replicate_tick_light(d, lp + g0, off(gf, g0), off(ec, g0), off(et, g0), lb, sio ? &so : nullptr,
                                     reach, st);
}

}  // namespace

int mraft::host::launch_tick(mraft_engine *h, const int32_t *lp, int32_t *gf, int32_t *ec, int32_t *et,
                             const mraft::StartIO *sio) {
  if (h->tick_mode != MRAFT_TICK_FULL) TRY(ensure_lite(h));
  if (h->nshards <= 1) {
    tick_range(h, dev_of(h), 0, 0, lp, gf, ec, et, h->stream, sio);
    HIP_TRY(hipGetLastError());
    return MRAFT_OK;
  }
  HIP_TRY(hipEventRecord(h->fork_ev, h->stream));
  for (int s = 0; s < h->nshards; ++s) HIP_TRY(hipStreamWaitEvent(h->shard_q[s], h->fork_ev, 0));
  for (int s = 0; s < h->nshards; ++s) {
    const int32_t g0 = (int32_t)((int64_t)h->G * s / h->nshards), g1 = (int32_t)((int64_t)h->G * (s + 1) / h->nshards);
    if (g1 <= g0) continue;
    tick_range(h, dev_slice(h, g0, g1), s, g0, lp, gf, ec, et, h->shard_q[s], sio);
  }
  h->shards_pending = true;
  HIP_TRY(hipGetLastError());
  return MRAFT_OK;
}

extern "C" {

int mraft_replicate_tick(mraft_engine *h, const int32_t *leader_peer, int32_t *group_flags,
                         int32_t where) {
  TRY(enter_tick(h));
  if (!leader_peer) return fail(MRAFT_E_INVAL, "leader_peer is null");
  Stage sg(h, where);
  const int32_t *lp = sg.in(leader_peer, h->G);
  int32_t *gf = sg.out(group_flags, h->G);
  TRY(sg.status());
  TRY(launch_tick(h, lp, gf, nullptr, nullptr));
  if (where == MRAFT_HOST) TRY(join_shards(h));
  return sg.finish();
}

int mraft_start_and_tick(mraft_engine *h, const int32_t *leader_peer, const int32_t *counts, int32_t *out_index,
                         int32_t *out_term, int32_t *out_is_leader, int32_t *item_err, int32_t *group_flags,
                         int32_t where) {
  TRY(enter_tick(h));
  if (!leader_peer || !counts || !out_index || !out_term || !out_is_leader || !item_err)
    return fail(MRAFT_E_INVAL, "null argument");
  Stage sg(h, where);
  const size_t G = h->G;
  const int32_t *lp = sg.in(leader_peer, G);
  const mraft::StartIO sio{sg.in(counts, G), sg.out(out_index, G), sg.out(out_term, G), sg.out(out_is_leader, G),
                           sg.out(item_err, G)};
  int32_t *gf = sg.out(group_flags, G);
  TRY(sg.status());
  TRY(launch_tick(h, lp, gf, nullptr, nullptr, &sio));
  if (where == MRAFT_HOST) TRY(join_shards(h));
  return sg.finish();
}

int mraft_replicate_tick_export(mraft_engine *h, const int32_t *leader_peer, int32_t *group_flags,
                                int32_t *commit, int32_t *term_leader, int32_t where) {
  TRY(enter_tick(h));
  if (!leader_peer || !commit || !term_leader) return fail(MRAFT_E_INVAL, "null argument");
  Stage sg(h, where);
  const int32_t *lp = sg.in(leader_peer, h->G);
  int32_t *gf = sg.out(group_flags, h->G), *c = sg.out(commit, h->G), *t = sg.out(term_leader, h->G);
  TRY(sg.status());
  TRY(launch_tick(h, lp, gf, c, t));
  if (where == MRAFT_HOST) TRY(join_shards(h));
  return sg.finish();
}

int mraft_replicate_tick_count(mraft_engine *h, const int32_t *leader_peer, int64_t out_words[3],
                               int32_t where) {
  TRY(enter(h));
  if (!leader_peer || !out_words) return fail(MRAFT_E_INVAL, "null argument");
  if (h->reach)
    return fail(MRAFT_E_INVAL, "the word count is defined for the full network only: a reachability mask is set");
  Stage sg(h, where);
  const int32_t *lp = sg.in(leader_peer, h->G);
  TRY(sg.status());
  constexpr size_t cw = (size_t)mraft::kCountStripes * mraft::kCountWords;
  unsigned long long *cnt;
  TRY(scratch(h, kScrTickCount, cw, &cnt));
  HIP_TRY(hipMemsetAsync(cnt, 0, cw * sizeof *cnt, h->stream));
  mraft::launch_replicate_tick_count(dev_of(h), lp, cnt, h->stream);
  HIP_TRY(hipGetLastError());
  unsigned long long hc[cw];
  HIP_TRY(hipMemcpyAsync(hc, cnt, sizeof hc, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int i = 0; i < 3; ++i) {
    unsigned long long t = 0;
    for (int x = 0; x < mraft::kCountStripes; ++x) t += hc[(size_t)x * mraft::kCountWords + i];
    out_words[i] = (int64_t)t;
  }
  return MRAFT_OK;
}

int mraft_set_tick_mode(mraft_engine *h, int32_t mode) {
  TRY(enter_handle(h));
  if (mode != MRAFT_TICK_FULL && mode != MRAFT_TICK_LIGHT && mode != MRAFT_TICK_AUTO)
    return fail(MRAFT_E_INVAL, "tick mode %d", mode);
  h->tick_mode = mode;
  return MRAFT_OK;
}

int32_t mraft_get_tick_mode(const mraft_engine *h) { return h ? h->tick_mode : -1; }

int64_t mraft_tick_light_fallbacks(mraft_engine *h) {
  if (!h) return -1;
  long long t = 0;
  for (int s = 0; s < std::max(1, (int)h->nshards); ++s) {
    const long long v = hint(h, kHintLite + s);
    if (v < 0) return -1;
    t += v;
  }
  return t;
}

}  // extern "C"
