// mraft_abi_timers.hip — the device-resident timers' entry points
// (include/mraft.h "timers"): enable and disable, load and store, arm, the
// ticker, the notes, and the one-call clock step.
#include "mraft_engine.h"
#include "mraft_timer_draw.h"

using namespace mraft::host;

namespace {

int check_now(int32_t now) {
  if (now < 0 || now > mraft::kTimerNowMax) return fail(MRAFT_E_INVAL, "now = %d outside [0, 2^30]", now);
  return MRAFT_OK;
}

// Every timer call but enable: a usable handle (enter) with timers enabled.
int enter_timers(mraft_engine *h) {
  TRY(enter(h));
  if (!h->tm_ed) return fail(MRAFT_E_NOSTATE, "timers are not enabled (mraft_timers_enable)");
  return MRAFT_OK;
}

mraft::TimerDev timers_of(const mraft_engine *h) { return mraft::TimerDev{h->tm_ed, h->tm_hd, h->tcfg}; }

}  // namespace

extern "C" {

int mraft_timers_enable(mraft_engine *h, const mraft_timer_config *cfg, int32_t now) {
  TRY(enter(h));
  if (!cfg) return fail(MRAFT_E_INVAL, "cfg is null");
  if (!mraft::timer_config_ok(*cfg))
    return fail(MRAFT_E_INVAL,
                "bad timer configuration heartbeat=%d election=[%d, %d) (need 1 <= heartbeat < 2^30, "
                "1 <= election_lo < election_hi <= 2^20)",
                cfg->heartbeat, cfg->election_lo, cfg->election_hi);
  TRY(check_now(now));
  // The arrays reach the handle only when both allocations and the arming
  // launch succeeded; until then they are locals, freed on failure. A second
  // enable re-arms the arrays the handle already has.
  int32_t *ed = h->tm_ed, *hd = h->tm_hd;
  const bool fresh = !h->tm_ed;
  if (fresh) {
    TRY(alloc_async(h, &ed, (size_t)gp_of(h), "election_due"));
    const int rc = alloc_async(h, &hd, (size_t)gp_of(h), "heartbeat_due");
    if (rc) {
      (void)hipFreeAsync(ed, h->stream);
      return rc;
    }
  }
  mraft::launch_timers_arm_all(mraft::TimerDev{ed, hd, *cfg}, gp_of(h), now, h->stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    if (fresh) {
      (void)hipFreeAsync(ed, h->stream);
      (void)hipFreeAsync(hd, h->stream);
    }
    return fail(MRAFT_E_HIP, "arming the timers failed: %s", hipGetErrorString(e));
  }
  h->tm_ed = ed;
  h->tm_hd = hd;
  h->tcfg = *cfg;
  return MRAFT_OK;
}

int mraft_timers_disable(mraft_engine *h) {
  TRY(enter_timers(h));
  for (int32_t **p : {&h->tm_ed, &h->tm_hd}) {
    if (*p) (void)hipFreeAsync(*p, h->stream);  // after the work already enqueued
    *p = nullptr;
  }
  return MRAFT_OK;
}

int mraft_timers_load(mraft_engine *h, const mraft_timers_soa *src, int32_t where) {
  TRY(enter_timers(h));
  if (!src) return fail(MRAFT_E_INVAL, "src is null");
  const size_t b = (size_t)gp_of(h) * sizeof(int32_t);
  TRY(copy_array(h, true, h->tm_ed, src->election_due, b, where));
  TRY(copy_array(h, true, h->tm_hd, src->heartbeat_due, b, where));
  return finish_copies(h, where);
}

int mraft_timers_store(mraft_engine *h, const mraft_timers_soa *dst, int32_t where) {
  TRY(enter_timers(h));
  if (!dst) return fail(MRAFT_E_INVAL, "dst is null");
  const size_t b = (size_t)gp_of(h) * sizeof(int32_t);
  TRY(copy_array(h, false, h->tm_ed, dst->election_due, b, where));
  TRY(copy_array(h, false, h->tm_hd, dst->heartbeat_due, b, where));
  return finish_copies(h, where);
}

int mraft_timers_arm(mraft_engine *h, const int32_t *slots, int64_t n, int32_t now, int32_t where) {
  TRY(enter_timers(h));
  if (n < 0 || (n > 0 && !slots)) return fail(MRAFT_E_INVAL, "null argument");
  TRY(check_now(now));
  if (n == 0) return MRAFT_OK;
  Stage sg(h, where);
  const int32_t *s = sg.in(slots, n);
  TRY(sg.status());
  mraft::launch_timers_arm(timers_of(h), s, n, gp_of(h), now, h->stream);
  return sg.finish();
}

int mraft_ticker(mraft_engine *h, int32_t now, int32_t *out_election_slots, int64_t cap_e, int64_t *out_n_e,
                 int32_t *out_heartbeat_slots, int64_t cap_h, int64_t *out_n_h, int32_t where) {
  TRY(enter_timers(h));
  if (cap_e < 0 || cap_h < 0 || !out_n_e || !out_n_h || (cap_e > 0 && !out_election_slots) ||
      (cap_h > 0 && !out_heartbeat_slots))
    return fail(MRAFT_E_INVAL, "null argument");
  TRY(check_now(now));
  // no list is longer than G*P: a larger buffer is used up to that
  cap_e = std::min<int64_t>(cap_e, gp_of(h));
  cap_h = std::min<int64_t>(cap_h, gp_of(h));
  Stage sg(h, where);
  int32_t *oe = sg.out(cap_e ? out_election_slots : nullptr, cap_e);
  int32_t *oh = sg.out(cap_h ? out_heartbeat_slots : nullptr, cap_h), *bc;
  int64_t *ne = sg.out(out_n_e, 1), *nh = sg.out(out_n_h, 1);
  TRY(sg.status());
  TRY(scratch(h, kScrTickerCnt, 2 * (size_t)mraft::ticker_blocks(gp_of(h)), &bc));
  mraft::launch_ticker(dev_of(h), timers_of(h), now, bc, oe, cap_e, ne, oh, cap_h, nh, h->stream);
  return sg.finish();
}

int mraft_timers_note(mraft_engine *h, int32_t kind, const void *records, const void *outcome,
                      const int32_t *item_err, int64_t n, int32_t now, int32_t where) {
  TRY(enter_timers(h));
  size_t rb = 0, ob = sizeof(int32_t);
  switch (kind) {
    case MRAFT_NOTE_AE_HANDLED: rb = sizeof(mraft_ae_args); ob = sizeof(mraft_ae_reply); break;
    case MRAFT_NOTE_IS_HANDLED: rb = sizeof(mraft_is_args); ob = sizeof(mraft_is_reply); break;
    case MRAFT_NOTE_RV_HANDLED: rb = sizeof(mraft_rv_args); ob = sizeof(mraft_rv_reply); break;
    case MRAFT_NOTE_AE_FOLDED: rb = sizeof(mraft_ae_result); break;
    case MRAFT_NOTE_IS_FOLDED: rb = sizeof(mraft_is_result); break;
    case MRAFT_NOTE_RV_FOLDED: rb = sizeof(mraft_rv_result); break;
    default: return fail(MRAFT_E_INVAL, "note kind %d", kind);
  }
  if (n < 0 || (n > 0 && (!records || !outcome))) return fail(MRAFT_E_INVAL, "null argument");
  TRY(check_now(now));
  if (n == 0) return MRAFT_OK;
  Stage sg(h, where);
  // records and outcomes of the kind's types: staged as bytes
  const char *r = sg.in((const char *)records, rb * (size_t)n), *o = sg.in((const char *)outcome, ob * (size_t)n);
  const int32_t *e = sg.in(item_err, n);
  TRY(sg.status());
  mraft::launch_timers_note(timers_of(h), kind, r, o, e, n, gp_of(h), now, h->stream);
  return sg.finish();
}

int mraft_clock_step(mraft_engine *h, int32_t now, uint32_t flags, uint8_t *cand_mask, int32_t *leader_peer,
                     int32_t *election_flags, int32_t *group_flags, int32_t *commit, int32_t *term_leader,
                     int32_t where) {
  TRY(enter_timers(h));
  if (flags & ~(uint32_t)MRAFT_CLOCK_SEND_ALL) return fail(MRAFT_E_INVAL, "unknown flags 0x%x", flags);
  TRY(check_now(now));
  Stage sg(h, where);
  const size_t G = (size_t)h->G;
  // the words one launch hands to the next live in the caller's buffer when
  // there is one, in the engine's scratch otherwise
  int32_t *need[4], *tg;
  int32_t *const outs[4] = {leader_peer, group_flags, commit, term_leader};
  const ScratchSlot slots[4] = {kScrClockLp, kScrClockGf, kScrClockCommit, kScrClockTl};
  for (int k = 0; k < 4; ++k) {
    if (outs[k])
      need[k] = sg.out(outs[k], G);
    else
      TRY(scratch(h, slots[k], G, &need[k]));
    TRY(sg.status());
  }
  uint8_t *cm = sg.out(cand_mask, G);
  int32_t *ef = sg.out(election_flags, G);
  TRY(sg.status());
  TRY(scratch(h, kScrClockTg, G, &tg));
  int32_t *lp = need[0], *gf = need[1];
  const mraft::TimerDev t = timers_of(h);
  // A-C: ticker, one election round, the sender (every launch of the step
  // under the reachability mask, when one is set)
  mraft::launch_clock_round(dev_of(h), t, now, flags, cm, lp, tg, ef, h->reach, h->stream);
  // D: the tick, under the handle's mode and shards
  TRY(launch_tick(h, lp, gf, need[2], need[3]));
  // E: the tick's resets, on the engine stream after every shard (a
  // device-side wait)
  TRY(join_shards(h));
  mraft::launch_clock_resets(dev_of(h), t, now, gf, lp, tg, h->reach, h->stream);
  return sg.finish();
}

}  // extern "C"
