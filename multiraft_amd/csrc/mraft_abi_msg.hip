// mraft_abi_msg.hip — the message path's entry points (include/mraft.h):
// gather and AppendEntries, the three reply folds, Start, the appliers,
// snapshots, RequestVote and the election rounds, the status export, and
// persistence. Host batches are staged, duplicate slots claimed and the
// kernels launched on the engine stream.
#include <vector>

#include "mraft_engine.h"

using namespace mraft::host;

extern "C" {

int mraft_gather_append_args(mraft_engine *h, const int32_t *slots, const int32_t *peers,
                             int64_t n, mraft_ae_args *out_args, int32_t *item_err, int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!slots || !peers || !out_args || !item_err)))
    return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  Stage sg(h, where);
  const int32_t *s = sg.in(slots, n), *p = sg.in(peers, n);
  mraft_ae_args *o = sg.out(out_args, n);
  int32_t *e = sg.out(item_err, n);
  TRY(sg.status());
  mraft::launch_gather_args(dev_of(h), s, p, n, o, e, h->stream);
  return sg.finish();
}

int mraft_handle_append_entries(mraft_engine *h, const mraft_ae_args *args, int64_t n,
                                const int32_t *entry_terms, int64_t n_entry_terms,
                                mraft_ae_reply *replies, int32_t *item_err, int32_t where) {
  return mraft_handle_append_entries_ex(h, args, n, entry_terms, n_entry_terms, replies, nullptr, item_err, where);
}

int mraft_handle_append_entries_ex(mraft_engine *h, const mraft_ae_args *args, int64_t n,
                                   const int32_t *entry_terms, int64_t n_entry_terms,
                                   mraft_ae_reply *replies, mraft_ae_result *results, int32_t *item_err,
                                   int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!args || !replies || !item_err)))
    return fail(MRAFT_E_INVAL, "null argument");
  // item indices are 32-bit in the claims and the ordered fallback
  if (n > INT32_MAX) return fail(MRAFT_E_INVAL, "n = %lld items exceeds 2^31 - 1", (long long)n);
  if (entry_terms && n_entry_terms < 0) return fail(MRAFT_E_INVAL, "n_entry_terms < 0");
  if (n == 0) return MRAFT_OK;
  TRY(ensure_claim(h));
  Stage sg(h, where);
  const mraft_ae_args *a = sg.in(args, n);
  const int32_t *en = sg.in(entry_terms, entry_terms ? n_entry_terms : 0);
  mraft_ae_reply *r = sg.out(replies, n);
  mraft_ae_result *rs = sg.out(results, n);
  int32_t *e = sg.out(item_err, n);
  TRY(sg.status());
  if (en) {  // entries in a caller buffer: one message per wave, nothing is read while written
    claim(h, a, n, nullptr, e);
    mraft::launch_handle_ae_host(dev_of(h), a, n, en, n_entry_terms, r, e, rs, h->stream);
    return sg.finish();
  }
  // Entries by reference into the engine's log: the claims with the set
  // heads, the main launch, the deferred launch — three launches, every count
  // they need stays on the device, nothing waits on the host (mraft_handle_ae.h
  // "a4" for the rules).
  if (!h->ae_total) TRY(alloc_async(h, &h->ae_total, mraft::kAeTotalWords, "AppendEntries counters", true));
  const size_t nn = (size_t)n;
  mraft::HsArgs ka{};
  ka.s = dev_of(h); ka.args = a; ka.n = n; ka.rep = r; ka.err = e; ka.res = rs;
  ka.total = h->ae_total; ka.claim = h->claim; ka.srcmark = h->srcmark; ka.epoch = h->epoch;
  uint8_t *sethd;
  TRY(scratch(h, kScrAeSoff, nn, &ka.soff));
  TRY(scratch(h, kScrAeSetHead, nn, &sethd));
  ka.sethd = sethd;
  TRY(scratch(h, kScrAeDefer, nn * mraft::kAeStripes, &ka.defer));  // a list of n per stripe
  // the deferred launch's grid: the last call's deferred count (a pinned word
  // the device writes; a stale value only changes the grid, never a result)
  const long long last_nd = hint(h, kHintDeferred);
  const long long gmin = h->defer_grid_min;
  const int grid = (int)(last_nd < gmin ? gmin : last_nd > kDeferGridMax ? kDeferGridMax : last_nd);
  ka.nslot = (int)std::min<int64_t>(grid, std::max<int64_t>(1, kCycSlotWords / h->L));
  // the fallback's per-item records, its L-word buffer and nslot cycle
  // buffers, and its reader counts
  void *order;
  TRY(scratch_bytes(h, kScrAeOrder, mraft::ae_order_carve(ka, nullptr), &order));
  mraft::ae_order_carve(ka, order);
  TRY(scratch_zeroed(h, kScrAeKin, nn, &ka.kin));  // epoch-tagged: a buffer of its own, zeroed when new
  ka.hint = h->dhint_dev;
  // MRAFT_STAGE_AUTO: a batch that exceeded the stage (its need published by
  // the device, kHintStageNeed) grows it for the calls after it (stream-ordered)
  if (h->stage_auto) {
    const long long need = hint(h, kHintStageNeed);
    if (need > h->stage_cap)
      h->stage_cap = std::min<int64_t>((int64_t)INT32_MAX, (need + need / 4 + kStageStep - 1) / kStageStep * kStageStep);
  }
  // the stage: when it cannot be allocated the batch runs with none (every
  // staged item then takes the ordered fallback: the same results, slower);
  // an automatic stage stops growing there
  if (h->stage_cap > 0 && scratch(h, kScrAeStage, (size_t)h->stage_cap, &ka.stage) != MRAFT_OK) {
    ka.stage = nullptr;
    h->stage_auto = false;
  }
  ka.stage_cap = ka.stage ? h->stage_cap : 0;
  const int ni = h->P - 1 < 1 ? 1 : h->P - 1 > 7 ? 7 : h->P - 1;
  const int64_t n_log = gp_of(h) * h->L;
  mraft::launch_claim_ae(a, n, n_log, h->L, gp_of(h), ni, h->claim, h->srcmark, h->epoch, e, sethd, h->ae_total,
                         h->stream);
  mraft::launch_handle_ae_ref(ka, ni, grid, h->stream);
  return sg.finish();
}

int mraft_set_stage_capacity(mraft_engine *h, int64_t words) {
  TRY(enter(h));
  if (words == MRAFT_STAGE_AUTO) {
    h->stage_auto = true;
    return MRAFT_OK;
  }
  if (words < 0 || words > INT32_MAX) return fail(MRAFT_E_INVAL, "stage capacity %lld out of [0, 2^31)", (long long)words);
  h->stage_cap = words;
  h->stage_auto = false;
  return MRAFT_OK;
}

int64_t mraft_get_stage_capacity(const mraft_engine *h) { return h ? h->stage_cap : -1; }

int mraft_process_append_replies(mraft_engine *h, const mraft_ae_result *items, int64_t n,
                                 const int64_t *seg_begin, int64_t n_seg, int32_t *out_flags,
                                 int32_t *item_err, int32_t where) {
  // three launches: the segment claims with the outputs zeroed, the fold
  // (which rejects a segment whose slot another one claimed), the tail (the
  // segments longer than a lane group, and the a1 scans the probes left open)
  return fold_replies(h, items, n, seg_begin, n_seg, out_flags, item_err, where, [=](const FoldBufs<mraft_ae_result> &b) -> int {
    void *sc;
    TRY(scratch_bytes(h, kScrFoldScan, mraft::fold_scan_bytes(n, b.ns), &sc));
    mraft::launch_fold(dev_of(h), b.it, n, b.sb, b.ns, gp_of(h), h->claim, h->epoch, b.se, b.fl, b.e, sc, h->stream);
    return MRAFT_OK;
  });
}

int mraft_start(mraft_engine *h, const int32_t *slots, const int32_t *counts, int64_t n,
                int32_t *out_index, int32_t *out_term, int32_t *out_is_leader, int32_t *item_err,
                int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!slots || !out_index || !out_term || !out_is_leader || !item_err)))
    return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  TRY(ensure_claim(h));
  Stage sg(h, where);
  const int32_t *s = sg.in(slots, n), *c = sg.in(counts, n);
  int32_t *oi = sg.out(out_index, n), *ot = sg.out(out_term, n), *ol = sg.out(out_is_leader, n);
  int32_t *e = sg.out(item_err, n);
  TRY(sg.status());
  mraft::launch_start(dev_of(h), s, c, n, oi, ot, ol, e, h->claim, h->epoch, h->stream);
  return sg.finish();
}

int mraft_collect_apply(mraft_engine *h, int32_t *out_from, int32_t *out_to, int32_t *out_snap_index,
                        int32_t *out_snap_term, int32_t where) {
  TRY(enter(h));
  if (!out_from || !out_to) return fail(MRAFT_E_INVAL, "null argument");
  if (!out_snap_index != !out_snap_term) return fail(MRAFT_E_INVAL, "snapshot outputs: both or neither");
  Stage sg(h, where);
  const size_t gp = (size_t)gp_of(h);
  int32_t *f = sg.out(out_from, gp), *t = sg.out(out_to, gp);
  int32_t *si = sg.out(out_snap_index, gp), *st = sg.out(out_snap_term, gp);
  TRY(sg.status());
  mraft::launch_collect_apply(dev_of(h), f, t, si, st, h->stream);
  return sg.finish();
}

int mraft_collect_apply_compact(mraft_engine *h, int32_t *out_slots, int32_t *out_snap_index,
                                int32_t *out_snap_term, int32_t *out_from, int32_t *out_to, int64_t cap,
                                int64_t *out_n, int32_t where) {
  TRY(enter(h));
  if (cap < 0 || !out_n || (cap > 0 && (!out_slots || !out_from || !out_to)) ||
      (!out_snap_index) != (!out_snap_term))
    return fail(MRAFT_E_INVAL, "null argument");
  Stage sg(h, where);
  int32_t *sl = sg.out(out_slots, cap), *si = sg.out(out_snap_index, cap), *stm = sg.out(out_snap_term, cap);
  int32_t *f = sg.out(out_from, cap), *t = sg.out(out_to, cap), *bc;
  int64_t *total = sg.out(out_n, 1);
  TRY(sg.status());
  TRY(scratch(h, kScrApplyBlocks, (size_t)((gp_of(h) + 255) / 256), &bc));
  mraft::launch_collect_apply_compact(dev_of(h), bc, cap, sl, si, stm, f, t, total, h->stream);
  return sg.finish();
}

int mraft_snapshot(mraft_engine *h, const int32_t *slots, const int32_t *index, int64_t n,
                   int32_t *item_err, int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!slots || !index || !item_err))) return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  TRY(ensure_claim(h));
  Stage sg(h, where);
  const int32_t *s = sg.in(slots, n), *x = sg.in(index, n);
  int32_t *e = sg.out(item_err, n);
  TRY(sg.status());
  claim(h, s, n, nullptr, e);
  mraft::launch_snapshot(dev_of(h), s, x, n, e, h->stream);
  return sg.finish();
}

int mraft_gather_install_snapshot_args(mraft_engine *h, const int32_t *slots, const int32_t *peers,
                                       int64_t n, mraft_is_args *out_args, int32_t *item_err,
                                       int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!slots || !peers || !out_args || !item_err)))
    return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  Stage sg(h, where);
  const int32_t *s = sg.in(slots, n), *p = sg.in(peers, n);
  mraft_is_args *o = sg.out(out_args, n);
  int32_t *e = sg.out(item_err, n);
  TRY(sg.status());
  mraft::launch_gather_is(dev_of(h), s, p, n, o, e, h->stream);
  return sg.finish();
}

int mraft_handle_install_snapshot(mraft_engine *h, const mraft_is_args *args, int64_t n,
                                  mraft_is_reply *replies, int32_t *out_flags, int32_t *item_err,
                                  int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!args || !replies || !out_flags || !item_err)))
    return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  TRY(ensure_claim(h));
  Stage sg(h, where);
  const mraft_is_args *a = sg.in(args, n);
  mraft_is_reply *r = sg.out(replies, n);
  int32_t *f = sg.out(out_flags, n), *e = sg.out(item_err, n);
  TRY(sg.status());
  claim(h, a, n, nullptr, e);
  mraft::launch_handle_is(dev_of(h), a, n, r, f, e, h->stream);
  return sg.finish();
}

int mraft_process_install_snapshot_replies(mraft_engine *h, const mraft_is_result *items, int64_t n,
                                           const int64_t *seg_begin, int64_t n_seg,
                                           int32_t *out_flags, int32_t *item_err, int32_t where) {
  return fold_records(h, items, n, seg_begin, n_seg, out_flags, item_err, where, mraft::launch_process_is);
}

int mraft_start_election(mraft_engine *h, const int32_t *slots, int64_t n, mraft_rv_args *out_args,
                         int32_t *item_err, int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!slots || !out_args || !item_err)))
    return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  TRY(ensure_claim(h));
  Stage sg(h, where);
  const int32_t *s = sg.in(slots, n);
  mraft_rv_args *o = sg.out(out_args, n);
  int32_t *e = sg.out(item_err, n);
  TRY(sg.status());
  claim(h, s, n, nullptr, e);
  mraft::launch_start_election(dev_of(h), s, n, o, e, h->stream);
  return sg.finish();
}

int mraft_handle_request_vote(mraft_engine *h, const mraft_rv_args *args, int64_t n,
                              mraft_rv_reply *replies, int32_t *item_err, int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!args || !replies || !item_err)))
    return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  TRY(ensure_claim(h));
  Stage sg(h, where);
  const mraft_rv_args *a = sg.in(args, n);
  mraft_rv_reply *r = sg.out(replies, n);
  int32_t *e = sg.out(item_err, n);
  TRY(sg.status());
  claim(h, a, n, nullptr, e);
  mraft::launch_handle_rv(dev_of(h), a, n, r, e, h->stream);
  return sg.finish();
}

int mraft_process_vote_replies(mraft_engine *h, const mraft_rv_result *items, int64_t n,
                               const int64_t *seg_begin, int64_t n_seg, int32_t *out_flags,
                               int32_t *item_err, int32_t where) {
  return fold_records(h, items, n, seg_begin, n_seg, out_flags, item_err, where, mraft::launch_tally);
}

int mraft_election_rounds(mraft_engine *h, const uint8_t *cand_mask, int32_t rounds,
                          int32_t *group_flags, int32_t where) {
  TRY(enter(h));
  if (!cand_mask || rounds < 0) return fail(MRAFT_E_INVAL, "null mask or negative rounds");
  Stage sg(h, where);
  const uint8_t *m = sg.in(cand_mask, (size_t)rounds * h->G);
  int32_t *gf = sg.out(group_flags, h->G);
  TRY(sg.status());
  mraft::launch_election_rounds(dev_of(h), m, rounds, gf, h->reach, h->stream);
  return sg.finish();
}

int mraft_export_group_status(mraft_engine *h, const int32_t *leader_peer, int32_t *commit,
                              int32_t *term_leader, int32_t where) {
  TRY(enter(h));
  if (!commit || !term_leader) return fail(MRAFT_E_INVAL, "null argument");
  Stage sg(h, where);
  const int32_t *lp = sg.in(leader_peer, h->G);
  int32_t *c = sg.out(commit, h->G), *t = sg.out(term_leader, h->G);
  TRY(sg.status());
  mraft::launch_export(dev_of(h), lp, c, t, h->stream);
  return sg.finish();
}

// ---------------------------------------------------------------- persistence

int mraft_collect_persist(mraft_engine *h, int32_t *out_bits, int32_t where) {
  TRY(enter(h));
  if (!out_bits) return fail(MRAFT_E_INVAL, "out_bits is null");
  Stage sg(h, where);
  int32_t *o = sg.out(out_bits, (size_t)gp_of(h));
  TRY(sg.status());
  mraft::launch_collect_persist(dev_of(h), o, h->stream);
  return sg.finish();
}

int mraft_read_persistent(mraft_engine *h, const int32_t *slots, int64_t n, mraft_persistent *out,
                          int32_t *out_terms, int64_t terms_cap) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!slots || !out))) return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  for (int64_t i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= gp_of(h)) return fail(MRAFT_E_INVAL, "slot %d out of range", slots[i]);
  int32_t *ds, *dt;
  mraft_persistent *dh;
  TRY(scratch(h, kScrPersistSlots, (size_t)n, &ds));
  TRY(scratch(h, kScrPersistHdr, (size_t)n, &dh));
  HIP_TRY(hipMemcpyAsync(ds, slots, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
  mraft::launch_read_persistent_hdr(dev_of(h), ds, n, dh, h->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, dh, sizeof(mraft_persistent) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  int64_t off = 0;
  for (int64_t i = 0; i < n; ++i) {
    out[i].terms_offset = off;
    off += (int64_t)out[i].last_index - out[i].dummy_index + 1;
  }
  if (!out_terms || terms_cap < off)
    return fail(MRAFT_E_INVAL, "read_persistent: %lld terms needed, capacity %lld", (long long)off,
                (long long)terms_cap);
  TRY(scratch(h, kScrPersistTerms, (size_t)off, &dt));
  HIP_TRY(hipMemcpyAsync(dh, out, sizeof(mraft_persistent) * n, hipMemcpyHostToDevice, h->stream));
  mraft::launch_read_persistent_terms(dev_of(h), dh, n, dt, h->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_terms, dt, sizeof(int32_t) * off, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return MRAFT_OK;
}

int mraft_restore(mraft_engine *h, const mraft_persistent *in, int64_t n, const int32_t *terms,
                  int64_t n_terms, int32_t *item_err) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && (!in || !item_err || (n_terms > 0 && !terms))))
    return fail(MRAFT_E_INVAL, "null argument");
  if (n == 0) return MRAFT_OK;
  std::vector<char> seen((size_t)gp_of(h), 0);
  for (int64_t i = 0; i < n; ++i) {
    const mraft_persistent &r = in[i];
    const int64_t cnt = (int64_t)r.last_index - r.dummy_index + 1;
    int e = MRAFT_ITEM_OK;
    if (r.slot < 0 || r.slot >= gp_of(h) || cnt < 1 || r.dummy_index < 0 || r.terms_offset < 0 ||
        r.terms_offset + cnt > n_terms)
      e = MRAFT_ITEM_BAD_SLOT;
    else if (cnt > h->L)
      e = MRAFT_ITEM_LOG_FULL;
    else if (seen[(size_t)r.slot])
      e = MRAFT_ITEM_DUP_SLOT;
    if (e == MRAFT_ITEM_OK) seen[(size_t)r.slot] = 1;
    item_err[i] = e;
  }
  mraft_persistent *dh;
  int32_t *dt, *de;
  TRY(scratch(h, kScrPersistHdr, (size_t)n, &dh));
  TRY(scratch(h, kScrPersistTerms, (size_t)(n_terms > 0 ? n_terms : 1), &dt));
  TRY(scratch(h, kScrRestoreErr, (size_t)n, &de));
  HIP_TRY(hipMemcpyAsync(dh, in, sizeof(mraft_persistent) * n, hipMemcpyHostToDevice, h->stream));
  if (n_terms > 0)
    HIP_TRY(hipMemcpyAsync(dt, terms, sizeof(int32_t) * n_terms, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(de, item_err, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
  mraft::launch_restore(dev_of(h), dh, n, dt, de, h->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  return MRAFT_OK;
}

int mraft_crash(mraft_engine *h, const int32_t *slots, int64_t n, int32_t *item_err, int32_t where) {
  TRY(enter(h));
  if (n < 0 || (n > 0 && !slots)) return fail(MRAFT_E_INVAL, "null argument");
  if (n > INT32_MAX) return fail(MRAFT_E_INVAL, "n = %lld items exceeds 2^31 - 1", (long long)n);
  if (n == 0) return MRAFT_OK;
  Stage sg(h, where);
  const int32_t *s = sg.in(slots, n);
  int32_t *e = sg.out(item_err, n);
  TRY(sg.status());
  // one launch, timers or not: the deadline arrays are null without them
  mraft::launch_crash(dev_of(h), s, n, e, h->tm_ed, h->tm_hd, h->stream);
  return sg.finish();
}

}  // extern "C"
