"""Model of the in-place crash (mraft_crash, include/mraft.h): the reference's
crash1 + Make + readPersist stated as the round trip the call replaces, on the
CPU oracle. The oracle has no such call and gets none: a crash is its
read_persistent followed by its restore, which is what a killed process and a
new Make on the same Persister amount to. Test infrastructure only.

The oracle's restore starts a new ring at 0 and the engine keeps the head, so
states are compared with assert_states_equal(..., heads=False); that the
engine moved no term is checked on its raw log_term and log_head
(assert_log_untouched)."""
from __future__ import annotations

import numpy as np

from multiraft_amd._abi import ITEM_BAD_SLOT, ITEM_BAD_STATE, TIMER_NEVER
from reach_model import ReachModel


class CrashModel(ReachModel):
    """ReachModel with crash(slots). Timers are optional: before enable() the
    model has no deadline arrays and crash() does the state part only."""

    def crash(self, slots):
        """item_err per item. The slots are deduplicated, the bad ones dropped
        with their codes, and the rest go through read_persistent -> restore."""
        st, gp = self.o.st, self.G * self.P
        slots = np.asarray(slots, np.int64).reshape(-1)
        err = np.zeros(len(slots), np.int32)
        inr = (slots >= 0) & (slots < gp)
        err[~inr] = ITEM_BAD_SLOT
        s = np.where(inr, slots, 0)
        n = st["last_index"][s].astype(np.int64) - st["dummy_index"][s]
        err[inr & ((n < 0) | (n >= self.L))] = ITEM_BAD_STATE
        good = np.unique(slots[err == 0]).astype(np.int32)
        if len(good):
            hdr, terms = self.o.read_persistent(good)
            rerr = self.o.restore(hdr, terms)
            assert not rerr.any(), rerr
            if self.ed is not None:
                self.ed[good] = TIMER_NEVER
                self.hd[good] = TIMER_NEVER
        return err


def assert_log_untouched(before: dict, after: dict, ctx: str = ""):
    """The call moves no term: the raw log array and the ring heads are
    bit-identical before and after it."""
    assert np.array_equal(before["log_head"], after["log_head"]), (ctx, "log_head moved")
    assert np.array_equal(before["log_term"], after["log_term"]), (ctx, "a log word was written")
