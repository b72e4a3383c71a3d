"""The model's clock step against the host-driven sequence on a second model
(tests/timers_sequence.py states the sequence, where the two must agree, and
the two documented heartbeat_due differences), over all CLOCK_CASES for
CLOCK_STEPS steps each.

The condition: at least 75 % of all group-runs are inside the equivalence.
Measured with these cases (MEASURED below, asserted so that the figure cannot
go stale): 2,682 of 3,340 group-runs inside (80.3 %), no state or election_due
difference among them, and 1,900 heartbeat_due differences, 306 at Leaders
that fired and were deposed and 1,594 at senders that had not fired."""
import numpy as np

from timers_cases import CLOCK_CASES, NOW0
from timers_sequence import model_pair, run_model_case

MEASURED = dict(groups=3340, inside=2682, hd_fired_not_sender=306, hd_sender_not_fired=1594)


def test_clock_step_equals_the_host_driven_sequence():
    total = {}
    for P, G, send_all in CLOCK_CASES:
        stats = run_model_case(P, G, send_all)[1]
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    print(total)
    assert total["inside"] >= 0.75 * total["groups"], total
    assert {k: total[k] for k in MEASURED} == MEASURED, total
    # the inside groups alone contain what the comparison is there for
    for k in ("grants", "elected", "sender_stepped_down", "fired_deposed", "hd_fired_not_sender",
              "hd_sender_not_fired"):
        assert total[k] >= 1, (k, total)


def test_sequence_side_is_a_real_second_run():
    """The two sides share nothing: the sequence side's state changes only
    through its own calls (a clock step on side one leaves side two alone)."""
    L, a, b = model_pair(3, 33, False)
    before = b.store_state()
    a.clock_step(NOW0, False)
    after = b.store_state()
    assert all(np.array_equal(before[k], after[k]) for k in before)
