"""CPU check that the seeded clock-step cases of tests/timers_cases.py (run on
the GPU by tests/test_timers_gpu.py) actually produce the situations they are
there for, counted by the model: two Leaders in one group with different and
with equal terms, a Leader whose heartbeat fired deposed by the election
round, a sender that steps down on a follower's higher term, followers that
need InstallSnapshot — and grants and elections, for the two timer resets of
the round."""
from timers_cases import CLOCK_CASES, CLOCK_STEPS, NOW0, clock_case_model


def test_clock_cases_cover_the_listed_situations():
    total = {}
    for P, G, send_all in CLOCK_CASES:
        m = clock_case_model(P, G, send_all)[-1]
        for k in range(CLOCK_STEPS):
            m.clock_step(NOW0 + k, send_all)
        for k, v in m.stats.items():
            total[k] = total.get(k, 0) + v
    print(total)
    for k in ("two_leaders_diff", "two_leaders_equal", "fired_deposed", "sender_stepped_down", "need_snapshot",
              "grants", "elected"):
        assert total[k] >= 10, (k, total)
