"""Which stream the engine ends up on (mraft_get_stream) after
mraft_set_stream, mraft_fanin_reserve_cus and mraft_set_tick_shards, in every
combination DESIGN.md's stream table lists: the caller's stream if one is set,
else the CU-masked tick stream if one exists, else the engine's own."""
import numpy as np
import pytest


@pytest.mark.gpu
def test_engine_stream_after_each_stream_call_gpu():
    import torch
    from oracle_lib import Oracle, assert_states_equal
    from multiraft_amd import Engine, synth_tick_state
    G, P, L = 8, 3, 16
    st, lp, _ = synth_tick_state(G, P, L, seed=7)
    caller = torch.cuda.Stream()  # kept alive to the end of the test
    c = caller.cuda_stream
    assert c
    with Engine(G, P, L) as e:
        e.load_state(st)
        s0 = e.stream()  # the engine's own
        assert s0 and s0 != c
        e.set_stream(c)
        assert e.stream() == c
        # no CUs reserved: the shard count leaves a caller's stream alone
        e.set_tick_shards(2)
        assert e.stream() == c
        e.set_tick_shards(1)
        assert e.stream() == c
        e.set_stream(None)
        assert e.stream() == s0
        # one shard: reserving CUs puts the engine on a new masked tick stream
        e.fanin_reserve_cus(8)
        masked = e.stream()
        assert masked and masked != s0
        e.set_stream(c)
        assert e.stream() == c
        e.set_stream(None)
        assert e.stream() == masked
        # shards carry the mask themselves: the masked tick stream goes ...
        e.set_tick_shards(2)
        assert e.stream() == s0
        # ... and comes back (its address may be the old one's: not compared)
        e.set_tick_shards(1)
        assert e.stream() and e.stream() != s0
        # one shard: a reservation replaces a caller's stream
        e.set_stream(c)
        e.fanin_reserve_cus(0)
        assert e.stream() == s0
        # two shards: a reservation leaves the engine stream as it is
        e.set_tick_shards(2)
        e.set_stream(c)
        e.fanin_reserve_cus(8)
        assert e.stream() == c
        e.fanin_reserve_cus(0)
        assert e.stream() == c
        # the handle still works
        gf = e.replicate_tick(lp)
        o = Oracle(G, P, L, st)
        assert np.array_equal(gf, o.replicate_tick(lp))
        assert_states_equal(e.store_state(), o.state(), G, P, L, "after the stream calls")
