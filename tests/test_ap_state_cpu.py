"""The evaluation state buffer without a GPU: the numpy restatement of its layout (tests/ap_state_util.py),
the key order, and the transport of sweep.gather_states in a one-rank gloo group."""
import numpy as np
import pytest

import ap_restatement as R
import ap_state_util as U


def test_keys_sort_like_scores():
    scores = np.array([-np.inf, -3.5, -1e-300, -0.0, 0.0, 5e-324, 0.25, 1.0, np.inf])
    keys = [U.key_of(s) for s in scores]
    assert keys[3] == keys[4] == 1 << 63                  # -0.0 is 0.0
    assert keys == sorted(keys) and len(set(keys)) == len(scores) - 1


def test_expected_state_round_trip():
    rs = R.APRestatement((3, 5, 8), None, 100, False)
    rs.scans.append({(0, 0): [(0.5, 1), (0.5, 0), (0.25, 0)], (2, 9): [(1.0, 1)]})
    rs.scans.append({(0, 0): [(0.25, 1)]})
    rs.hard_fn[1, 2], rs.flags[0, 0], rs.flags[1, 2] = 7, 3, 1
    buf = U.expected_state(rs)
    st = U.parse_state(buf)
    assert len(buf) % 8 == 0 and (st["C"], st["O"], st["R"]) == (3, 10, 3)
    assert st["run_off"].tolist() == [0] + [2] * 29 + [3]
    assert st["key"].tolist() == [U.key_of(0.25), U.key_of(0.5), U.key_of(1.0)]
    assert st["n_true"].tolist() == [1, 1, 1] and st["n_false"].tolist() == [1, 1, 0]
    assert st["hard_fn"][12] == 7 and st["flags"][0] == 3 and st["flags"][12] == 1
    np.testing.assert_array_equal(U.build_state(st), buf)


@pytest.mark.parametrize("gather", (True, False), ids=("gather", "all_gather"))
def test_gather_states_in_a_one_rank_group(gather, monkeypatch):
    import torch.distributed as dist
    from maskclustering_amd import frame_shard
    from maskclustering_amd.sweep import gather_states
    if not gather:
        monkeypatch.setattr(frame_shard, "_GATHER_BACKENDS", ())
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{U.free_port()}", rank=0, world_size=1)
    try:
        state = np.arange(48, dtype=np.uint8)
        got = gather_states(state, dist.group.WORLD, dst=0)
        assert len(got) == 1 and got[0].device.type == "cpu"
        np.testing.assert_array_equal(got[0].numpy(), state)
    finally:
        dist.destroy_process_group()
