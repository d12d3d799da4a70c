"""The input conditions of test_gpu_s1_query.py, asserted without a GPU from the inputs and the oracle alone
(s1_query_inputs.py): slots on both sides of the split cases' caps, and of the default caps on the small shape;
first-K truncation that changes a neighbour set under every parameter set of the first-K cases, on slots that all
take the staged kernel; scene points on cell borders and duplicates in the quantised scene; no crop at all in the
shifted one."""
import numpy as np
import pytest

import s1_query_inputs as qi


@pytest.fixture(scope="module")
def inputs():
    return qi.inputs()


@pytest.mark.parametrize("name", ["s1_dense", "tiny", "small"])
def test_slots_on_both_sides_of_the_split_caps(inputs, name):
    qi.check_split(inputs[name], qi.references(inputs[name]))


def test_small_shape_has_slots_beyond_the_default_caps(inputs):
    prof = qi.slot_profile(inputs["small"], qi.references(inputs["small"]))
    assert (prof[:, 0] > qi.DEFAULT_CAND).any() and (prof[:, 1] > qi.DEFAULT_CELLS).any()
    assert ((prof[:, 0] <= qi.DEFAULT_CAND) & (prof[:, 2] <= qi.DEFAULT_CELLS)).any()


@pytest.mark.parametrize("prm", qi.FIRSTK, ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
def test_first_k_binds_on_staged_slots(prm):
    inp = qi.clustered_input()
    qi.check_first_k_binds(inp, prm)
    qi.check_all_staged(inp, qi.references(inp, **prm), radius=prm.get("ball_radius", 0.01))


def test_quantised_scene_has_border_points_and_duplicates():
    inp = qi.quantised_input()
    qi.check_quantised(inp[0])
    assert sum(len(r[0]) for r in qi.references(inp)) > 0  # and masks are still kept over it


def test_shifted_scene_leaves_every_crop_empty():
    ref = qi.references(qi.shifted_input())
    st = np.concatenate([r[3] for r in ref])
    assert len(st) and (st[:, 5] == 0).all() and (st[:, 8] == 0).all() and all(len(r[0]) == 0 for r in ref)
