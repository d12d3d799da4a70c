"""The S1 pixel- and voxel-stage inputs (s1_voxel_inputs.py) reach what they are for, checked without a GPU:
per case the restatement's voxel counts equal the oracle's nvox column, each tier's modelled verdict is the one
the case is named for, no (p - vmin) / voxel lies within the witness's margin of an integer, and the oracle's
means equal the longdouble witness's within c * 2^-52 * max|mean| for a voxel of c points.  The tiers' sizes come
from mc_bp_voxel.inl, so a retuned constant moves the cases or fails here."""
import numpy as np
import pytest

import s1_voxel_inputs as V


def test_tier_constants_and_which_table_routes_exist():
    c = V.constants()
    # a slot at kVxV voxels can meet kVxT new ones in one chunk: the first tier's table can fill before the id
    # test sees the overflow (the probe loop's h < 0 exit); the second tier's cannot
    assert c["kVxV"] + c["kVxT"] > c["kVxH"]
    assert c["kVxV2"] + c["kVxT2"] <= c["kVxH2"]
    assert c["kVxL2"] < c["kVxV"] and c["kVxV"] < c["kVxH"] < c["kVxV2"]
    assert set(V.COUNTS) == {c["kVxL2"] - 1, c["kVxL2"], c["kVxL2"] + 1, c["kVxV"], c["kVxV"] + 1, c["kVxH"] + 1,
                             c["kVxV2"], c["kVxV2"] + 1}
    assert all(any(n % t == r for n in V.CHUNK_SIZES) for t in (c["kVxT"], c["kVxT2"]) for r in (0, 1))


def test_model_of_a_tier():
    """abandons() on hand-made key sequences: each verdict and the chunk that decides between table and ids"""
    idx = np.zeros((12, 3), np.int64)
    rank = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5])
    assert V.abandons(rank, idx, 4, 8, 6) is None
    assert V.abandons(rank, idx, 4, 8, 5) == "ids"
    assert V.abandons(rank, idx, 12, 5, 4) == "table"      # one chunk takes the keys past H
    assert V.abandons(rank, idx, 2, 5, 4) == "ids"         # short chunks: the id test sees 5 > 4 first
    far = idx.copy()
    far[7, 1] = V.SPAN
    assert V.abandons(rank, far, 4, 8, 6) == "span"
    far[7, 1] = V.SPAN - 1
    assert V.abandons(rank, far, 4, 8, 6) is None


@pytest.mark.parametrize("name", V.CASES + ["idx21over"])
def test_case_reaches_what_it_is_for(name):
    print(name, V.check_case(name))


def test_restatement_agrees_with_the_list_inputs_restatement():
    """restate() against s1_list_inputs.voxel_points (np.add.at sums) on a case with several slots: the same
    voxels in the same order, means within a rounding per point"""
    from s1_list_inputs import voxel_points
    c = V.case("chunks")
    vp = voxel_points(c.depth[0], c.seg[0], c.K[0], c.T[0])
    slots = c.slots()
    assert sorted(vp) == sorted(slots)
    for i, s in slots.items():
        m = V.oracle_means(s)
        assert m.shape == vp[i].shape
        np.testing.assert_allclose(m, vp[i], rtol=0, atol=len(s.pixels) * 2.0 ** -52 * np.abs(m).max())
