"""The inputs of the S1 eps-list boundary tests (test_gpu_s1_lists.py) meet their conditions, checked without a
GPU from the oracle and a numpy restatement of its voxel points (s1_list_inputs.py): eps-neighbour counts at
every multiple of 8, at the cap of 64 and above it, lists on both sides of every MC_BP_NBCAP of the cases, and
a slot in every LDS size class under the cases' MC_BP_MIN_CLASS values."""
from s1_list_inputs import check_inputs_reach_every_boundary_and_class, dense_inputs, oracle_references


def test_dense_inputs_reach_every_list_boundary_and_size_class():
    inputs = dense_inputs()
    hist, reached = check_inputs_reach_every_boundary_and_class(inputs, oracle_references(inputs))
    assert hist[64] > 0 and hist[65:].sum() > 0 and reached == [0, 1, 2, 3, 4, 5, 6]
