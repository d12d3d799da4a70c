"""The inputs of the S1 ring-search tests (test_gpu_s1_ring.py) meet their conditions, checked without a GPU from
the inputs and the witness alone (s1_ring_inputs.py): deferred points that settle at R = 1, at R = 2 and by the
whole cloud, at least ten each; a slot whose 2 n buckets are fewer than the 125 cells of a search; deferred
points in cell 0 or 1 on every axis and in the slot's last cell; deferred points with one of their k nearest in
a shell cell; an exact tie at the k-th distance across two cells; consecutive slots of 20 to 60 points; a slot of
more than 3072 voxels with deferred points.  No decision of the witness sits on a knife edge."""
from s1_ring_inputs import check_inputs, ring_inputs


def test_ring_inputs_reach_every_condition():
    rep = check_inputs(ring_inputs())
    assert min(rep.values()) >= 1, rep
