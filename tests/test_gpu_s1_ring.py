"""S1 denoise ring search with a lane-private mark and walk (k_bp_knn_ring, mc_bp_denoise.inl; mc_bp_ring.hpp): two
160 x 120 frames (s1_ring_inputs.py: deferred points that settle at R = 1, at R = 2 and by the whole cloud; a
slot of 36 points, whose buckets the cells of a search must share; deferred points at the grid's first and last
cells; k nearest neighbours in shell cells; exact ties at the k-th distance across cells; consecutive small
slots, so that a wave holds points of several grids; a slot of more than 3072 voxels), under MC_BP_MIN_CLASS
0 / 2 / 5 / 6 crossed with MC_BP_NBCAP 64 and 30 (lists over the cap go to the ring queue), bit-exact against
the CPU restatement (oracle/s1_oracle.c): statistics columns and every mask.

The conditions on the inputs are asserted from the inputs and the witness alone, before any device result
(test_inputs_reach_every_condition; test_s1_ring_inputs_cpu.py asserts the same without a GPU)."""
import pytest

from s1_ring_inputs import MIN_CLASSES, NBCAPS, check_inputs, oracle_reference, ring_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    return ring_inputs()


@pytest.fixture(scope="module")
def reference(inputs):
    return oracle_reference(inputs)


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


def test_inputs_reach_every_condition(inputs):
    check_inputs(inputs)


@pytest.mark.parametrize("min_cls", MIN_CLASSES)
@pytest.mark.parametrize("nbcap", NBCAPS)
def test_ring_search_matches_oracle(ctx, inputs, reference, monkeypatch, nbcap, min_cls):
    from test_gpu_s1_lists import _check
    monkeypatch.setenv("MC_BP_NBCAP", str(nbcap))
    monkeypatch.setenv("MC_BP_MIN_CLASS", str(min_cls))
    _check(ctx, inputs, reference)
