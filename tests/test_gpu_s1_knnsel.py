"""S1 denoise k-NN list pass with 16 distance classes, one fetch round and a sorting network (k_bp_denoise_lds
step 10 for the classes of up to 4096 points; mc_bp_knnsel.hpp): three 160 x 120 frames (s1_knnsel_inputs.py:
a lattice wall whose distances tie, with selected sets of exactly k and beyond the network's 24 inputs; a
slot with a dropped second component; a slot with fewer than k kept points; a slot of 3600 voxels, whose
sorted positions use all twelve position bits of an entry; a generic surface), under MC_BP_MIN_CLASS 0 / 2 /
4 / 5 / 6 (every LDS size class, the 16384 class with its unchanged 2-bit entries, and the global-memory
kernel) crossed with MC_BP_NBCAP 64 and 30 (lists over the cap go to the ring queue), bit-exact against the
CPU restatement (oracle/s1_oracle.c): statistics columns and every mask.

The conditions on the inputs are asserted from the inputs and the oracle alone, before any device result
(test_inputs_reach_every_path; test_s1_knnsel_inputs_cpu.py asserts the same without a GPU)."""
import pytest

from s1_knnsel_inputs import MIN_CLASSES, NBCAPS, check_inputs, knnsel_inputs, oracle_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    return knnsel_inputs()


@pytest.fixture(scope="module")
def reference(inputs):
    return oracle_reference(inputs)


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


def test_inputs_reach_every_path(inputs, reference):
    check_inputs(inputs, reference)


@pytest.mark.parametrize("min_cls", MIN_CLASSES)
@pytest.mark.parametrize("nbcap", NBCAPS)
def test_knn_selection_matches_oracle(ctx, inputs, reference, monkeypatch, nbcap, min_cls):
    from test_gpu_s1_lists import _check
    monkeypatch.setenv("MC_BP_NBCAP", str(nbcap))
    monkeypatch.setenv("MC_BP_MIN_CLASS", str(min_cls))
    _check(ctx, inputs, reference)
