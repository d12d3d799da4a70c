"""The inputs of the S1 k-NN selection tests (test_gpu_s1_knnsel.py) meet their conditions, checked without a
GPU from the inputs, the oracle and the numpy restatement of the distance class (s1_knnsel_inputs.py): on the
lattice wall a point whose selected set exceeds the sorting network (the leftover path), one whose set is
exactly k, and points with fewer than k list entries (the ring queue); a slot with a component the 20 % filter
drops; a slot with fewer than k kept points; a slot of 3073 .. 4096 voxels; lists on both sides of the small
MC_BP_NBCAP."""
import numpy as np

from s1_knnsel_inputs import KNN, KNN_NET, check_inputs, knn_class, knnsel_inputs, oracle_reference


def test_knnsel_inputs_reach_every_path():
    inp = knnsel_inputs()
    cnt, sel = check_inputs(inp, oracle_reference(inp))
    assert sel.max() > KNN_NET and (sel == KNN).any() and (cnt < KNN).any()
    # lattice distances tie: the wall's selected sets end on a whole tie group
    assert len(np.unique(sel[sel > 0])) >= 4


def test_class_restatement_is_monotone_and_clamped():
    eps2 = 0.04 * 0.04
    d2 = np.sort(np.random.default_rng(3).random(200000) * eps2)
    d2 = d2[d2 < eps2]
    c = knn_class(d2)
    assert c[0] == 0 and c.max() == 15 and (np.diff(c.astype(np.int64)) >= 0).all()
    assert knn_class(np.array([np.nextafter(eps2, 0.0)]))[0] == 15
