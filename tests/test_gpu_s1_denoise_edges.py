"""S1 denoise on the device against the independent witness (s1_witness.py) directly: no oracle enters.  The
inputs (s1_denoise_inputs.py) put DBSCAN's border rule and the class filter's limit where they decide a
statistics column: contested border points whose label decides 19 points' survival (the lower-numbered
cluster first and later in space, on an exact lattice and under a turned pose), a border point between three
clusters (at min_points = 6), a border point reached by one core point, classes of exactly 0.2 n and one
below, noise classes that are kept, slots that are all noise, slots of one and two voxels.  The rule is
implemented once per size class (k_bp_denoise_lds<N> step 8, k_bp_denoise), each with a list path and a
cell-walk path, so the cases cross MC_BP_MIN_CLASS 0 / 2 / 4 / 5 / 6 with MC_BP_NBCAP 64 and 2 (2: below
min_points - 1, every border point walks the cells).  The mc_bp_params fields of the denoise
(dbscan_min_points, dbscan_eps, component_min_fraction, sor_neighbors, sor_std_ratio) run at values other
than the reference's, in the smallest class by size and in the global-memory kernel.  Bit-equal statistics
columns and point sets; no slot is skipped or masked.

What the cases would catch, by the witness's numbers: were step 8's `sB[r2] < best` flipped to `>`, the
contested point of ids 1 and 2 (frames 0 and 1) would not join cluster 0 (from best = INT_MAX no cluster is
ever taken and every border point turns noise; were the largest key taken, it would join cluster 1), cluster
0 would count 19 < 0.2 * 100, and ndbscan would be 80 (or 81) instead of 100; id 5's ndbscan would be 26
instead of 27.  Were the class filter's `<` a `<=`, id 4's class of exactly 20 of 100 would be dropped
(ndbscan 61 instead of 81), and so would cluster 0 of ids 1 and 2 (80 instead of 100) and id 6's noise class
of 10 of 50 (40 instead of 50).

The conditions on the inputs are asserted from the witness alone under every parameter set, with no knife-edge
decision among them (test_inputs_meet_their_conditions; test_s1_witness_cpu.py asserts the same without a
GPU, and compares the witness with the oracle, scikit-learn and scipy)."""
import numpy as np
import pytest

import s1_denoise_inputs as D
import s1_witness as W

pytestmark = pytest.mark.gpu

VARIANTS = [v for v in D.VARIANTS if v != "default"]


@pytest.fixture(scope="module")
def inputs():
    return D.denoise_inputs()


@pytest.fixture(scope="module")
def witnessed(inputs):
    """variant -> the witness's frames under its parameters, computed once"""
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = D.witness_reference(inputs, **D.VARIANTS[variant])
        return cache[variant]
    return get


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


@pytest.mark.parametrize("variant", list(D.VARIANTS))
def test_inputs_meet_their_conditions(inputs, witnessed, variant):
    D.check_inputs(inputs, witnessed(variant), **D.VARIANTS[variant])


def _check(ctx, inp, wit, few_points=25, **prm):
    """mc_backproject on the inputs against the witness's frames: statistics columns and every mask"""
    from test_gpu_s1 import CMP_COLS, _run
    col, lab, off, pts = _run(ctx, *inp, **W.abi_params(prm))
    st = ctx.bp_candidates()
    g = 0
    for f, fr in enumerate(wit):
        big = np.array([W.stats_row(s) for s in fr.values() if s["npix"] >= few_points], np.int64)
        dev = st[st[:, 0] == f]
        assert len(dev) == len(big), f"frame {f}: candidates {len(dev)} vs {len(big)}"
        print(f"frame {f}: device {dev[:, [c for c, _ in CMP_COLS]].tolist()}")
        for k, (dc, _) in enumerate(CMP_COLS):
            np.testing.assert_array_equal(dev[:, dc], big[:, k], err_msg=f"frame {f} column {W.STAT_NAMES[k]}")
        for s in fr.values():
            if not s["kept"]:
                continue
            assert col[g] == f and lab[g] == s["id"], (f, s["id"])
            np.testing.assert_array_equal(pts[off[g]:off[g + 1]], s["points"], err_msg=f"frame {f} id {s['id']}")
            g += 1
    assert g == len(col)


@pytest.mark.parametrize("min_cls", D.MIN_CLASSES)
@pytest.mark.parametrize("nbcap", D.NBCAPS)
def test_border_and_class_edges_match_witness(ctx, inputs, witnessed, monkeypatch, nbcap, min_cls):
    monkeypatch.setenv("MC_BP_NBCAP", str(nbcap))
    monkeypatch.setenv("MC_BP_MIN_CLASS", str(min_cls))
    _check(ctx, inputs, witnessed("default"))


@pytest.mark.parametrize("min_cls", [0, 6])
@pytest.mark.parametrize("variant", VARIANTS)
def test_parameter_variants_match_witness(ctx, inputs, witnessed, monkeypatch, variant, min_cls):
    monkeypatch.setenv("MC_BP_MIN_CLASS", str(min_cls))
    _check(ctx, inputs, witnessed(variant), **D.VARIANTS[variant])


@pytest.mark.parametrize("variant", ["default", "min_points_6"])
def test_one_frame_batches_match_witness(ctx, inputs, witnessed, monkeypatch, variant):
    monkeypatch.setenv("MC_BP_BATCH_PIXELS", str(D.H * D.Wd))
    _check(ctx, inputs, witnessed(variant), **D.VARIANTS[variant])
