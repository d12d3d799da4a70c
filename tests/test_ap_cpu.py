"""The AP restatement (tests/ap_restatement.py) against the reference's own evaluate_matches on
tests/golden/ap_small.npz (made by tests/golden/make_ap_golden.py), class-aware and --no_class.

The AP bound, n * 2^-52 absolute with n the cell's number of precision/recall points, is derived:
precision, recall and step widths are bit-equal to numpy's (one rounding each), every term of the
final sum is at most 1 in magnitude and so is the sum, so a reordered or fused sum of n such
terms differs by at most n ulp of 1."""
import json
import os

import numpy as np
import pytest

import ap_restatement as R
from conftest import GOLDEN

MODES = ("ca", "nc")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ap_small.npz"))


def restate(z, mode, scans=None):
    rs = R.APRestatement(z["class_ids"], z["overlaps"], int(z["min_region_size"]), mode == "nc")
    tables = []
    for s in range(int(z["num_scans"])) if scans is None else scans:
        tables.append(rs.add_scan(z[f"s{s}_gt"], z[f"s{s}_off"], z[f"s{s}_pts"], z[f"s{s}_classes"], z[f"s{s}_scores"]))
    return rs, tables


def npoints(shape, curves):
    n = np.ones(shape)
    for (c, o), cv in curves.items():
        n[c, o] = len(cv[0]) + 1
    return n


@pytest.mark.parametrize("mode", MODES)
def test_scan_tables_equal_the_reference_dicts(golden, mode):
    labels = [str(x) for x in golden["class_labels"]]
    _, tables = restate(golden, mode)
    for s, t in enumerate(tables):
        g2p = json.loads(str(golden[f"{mode}_s{s}_gt2pred"]))
        p2g = json.loads(str(golden[f"{mode}_s{s}_pred2gt"]))
        R.assert_tables_equal(t, R.tables_from_dicts(g2p, p2g, labels), f"{mode} scan {s}")


@pytest.mark.parametrize("mode", MODES)
def test_ap_equals_the_reference(golden, mode):
    rs, _ = restate(golden, mode)
    ap, stats, curves = rs.result()
    want = golden[f"{mode}_ap"][0]
    n = npoints(ap.shape, curves)
    assert R.ap_close(ap, want, n)
    assert np.sum((want > 0) & (want < 1)) >= (20 if mode == "ca" else 6)      # the fixture is not vacuous
    assert all(v >= 1 for v in rs.counters.values()), rs.counters
    labels = [str(x) for x in golden["class_labels"]]
    avgs = json.loads(str(golden[f"{mode}_avgs"]))
    mine = R.compute_averages(ap, golden["overlaps"], labels)
    bound = n.max() * 2.0 ** -52
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert abs(mine[k] - avgs[k]) <= bound, k
    for name in labels:
        for k, v in avgs["classes"][name].items():
            got = mine["classes"][name][k]
            assert (np.isnan(got) and np.isnan(v)) or abs(got - v) <= bound, (name, k)


@pytest.mark.parametrize("mode", MODES)
def test_ap_does_not_depend_on_the_example_order(golden, mode):
    """What licenses the device's free order of examples within a cell."""
    rs, _ = restate(golden, mode)
    ap, stats, curves = rs.result()
    for seed in range(3):
        ap2, stats2, curves2 = rs.result(rng=np.random.default_rng(seed))
        np.testing.assert_array_equal(stats2, stats)
        np.testing.assert_array_equal(ap2, ap)       # same curve, same sum order: bit-equal
        for k in curves:
            for a, b in zip(curves[k], curves2[k]):
                np.testing.assert_array_equal(a, b)


def test_package_averages_equal_the_restatement(golden):
    from maskclustering_amd.sweep import compute_averages
    labels = [str(x) for x in golden["class_labels"]]
    ap = golden["ca_ap"][0]
    a, b = compute_averages(ap, golden["overlaps"], labels), R.compute_averages(ap, golden["overlaps"], labels)
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert a[k] == b[k]
    assert a["classes"].keys() == b["classes"].keys()


def test_pack_matches_round_trip(golden):
    """The drop-in's packing of the reference's dicts carries the same scan as the restatement's tables."""
    from maskclustering_amd.evaluation.evaluate import pack_matches
    labels = [str(x) for x in golden["class_labels"]]
    for mode in MODES:
        a = R.APRestatement(golden["class_ids"], golden["overlaps"], int(golden["min_region_size"]), mode == "nc")
        for s in range(int(golden["num_scans"])):
            g2p = json.loads(str(golden[f"{mode}_s{s}_gt2pred"]))
            p2g = json.loads(str(golden[f"{mode}_s{s}_pred2gt"]))
            a.add_tables(pack_matches(g2p, p2g, labels))
        b, _ = restate(golden, mode)
        ap_a, st_a, _ = a.result()
        ap_b, st_b, _ = b.result()
        np.testing.assert_array_equal(st_a, st_b)
        np.testing.assert_array_equal(ap_a, ap_b)
