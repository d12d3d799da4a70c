"""S1 ball query: the staged kernel (k_bp_query_lds: a slot's cropped scene points cell-sorted in LDS) and the
kernel it hands large slots to (k_bp_query), bit-exact against the CPU restatement (oracle/s1_oracle.c): masks
and statistics columns of every frame, through test_gpu_s1's _run and CMP_COLS.

The cases: the two kernels alone and splitting a batch between them (MC_BP_QUERY_STAGED, MC_BP_QUERY_CAND,
MC_BP_QUERY_CELLS); first-K truncation on the staged path, and ball_k above 20 (the fallback's wide list);
scene points on cell borders and duplicates; a scene with nothing in any box; one or two workgroups taking
every slot in turn (MC_BP_QUERY_GRID: the LDS state of a workgroup is reused slot after slot); repeated runs.
The inputs must exercise what the cases are about: s1_query_inputs.py asserts it from the inputs and the oracle
alone (here in test_inputs_meet_their_conditions, and without a GPU in test_s1_query_inputs_cpu.py)."""
import os

import numpy as np
import pytest

import s1_query_inputs as qi
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    return qi.inputs()


@pytest.fixture(scope="module")
def refs(inputs):
    return {name: qi.references(inp) for name, inp in inputs.items()}


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


def _check(ctx, inp, ref, **prm):
    """mc_backproject on one input against the oracle's frames (statistics columns and every mask); returns
    the masks and the statistics"""
    from test_gpu_s1 import CMP_COLS, _run
    col, lab, off, pts = _run(ctx, *inp, **prm)
    st = ctx.bp_candidates()
    g = 0
    for f, (ol, oo, op, ost) in enumerate(ref):
        big = ost[ost[:, 1] >= 25]
        dev = st[st[:, 0] == f]
        assert len(dev) == len(big), f"frame {f}: candidates {len(dev)} vs {len(big)}"
        for dc, oc in CMP_COLS:
            np.testing.assert_array_equal(dev[:, dc], big[:, oc], err_msg=f"frame {f} stat column {dc}")
        for k in range(len(ol)):
            assert col[g] == f and lab[g] == ol[k], (f, k)
            np.testing.assert_array_equal(pts[off[g]:off[g + 1]], op[oo[k]:oo[k + 1]], err_msg=f"frame {f} id {ol[k]}")
            g += 1
    assert g == len(col)
    return tuple(np.array(a) for a in (col, lab, off, pts)), np.array(st)


def test_inputs_meet_their_conditions(inputs, refs):
    for name in inputs:
        qi.check_split(inputs[name], refs[name])
    qi.check_quantised(qi.quantised_input()[0])


# 1. the paths agree
PATHS = {"default": {}, "fallback_only": {"MC_BP_QUERY_STAGED": "0"},
         "split_by_crop": {"MC_BP_QUERY_CAND": str(qi.SPLIT_CAND)},
         "split_by_cells": {"MC_BP_QUERY_CELLS": str(qi.SPLIT_CELLS)},
         "split_by_both": {"MC_BP_QUERY_CAND": str(qi.SPLIT_CAND), "MC_BP_QUERY_CELLS": str(qi.SPLIT_CELLS)}}


@pytest.mark.parametrize("name", ["s1_dense", "tiny", "small"])
@pytest.mark.parametrize("path", list(PATHS))
def test_paths_agree_with_oracle(ctx, inputs, refs, monkeypatch, path, name):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    (col, lab, off, pts), _ = _check(ctx, inputs[name], refs[name])
    if name == "s1_dense":  # the reference's own glue output of the same frames
        z = np.load(os.path.join(GOLDEN, "s1_dense.npz"))
        np.testing.assert_array_equal(lab, z["out_labels"])
        np.testing.assert_array_equal(off, z["out_off"])
        np.testing.assert_array_equal(pts, z["out_pts"])


# 2. first-K binds (the clustered scene: every slot is staged under the default caps)
@pytest.mark.parametrize("prm", qi.FIRSTK + [dict(ball_k=21), dict(ball_k=32)],
                         ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
def test_first_k_matches_oracle(ctx, prm):
    inp = qi.clustered_input()
    ref = qi.references(inp, **prm)
    if prm in qi.FIRSTK:
        assert qi.neighbour_sets(ref) != qi.neighbour_sets(qi.references(inp, **dict(prm, ball_k=32)))
        qi.check_all_staged(inp, ref, radius=prm.get("ball_radius", 0.01))
    _check(ctx, inp, ref, **prm)


@pytest.mark.parametrize("ball_k", [21, 32])
def test_wide_list_of_the_fallback_matches_oracle(ctx, monkeypatch, ball_k):
    monkeypatch.setenv("MC_BP_QUERY_STAGED", "0")
    inp = qi.clustered_input()
    _check(ctx, inp, qi.references(inp, ball_k=ball_k), ball_k=ball_k)


# 3. cell borders and duplicates
@pytest.mark.parametrize("path", ["default", "fallback_only", "split_by_both"])
def test_quantised_scene_matches_oracle(ctx, monkeypatch, path):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    inp = qi.quantised_input()
    qi.check_quantised(inp[0])
    (col, _, _, _), _ = _check(ctx, inp, qi.references(inp))
    assert len(col) > 0


# 4. nothing in the box
def test_empty_crops_then_a_normal_call(ctx, inputs, refs):
    inp = qi.shifted_input()
    (col, lab, off, pts), st = _check(ctx, inp, qi.references(inp))
    assert len(col) == 0 and len(lab) == 0 and len(pts) == 0 and len(off) == 1 and off[0] == 0
    assert len(st) > 0 and (st[:, 9] == 0).all() and (st[:, 8] == 0).all() and (st[:, 7] == 0).all()
    _check(ctx, inputs["tiny"], refs["tiny"])


# 5. LDS reuse: one or two workgroups take every slot in turn
@pytest.mark.parametrize("grid", ["1", "2"])
def test_few_workgroups_equal_the_default_grid(ctx, inputs, refs, monkeypatch, grid):
    want, want_st = _check(ctx, inputs["small"], refs["small"])
    monkeypatch.setenv("MC_BP_QUERY_GRID", grid)
    got, got_st = _check(ctx, inputs["small"], refs["small"])
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(want_st, got_st)


# 6. repeat
def test_two_runs_are_bit_identical(ctx, inputs):
    from test_gpu_s1 import _run
    a = tuple(np.array(x) for x in _run(ctx, *inputs["small"]))
    sa = np.array(ctx.bp_candidates())
    b = _run(ctx, *inputs["small"])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(sa, ctx.bp_candidates())
