"""S1 denoise eps-neighbour lists at their word and cap boundaries (mc_bp_denoise_lds.inl: a list is eight 16-byte
words of eight u16 entries; lds_eps_pairs fills them entry by entry at slots its LDS atomics return,
lds_eps_own stores whole words of eight, a partial last word after the walk and nothing past the cap of 64):
MC_BP_NBCAP at 7 / 8 / 9 (the first word's flush), 16 / 17 (a later one) and 64 (the cap), crossed with
MC_BP_MIN_CLASS 0 / 2 / 4 / 5 / 6 (every LDS size class by slot size, then all slots in the 2048, 4096 and
16384 classes and in the global-memory kernel), on the dense S1 inputs of test_gpu_s1.py and one larger
frame, bit-exact against the CPU restatement (oracle/s1_oracle.c) and the reference's glue fixture.

The inputs must exercise what the cases are about, which test_inputs_reach_every_boundary_and_class asserts
from the inputs alone (s1_list_inputs.py; no device result enters, and test_s1_list_inputs_cpu.py asserts the
same without a GPU): the points' eps-neighbour counts must include multiples of 8, the value 64 and values
above 64, and the slots' voxel counts must put at least one slot in each LDS class."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from s1_list_inputs import (MIN_CLASSES, NBCAPS, check_inputs_reach_every_boundary_and_class, dense_inputs,
                            oracle_references)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    return dense_inputs()


@pytest.fixture(scope="module")
def references(inputs):
    return oracle_references(inputs)


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


def test_inputs_reach_every_boundary_and_class(inputs, references):
    check_inputs_reach_every_boundary_and_class(inputs, references)


def _check(ctx, inp, ref):
    """mc_backproject on one input against the oracle's frames (statistics columns and every mask);
    returns the masks"""
    from test_gpu_s1 import CMP_COLS, _run
    col, lab, off, pts = _run(ctx, *inp)
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
    return col, lab, off, pts


@pytest.mark.parametrize("min_cls", MIN_CLASSES)
@pytest.mark.parametrize("nbcap", NBCAPS)
def test_list_word_and_cap_boundaries_match_oracle(ctx, inputs, references, monkeypatch, nbcap, min_cls):
    monkeypatch.setenv("MC_BP_NBCAP", str(nbcap))
    monkeypatch.setenv("MC_BP_MIN_CLASS", str(min_cls))
    got = {name: _check(ctx, inp, references[name]) for name, inp in inputs.items()}
    z = np.load(os.path.join(GOLDEN, "s1_dense.npz"))  # the reference's own glue output of the same frames
    col, lab, off, pts = got["s1_dense"]
    np.testing.assert_array_equal(lab, z["out_labels"])
    np.testing.assert_array_equal(off, z["out_off"])
    np.testing.assert_array_equal(pts, z["out_pts"])
