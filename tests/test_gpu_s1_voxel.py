"""S1's pixel lists and voxel means, read back from the device (Context.bp_voxels) and compared bit for bit, at
every size-dependent branch of mc_bp_pixels.inl and mc_bp_voxel.inl (s1_voxel_inputs.py names the cases and
test_s1_voxel_inputs_cpu.py asserts without a GPU that each reaches its branch):

  * every slot's pixel list equals the restatement's valid pixels, row-major;
  * its voxel count and its means, as float64 bit patterns and in order, equal the oracle's sequential fold
    (oracle.s1_voxel) over the restated world points; its grid origin equals min - voxel / 2;
  * with MC_VX_GLOBAL unset, the slots each LDS tier handed on are as many as the tier model says: the natural
    hand-offs (ids, table, span), which abandon a slot after running sums were written into its range;
  * the statistics columns and every mask's point set equal the oracle's, as in test_gpu_s1.py.

Each case runs with MC_VX_GLOBAL unset, 1 (every slot in k_bp_voxel) and 2 (every slot in the second LDS tier,
where the 511 / 512 / 513 cases sit on kVxL2: running sums in LDS below it, in HBM from it on)."""
import os

import numpy as np
import pytest

import s1_voxel_inputs as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

KNOBS = [None, "1", "2"]


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


@pytest.fixture(scope="module")
def references():
    """case -> (scene, per frame: the restated slots, their oracle means, the oracle's frame), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            c = V.case(name)
            frames = []
            for f in range(len(c.depth)):
                slots = c.slots(f)
                means = {i: V.oracle_means(s, c.voxel) for i, s in slots.items()}
                frames.append((slots, means, V.oracle_frame(c, f)))
            cache[name] = (c.scene(), frames)
        return cache[name]
    return get


def _backproject(ctx, c, scene):
    from maskclustering_amd import _native
    ctx.set_points(scene)
    ctx.backproject(c.depth, c.seg, c.K, c.T, _native.bp_params(voxel_size=c.voxel) if c.voxel != V.VOXEL else None)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_voxels(vx, frames, name):
    want = [(f, i) for f, (slots, _, _) in enumerate(frames) for i in slots]
    assert [tuple(r) for r in vx["slots"][:, :2].tolist()] == want, f"{name}: the slots' (frame, id)"
    for x, (f, i) in enumerate(want):
        s, means = frames[f][0][i], frames[f][1][i]
        tag = f"{name} frame {f} id {i}"
        assert vx["slots"][x, 2] == len(s.pixels), tag
        np.testing.assert_array_equal(vx["pixels"][x], s.pixels, err_msg=tag + ": pixel list")
        assert vx["slots"][x, 3] == len(means) == s.nvox, f"{tag}: {vx['slots'][x, 3]} voxels, the oracle {len(means)}"
        np.testing.assert_array_equal(_bits(vx["origin"][x]), _bits(s.vmin), err_msg=tag + ": grid origin")
        got, ref = _bits(vx["means"][x]), _bits(means)
        bad = np.flatnonzero((got != ref).any(axis=1))
        assert len(bad) == 0, (f"{tag}: {len(bad)} of {len(ref)} voxel means differ in their bits, the first at voxel "
                               f"{bad[0]}: {vx['means'][x][bad[0]]!r} vs {means[bad[0]]!r}")


def _check_end_to_end(ctx, frames, name):
    from test_gpu_s1 import CMP_COLS
    col, lab, off, pts = ctx.bp_masks()
    st = ctx.bp_candidates()
    g = 0
    for f, (_, _, (ol, oo, op, ost)) in enumerate(frames):
        big = ost[ost[:, 1] >= V.FEW]
        dev = st[st[:, 0] == f]
        assert len(dev) == len(big), f"{name} frame {f}: candidates {len(dev)} vs {len(big)}"
        for dc, oc in CMP_COLS:
            np.testing.assert_array_equal(dev[:, dc], big[:, oc], err_msg=f"{name} frame {f} stat column {dc}")
        for k in range(len(ol)):
            assert col[g] == f and lab[g] == ol[k], (name, f, k)
            np.testing.assert_array_equal(pts[off[g]:off[g + 1]], op[oo[k]:oo[k + 1]], err_msg=f"{name} frame {f} id {ol[k]}")
            g += 1
    assert g == len(col)


@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", V.CASES)
def test_pixel_lists_and_voxel_means_bit_for_bit(ctx, references, monkeypatch, name, knob):
    if knob is None:
        monkeypatch.delenv("MC_VX_GLOBAL", raising=False)
    else:
        monkeypatch.setenv("MC_VX_GLOBAL", knob)
    scene, frames = references(name)
    _backproject(ctx, V.case(name), scene)
    vx = ctx.bp_voxels()
    _check_voxels(vx, frames, name)
    if knob is None:
        want = V.handed([s for slots, _, _ in frames for s in slots.values()])
        assert vx["handed"] == want, f"{name}: the tiers handed on {vx['handed']}, the model says {want}"
    _check_end_to_end(ctx, frames, name)


def test_axis_limit_refused_is_a_status_and_the_context_goes_on(references, monkeypatch):
    """a voxel index of 2^21 on an axis: MC_ERR_UNSUPPORTED from k_bp_voxel's flag (the index is clamped before
    the key is packed), no result to read back, and the same context then runs s1_tiny to the golden"""
    from maskclustering_amd import _native
    monkeypatch.delenv("MC_VX_GLOBAL", raising=False)
    ctx = _native.Context(0)
    scene, _ = references("idx21over")
    with pytest.raises(_native.McError) as e:
        _backproject(ctx, V.case("idx21over"), scene)
    assert e.value.code == _native.MC_ERR_UNSUPPORTED and "voxel index beyond 2^21 per axis" in str(e.value)
    with pytest.raises(_native.McError) as e:
        ctx.bp_voxels()
    assert e.value.code == _native.MC_ERR_STATE
    z = dict(np.load(os.path.join(GOLDEN, "s1_tiny.npz")))
    ctx.set_points(np.asarray(z["in_scene"], np.float64).astype(np.float32))
    ctx.backproject(z["in_depth"], z["in_seg"], z["in_intrinsics"], z["in_poses"])
    col, lab, off, pts = ctx.bp_masks()
    np.testing.assert_array_equal(lab, z["out_labels"])
    np.testing.assert_array_equal(off, z["out_off"])
    np.testing.assert_array_equal(pts, z["out_pts"])
    scene, frames = references("idx21ok")       # and the accepted side of the limit on this context
    _backproject(ctx, V.case("idx21ok"), scene)
    _check_voxels(ctx.bp_voxels(), frames, "idx21ok")


def test_read_back_needs_a_call_of_one_batch(references, monkeypatch):
    from maskclustering_amd import _native
    monkeypatch.delenv("MC_VX_GLOBAL", raising=False)
    ctx = _native.Context(0)
    with pytest.raises(_native.McError) as e:       # no call yet
        ctx.bp_voxels()
    assert e.value.code == _native.MC_ERR_STATE
    c = V.case("pix96")
    scene, frames = references("pix96")
    assert len(c.depth) == 2
    monkeypatch.setenv("MC_BP_BATCH_PIXELS", str(c.depth.shape[1] * c.depth.shape[2]))   # a frame per batch
    _backproject(ctx, c, scene)
    assert ctx.bp_batching()["frames_per_batch"] == 1
    with pytest.raises(_native.McError) as e:
        ctx.bp_voxels()
    assert e.value.code == _native.MC_ERR_STATE and "2 batches" in str(e.value)
    _check_end_to_end(ctx, frames, "pix96 in two batches")
    monkeypatch.delenv("MC_BP_BATCH_PIXELS")
    _backproject(ctx, c, scene)
    _check_voxels(ctx.bp_voxels(), frames, "pix96")
