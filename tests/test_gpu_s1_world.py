"""S1 voxels: the per-slot choice between the affine and the general form of a pixel's world point
(mc_bp_world.hpp: bp_pose_affine, bp_world_affine, bp_world) in the three voxel kernels: the first LDS tier
(MC_VX_GLOBAL=0), the global-hash kernel (1) and the second LDS tier (2).  On the `small` frames:
  * rigid poses take the affine path: masks and statistics equal the oracle's (which always divides by w);
  * every pose multiplied by 2 (row 3 = (0, 0, 0, 2)) takes the general path; doubling and halving are
    exact, so the world points, hence the masks, are the rigid run's bit for bit, and the oracle's;
  * doubled and rigid poses alternating inside one batch: the choice is per slot;
  * row 3 = (1e-3, 0, 0, 1): a true homogeneous divide, against the oracle."""
import numpy as np
import pytest

import s1_query_inputs as qi

pytestmark = pytest.mark.gpu

TIERS = [0, 1, 2]
NVOX = 3  # device statistics columns: frame id npix nvox ndbscan nsor -1 ncovered nneighbors kept


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


@pytest.fixture(scope="module")
def frames():
    from maskclustering_amd.synthetic_frames import make_frames_shape
    fr = make_frames_shape("small", seed=0)
    T = np.ascontiguousarray(fr.poses, dtype=np.float64)
    assert np.array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(T), 1))), "the small frames' poses are rigid"
    mixed = T.copy()
    mixed[::2] *= 2.0
    proj = T.copy()
    proj[:, 3, 0] = 1e-3
    poses = {"rigid": T, "doubled": T * 2.0, "mixed": mixed, "projective": proj}
    for a in poses.values():
        a.setflags(write=False)
    base = (fr.scene_points.astype(np.float32), fr.depth, fr.seg, fr.intrinsics)
    return {k: base + (v,) for k, v in poses.items()}


@pytest.fixture(scope="module")
def refs(frames):
    """the oracle's frames per pose set, computed once, read-only"""
    return {k: qi.references(inp) for k, inp in frames.items()}


@pytest.fixture(scope="module")
def rigid_runs():
    return {}


def _rigid(ctx, frames, refs, rigid_runs, tier):
    """the rigid run's masks and statistics under this tier (checked against the oracle), run once"""
    from test_gpu_s1_query import _check
    if tier not in rigid_runs:
        masks, st = _check(ctx, frames["rigid"], refs["rigid"])
        assert len(masks[0]) > 0, "the rigid run keeps no mask"
        rigid_runs[tier] = (masks, st)
    return rigid_runs[tier]


@pytest.mark.parametrize("tier", TIERS)
def test_rigid_poses_match_oracle(ctx, frames, refs, rigid_runs, monkeypatch, tier):
    monkeypatch.setenv("MC_VX_GLOBAL", str(tier))
    masks, st = _rigid(ctx, frames, refs, rigid_runs, tier)
    assert (st[:, NVOX] > 0).any()


@pytest.mark.parametrize("case", ["doubled", "mixed"])
@pytest.mark.parametrize("tier", TIERS)
def test_doubled_poses_take_the_general_path_to_the_same_masks(ctx, frames, refs, rigid_runs, monkeypatch, tier, case):
    from test_gpu_s1_query import _check
    monkeypatch.setenv("MC_VX_GLOBAL", str(tier))
    want, want_st = _rigid(ctx, frames, refs, rigid_runs, tier)
    got, got_st = _check(ctx, frames[case], refs[case])  # (the oracle's masks and statistics of these poses)
    assert len(want[0]) > 0
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(want_st, got_st)


@pytest.mark.parametrize("tier", TIERS)
def test_projective_pose_divides_by_w(ctx, frames, refs, monkeypatch, tier):
    from test_gpu_s1_query import _check
    monkeypatch.setenv("MC_VX_GLOBAL", str(tier))
    masks, st = _check(ctx, frames["projective"], refs["projective"])  # every statistics column and every mask
    assert (st[:, NVOX] > 0).any(), "no slot with voxels"
    rig = refs["rigid"]
    assert any(not np.array_equal(a[3][:, :5], b[3][:, :5]) for a, b in zip(refs["projective"], rig)), \
        "the projective poses give the rigid poses' voxels: the divide is not exercised"
