"""Scene point cloud fusion without a GPU: the numpy restatement (tests/scene_cloud_restatement.py)
against the C oracle's voxel_down_sample, the flush schedule, the PLY writer read back, and the
golden made by the reference's own create_downsampled_point_cloud
(tests/golden/make_scene_cloud_golden.py), which pins the glue: frame order, stride, flush rule,
remainder, final pass."""
import os

import numpy as np
import pytest

import scene_cloud_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))


def golden_frames():
    """The golden's frames as the reference lists them: ids by integer value, then [::stride]."""
    g = np.load(os.path.join(HERE, "golden", "scene_cloud_golden.npz"))
    names = [str(n) for n in g["names"]]
    order = sorted(range(len(names)), key=lambda i: int(names[i].split(".")[0]))[::int(g["stride"])]
    depth = (g["depth_u16"][order].astype(np.float64) / float(g["depth_scale"])).astype(np.float32)
    m = g["intrinsic"]
    K = np.tile(np.array([m[0, 0], m[1, 1], m[0, 2], m[1, 2]]), (len(order), 1))
    return g, depth, g["rgb"][order], K, g["poses"][order]


def test_restatement_voxel_down_sample_equals_the_oracle_bit_for_bit():
    from oracle import oracle
    depth, rgb, K, T = R.synthetic_frames(3, 48, 64, seed=3)
    pts = np.concatenate([R.frame_points(depth[f], rgb[f], K[f], T[f])[0] for f in range(3)])
    for voxel in (0.005, 0.05, 0.5, 5.0):
        want = oracle.s1_voxel(pts, voxel)
        got, _, cnt = R.voxel_down_sample(pts, None, voxel)
        assert got.shape == want.shape and int(cnt.sum()) == len(pts)
        assert got.tobytes() == want.tobytes(), voxel  # means and order


def test_left_fold_differs_from_pairwise_sum_so_the_order_is_observable():
    depth, rgb, K, T = R.synthetic_frames(3, 48, 64, seed=3)
    pts = np.concatenate([R.frame_points(depth[f], rgb[f], K[f], T[f])[0] for f in range(3)])
    got, _, cnt = R.voxel_down_sample(pts, None, 50.0)
    assert len(cnt) == 1 and cnt[0] == len(pts) > 5000
    pairwise = np.array([np.ascontiguousarray(pts[:, r]).sum() for r in range(3)])  # numpy's pairwise sum
    assert (pairwise / len(pts)).tobytes() != got[0].tobytes()


@pytest.mark.parametrize("F,B,want", [(7, 3, [(0, 3), (3, 6), (6, 7)]), (6, 3, [(0, 3), (3, 6)]), (2, 3, [(0, 2)]),
                                      (3, 1, [(0, 1), (1, 2), (2, 3)]), (0, 3, [])])
def test_flush_schedule(F, B, want):
    assert R.flush_schedule(F, B) == want


def test_depth_edges_of_the_validity_rule():
    d = np.array([[0.0, -1.0, np.nan, np.inf, 20.0, np.nextafter(np.float32(20.0), np.float32(0.0)), 1.0]], np.float32)
    assert R.valid_pixels(d).tolist() == [[False, False, False, False, False, True, True]]


def test_write_ply_reads_back(tmp_path):
    from maskclustering_amd.scene_cloud import write_ply
    rng = np.random.default_rng(0)
    p = rng.standard_normal((17, 3)) * 100
    c = rng.random((17, 3))
    c[0] = (0.0, 1.0, 0.5)
    c[1] = (-0.25, 1.5, 0.4999 / 255)
    path = tmp_path / "cloud.ply"
    write_ply(str(path), p, c)
    raw = path.read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and "element vertex 17" in lines
    props = [ln for ln in lines if ln.startswith("property")]
    assert props == ["property double x", "property double y", "property double z", "property uchar red",
                     "property uchar green", "property uchar blue"]
    rec = np.frombuffer(body, dtype=[("p", "<f8", 3), ("c", "u1", 3)])
    assert len(rec) == 17 and rec["p"].tobytes() == p.tobytes()
    assert np.array_equal(rec["c"], np.round(np.clip(c, 0, 1) * 255).astype(np.uint8))
    assert rec["c"][0].tolist() == [0, 255, 128] and rec["c"][1].tolist() == [0, 255, 0]
    write_ply(str(path), np.zeros((0, 3)), np.zeros((0, 3)))
    assert path.read_bytes().endswith(b"end_header\n")


def test_golden_of_the_reference_function_pins_the_glue():
    g, depth, rgb, K, T = golden_frames()
    assert [str(n) for n in g["names"]] != sorted((str(n) for n in g["names"]), key=lambda s: int(s.split(".")[0]))
    assert len(depth) == 4 and int(g["buffer_size"]) == 3  # a full buffer and a remainder of one frame
    info = {}
    p, c = R.fuse_frames(depth, rgb, K, T, float(g["voxel_size"]), int(g["buffer_size"]), info=info)
    assert p.tobytes() == g["points"].tobytes() and c.tobytes() == g["colors"].tobytes()
    assert len(info["sizes"]) == 3
    # the order of the frames, the stride and the buffers are observable: other choices give other bytes
    q, _ = R.fuse_frames(depth[::-1], rgb[::-1], K[::-1], T[::-1], float(g["voxel_size"]), 3)
    assert q.tobytes() != p.tobytes()
    q, _ = R.fuse_frames(depth, rgb, K, T, float(g["voxel_size"]), 4)
    assert q.tobytes() != p.tobytes()


def test_read_scene_frames_orders_by_integer_and_refuses_another_colour_size(tmp_path):
    from PIL import Image
    from maskclustering_amd.scene_cloud import read_scene_frames
    depth, rgb, K, T = R.synthetic_frames(3, 6, 8, seed=5)
    for sub in ("depth", "color", "pose", "intrinsic"):
        os.makedirs(tmp_path / sub)
    m = np.eye(4)
    m[0, 0], m[1, 1], m[0, 2], m[1, 2] = K[0]
    np.savetxt(tmp_path / "intrinsic" / "intrinsic_depth.txt", m)
    ids = ["10", "2", "7"]
    for k, fid in enumerate(ids):
        Image.fromarray(np.round(depth[k].astype(np.float64) * 1000).astype(np.uint16)).save(tmp_path / "depth" / f"{fid}.png")
        Image.fromarray(rgb[k]).save(tmp_path / "color" / f"{fid}.jpg", format="PNG")
        np.savetxt(tmp_path / "pose" / f"{fid}.txt", T[k])
    got_ids, d, c, kk, tt = read_scene_frames(str(tmp_path), stride=2)
    assert got_ids == ["2", "10"]  # 2, 7, 10 by integer value, then every second
    assert d.dtype == np.float32 and d.shape == (2, 6, 8) and c.tobytes() == rgb[[1, 0]].tobytes()
    want = (np.round(depth[[1, 0]].astype(np.float64) * 1000).astype(np.uint16).astype(np.float64) / 1000).astype(np.float32)
    assert d.tobytes() == want.tobytes() and tt.tobytes() == T[[1, 0]].tobytes() and kk.tobytes() == K[[0, 0]].tobytes()
    Image.fromarray(rgb[0][:3]).save(tmp_path / "color" / "2.jpg", format="PNG")
    with pytest.raises(ValueError, match="resize"):
        read_scene_frames(str(tmp_path))
