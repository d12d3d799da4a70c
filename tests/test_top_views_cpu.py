"""CPU checks of the projected boxes: the numpy restatement (tests/top_views_restatement.py) against
the fixture made by the reference's own code (tests/golden/make_top_views_golden.py), the shared
arithmetic of maskclustering_amd/csrc/mc_proj_plan.hpp (built stand-alone under the address and
undefined-behaviour sanitizers) against the restatement, the top-k selection, the draw clamp and
the request order of ``object_boxes``.  The GPU tests (test_gpu_top_views.py) compare the device
path with the same fixture and restatement."""
import os
import subprocess

import numpy as np
import pytest

import top_views_restatement as R
from conftest import GOLDEN, REPO

FRAGILE_CAP = 0.01       # of the scene set's requests


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "top_views.npz")))


def scene_restatement(z):
    """(boxes [2, n, 4], status [2, n], inside [2, n], fragile [2, n]) of the scene set, both image sizes"""
    w2c = np.stack([np.linalg.inv(e) for e in z["extrinsics"]])
    out = [R.boxes(z["points"], z["obj_pt_off"], z["obj_pts"], z["intrinsics"][s], w2c, int(z["sizes"][s, 0]),
                   int(z["sizes"][s, 1]), z["requests"][:, 0], z["requests"][:, 1]) for s in range(2)]
    return tuple(np.stack([o[i] for o in out]) for i in range(4))


def edge_restatement(z, j):
    n = int(z["edge_npts"][j])
    with np.errstate(all="ignore"):
        w2c = np.linalg.inv(z["edge_ext"][j])
    return R.project(z["edge_pts"][j][:n], w2c, z["edge_intrinsics"], int(z["edge_size"][j, 0]), int(z["edge_size"][j, 1]))


def test_edge_set_equals_reference_exactly(gold):
    z = gold
    for j, name in enumerate(z["edge_name"]):
        st, box, _, _ = edge_restatement(z, j)
        assert st == z["edge_status"][j] and list(box) == list(z["edge_box"][j]), (name, st, box)


def test_scene_set_equals_reference_where_not_fragile(gold):
    z = gold
    boxes, status, _, fragile = scene_restatement(z)
    assert fragile.mean() <= FRAGILE_CAP, fragile.sum()
    keep = ~fragile
    np.testing.assert_array_equal(status[keep], z["status"][keep])
    np.testing.assert_array_equal(boxes[keep], z["boxes"][keep])


def test_fixture_covers_its_cases(gold):
    z = gold
    n_obj = np.diff(z["obj_pt_off"])
    assert len(z["points"]) >= 3000 and len(n_obj) == 8 and len(z["extrinsics"]) == 6
    assert (n_obj > 1000).any() and (n_obj == 1).any() and (n_obj == 0).any()
    assert [tuple(s) for s in z["sizes"]] == [(131, 97), (640, 480)]
    req = [tuple(r) for r in z["requests"]]
    assert len(set(req)) < len(req)                                      # duplicates
    assert set(req) == {(o, f) for o in range(8) for f in range(6)}
    assert set(np.unique(z["status"])) == {R.OK, R.BEHIND, R.OUTSIDE}
    boxes, status, inside, _ = scene_restatement(z)
    whole = cut = False
    for s in range(2):
        W, H = z["sizes"][s]
        for j, (o, f) in enumerate(req):
            if status[s, j] == R.OK and n_obj[o] > 1:
                touches = boxes[s, j, 0] == 0 or boxes[s, j, 1] == 0 or boxes[s, j, 2] == W - 1 or boxes[s, j, 3] == H - 1
                whole |= inside[s, j] == n_obj[o] and not touches
                cut |= inside[s, j] < n_obj[o] and touches
    assert whole and cut
    by_obj = {o: {z["status"][0][j] for j, r in enumerate(req) if r[0] == o} for o in range(8)}
    assert by_obj[4] == {R.BEHIND} and R.BEHIND in by_obj[5] and R.OK in by_obj[5] and R.OUTSIDE in by_obj[6]
    # the edge values land where the half-to-even rule puts them
    edge = {str(n): (int(s), [int(v) for v in b]) for n, s, b in zip(z["edge_name"], z["edge_status"], z["edge_box"])}
    for pose in ("id", "perm"):
        assert edge[f"{pose} x=-0.26 w=131"][0] == R.OUTSIDE                       # u = -0.52 -> -1
        assert edge[f"{pose} x=-0.25 w=131"] == (R.OK, [0, 0, 0, 0])                 # u = -0.5 -> -0.0: pixel 0
        assert edge[f"{pose} x=0.75 w=131"] == (R.OK, [2, 0, 2, 0])                  # 1.5 -> 2
        assert edge[f"{pose} x=1.25 w=131"] == (R.OK, [2, 0, 2, 0])                  # 2.5 -> 2
        assert edge[f"{pose} x=65.25 w=131"] == (R.OK, [130, 0, 130, 0])             # 130.5 -> 130, in at 131
        assert edge[f"{pose} x=65.25 w=8"][0] == R.OUTSIDE
        assert edge[f"{pose} x=319.75 w=640"][0] == R.OUTSIDE                       # 639.5 -> 640: out
        assert edge[f"{pose} y=319.75 h=640"][0] == R.OUTSIDE
        assert edge[f"{pose} y=65.25 h=131"] == (R.OK, [0, 130, 0, 130])
        assert edge[f"{pose} z=0.0"][0] == R.BEHIND and edge[f"{pose} z=-1.0"][0] == R.BEHIND
        assert edge[f"{pose} z=1e-320"] == (R.OK, [0, 0, 0, 0])                      # 0 / tiny = 0
        assert edge[f"{pose} z=1e-320 x=1"][0] == R.OUTSIDE                         # 1 / tiny = inf
        assert edge[f"{pose} empty"][0] == R.BEHIND
    assert edge["all -inf"][0] == R.BEHIND                                           # a NaN z is not > 0
    assert set(z["clamps"][:, 6]) == {2, 5}


@pytest.mark.parametrize("k", [1, 5, 9, 16])
def test_top_k_equals_python_sort(k):
    rng = np.random.default_rng(k)
    lists = [[], [0.5], [0.3, 0.3], [0.2, 0.9, 0.9, 0.2, 0.9], list(rng.integers(0, 4, 40) / 4.0), list(rng.random(7)),
             list(rng.integers(0, 3, 12) / 2.0)]
    for cov in lists:
        entries = [(i, c) for i, c in enumerate(cov)]
        want = [i for i, _ in sorted(entries, key=lambda e: e[1], reverse=True)[:k]]
        assert list(R.top_k(cov, k)) == want, (cov, k)
    off = np.concatenate([[0], np.cumsum([len(c) for c in lists])])
    cov = np.concatenate([np.asarray(c, np.float64) for c in lists])
    frame = np.arange(len(cov)) * 3 % 11
    pos, fr = R.top_requests(off, cov, frame, k)
    assert pos.shape == (len(lists), k)
    for f, c in enumerate(lists):
        m = min(k, len(c))
        assert list(pos[f, :m]) == list(R.top_k(c, k)) and (pos[f, m:] == -1).all() and (fr[f, m:] == -1).all()
        assert list(fr[f, :m]) == [frame[off[f] + p] for p in pos[f, :m]]


def test_clamp_equals_recorded_rectangle_arguments(gold):
    from maskclustering_amd import top_images
    for row in gold["clamps"]:
        bbox, (W, H, t), want = tuple(int(v) for v in row[:4]), (int(v) for v in row[4:7]), [int(v) for v in row[7:]]
        for fn in (R.draw_clamp, top_images.clip_draw_box):
            p0, p1 = fn(bbox, W, H, t)
            assert [*p0, *p1] == want, (fn.__module__, bbox, W, H, t)
    assert (gold["clamps"][:, 7] > gold["clamps"][:, 9]).any()              # min > max after clamping occurs


def test_object_boxes_issues_requests_in_the_reference_order(monkeypatch):
    from maskclustering_amd import _device, top_images
    seen = {}

    class FakeContext:
        def proj_boxes(self, points, off, ids, k, w2c, width, height, req_object, req_frame):
            seen.update(points=points, off=off, ids=ids, k=k, w2c=w2c, size=(width, height), obj=list(req_object),
                        frame=list(req_frame))
            n = len(req_object)
            status = np.array([j % 3 for j in range(n)], np.int32)
            return np.arange(4 * n, dtype=np.int32).reshape(n, 4), status, np.zeros(n, np.int32)

    monkeypatch.setattr(_device, "context", lambda: FakeContext())
    masks = lambda frames: [(f, 1, 0.9 - 0.01 * i) for i, f in enumerate(frames)]  # noqa: E731
    od = {7: {"point_ids": [4, 2], "mask_list": masks([30, 10, 30])},
          3: {"point_ids": [1], "mask_list": []},
          5: {"point_ids": np.array([0, 3, 5]), "mask_list": masks(range(0, 120, 10))}}
    ext = {f: np.eye(4) for f in range(0, 120, 10)}                              # camera -> world: shifted by f along x
    for f in ext:
        ext[f][0, 3] = f
    out = top_images.object_boxes(od, np.zeros((6, 3)), lambda f: (100.0 + f, 100.0, 5.0, 6.0), ext, 131, 97, top_k=9)
    want = [(7, 30), (7, 10), (7, 30)] + [(5, f) for f in range(0, 90, 10)]      # object order, mask_list[:9], 3 skipped
    assert [(k, f) for k, f, _ in out] == want
    assert seen["obj"] == [0, 0, 0] + [1] * 9 and list(seen["off"]) == [0, 2, 5] and list(seen["ids"]) == [4, 2, 0, 3, 5]
    frames = [30, 10] + [f for f in range(0, 90, 10) if f not in (30, 10)]       # distinct, in order of first use
    assert [frames[i] for i in seen["frame"]] == [f for _, f in want]
    np.testing.assert_array_equal(seen["k"][:, 0], [100.0 + f for f in frames])
    np.testing.assert_array_equal(seen["w2c"][:, 0, 3], [-float(f) for f in frames])  # inverted on the host
    assert seen["size"] == (131, 97)
    assert [b for _, _, b in out] == [tuple(range(4 * j, 4 * j + 4)) if j % 3 == 0 else None for j in range(len(want))]
    assert top_images.object_boxes({1: {"point_ids": [0], "mask_list": []}}, np.zeros((1, 3)), {}, {}, 8, 8) == []


def _hex(v):
    return float(v).hex()


def test_plan_header_equals_restatement(tmp_path, gold):
    exe = tmp_path / "proj_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(REPO, "maskclustering_amd", "csrc"), os.path.join(REPO, "scripts", "proj_plan_check.cpp"),
                           "-o", str(exe)])
    z = gold
    cases = []                                                             # (points, w2c, k, W, H)
    w2c = np.stack([np.linalg.inv(e) for e in z["extrinsics"]])
    for s in range(2):
        for o, f in z["requests"]:
            ids = z["obj_pts"][z["obj_pt_off"][o]:z["obj_pt_off"][o + 1]]
            cases.append((z["points"][ids], w2c[f], z["intrinsics"][s, f], int(z["sizes"][s, 0]), int(z["sizes"][s, 1])))
    for j in range(len(z["edge_name"])):
        with np.errstate(all="ignore"):
            m = np.linalg.inv(z["edge_ext"][j])
        cases.append((z["edge_pts"][j][:int(z["edge_npts"][j])], m, z["edge_intrinsics"], int(z["edge_size"][j, 0]),
                      int(z["edge_size"][j, 1])))
    big = np.array([[1e308, 1e308, 1e-308], [-1e308, 3.0, 1e-300], [np.nan, 1.0, 1.0], [1.0, np.inf, 2.0], [2.5, -2.5, 1.0],
                    [2 ** 31 / 2.0, 0.0, 1.0], [2 ** 40, 2 ** 40, 1.0]])
    k2 = np.array([2.0, 2.0, 0.0, 0.0])
    cases += [(big, np.eye(4), k2, 2 ** 30, 2 ** 30), (big[4:], np.eye(4), k2, 1, 1), (big, np.full((4, 4), np.nan), k2, 8, 8)]
    clamps = [tuple(int(v) for v in row[:7]) for row in z["clamps"]]
    text = []
    for p, m, k, W, H in cases:
        text.append(f"P {W} {H} {len(p)} " + " ".join(_hex(v) for v in np.asarray(m).ravel()) + " " + " ".join(_hex(v) for v in k))
        text += [" ".join(_hex(v) for v in row) for row in np.asarray(p, np.float64).reshape(-1, 3)]
    text += ["C " + " ".join(str(v) for v in c) for c in clamps]
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    lines = iter(r.stdout.splitlines())
    for i, (p, m, k, W, H) in enumerate(cases):
        st, box, ins, _ = R.project(p, m, k, W, H)
        assert next(lines).split() == ["P", str(st), *(str(v) for v in box), str(ins)], i
    for c in clamps:
        p0, p1 = R.draw_clamp(c[:4], *c[4:])
        assert next(lines).split() == ["C", *(str(v) for v in (*p0, *p1))], c
    assert next(lines, None) is None


def test_shim_routes_the_reference_module(tmp_path, monkeypatch):
    """python -m maskclustering_amd.top_images: the module named get_top_images on the path gets our
    get_bbox_by_projection, then its own main() runs"""
    import sys
    from maskclustering_amd import top_images
    (tmp_path / "get_top_images.py").write_text(
        "CALLS = []\n"
        "def get_bbox_by_projection(pcd, intr, ext):\n    return 'theirs'\n"
        "def main():\n    CALLS.append(get_bbox_by_projection)\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    monkeypatch.delitem(sys.modules, "get_top_images", raising=False)
    top_images.main()
    assert sys.modules["get_top_images"].CALLS == [top_images.get_bbox_by_projection]
    monkeypatch.delitem(sys.modules, "get_top_images", raising=False)
