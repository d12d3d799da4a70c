"""Label images from instance masks without a GPU: the numpy restatement of mask_predict.py:94-113
(tests/label_paint_restatement.py) against the fixture the reference's own program painted
(tests/golden/make_label_paint_golden.py), the properties of the rule, and the overflow at 256 kept."""
import numpy as np
import pytest

import label_paint_restatement as R


def random_frame(rng, n, H, W, dtype=np.uint8):
    yy, xx = np.mgrid[0:H, 0:W]
    c = rng.uniform(0, [H, W], (n, 2))
    r = rng.uniform(1, max(H, W) / 2, n)
    masks = np.stack([((yy - c[i, 0]) ** 2 + (xx - c[i, 1]) ** 2 <= r[i] ** 2) for i in range(n)]).astype(dtype)
    return masks, rng.uniform(0, 1, n).astype(np.float32)


def test_restatement_paints_what_the_reference_painted():
    frames = R.load_golden()
    assert len(frames) == 9
    for k, fr in enumerate(frames):
        image, kept, area = R.paint_frame(fr["masks"], fr["scores"], fr["threshold"])
        assert image.dtype == np.uint8 and image.tobytes() == fr["image"].tobytes(), k


def test_fixture_holds_the_cases_it_is_there_for():
    fr = R.load_golden()
    f32 = np.float32
    # a kept instance fully covered by higher ranks: its id is absent from the image
    img, kept, area = R.paint_frame(fr[0]["masks"], fr[0]["scores"], 0.5)
    assert list(kept) == [2, 1, 3, 0, 4] and area[2] == 400 and 1 not in img and set(np.unique(img)) == {0, 2, 3, 4, 5}
    # 399 is skipped and takes no id, 400 is kept
    img, kept, area = R.paint_frame(fr[1]["masks"], fr[1]["scores"], 0.5)
    assert list(area) == [399, 400, 1920] and list(kept) == [2, 1]
    # at the threshold selected, one ulp below and NaN not, +inf last
    assert fr[2]["scores"][0] == f32(0.5) and fr[2]["scores"][1] == np.nextafter(f32(0.5), f32(0)) and np.isnan(fr[2]["scores"][2])
    assert list(R.paint_frame(fr[2]["masks"], fr[2]["scores"], 0.5)[1]) == [0, 3]
    # nothing selected
    assert not fr[3]["image"].any() and len(R.paint_frame(fr[3]["masks"], fr[3]["scores"], 0.5)[1]) == 0
    # the tie goes by ascending index
    assert fr[4]["scores"][1] == fr[4]["scores"][3] and list(R.paint_frame(fr[4]["masks"], fr[4]["scores"], 0.5)[1]) == [0, 1, 3, 2]
    # float32(0.7) < 0.7, yet it is selected at threshold 0.7
    assert fr[8]["threshold"] == 0.7 and float(fr[8]["scores"][0]) < 0.7
    assert list(R.paint_frame(fr[8]["masks"], fr[8]["scores"], 0.7)[1]) == [0, 2, 3]
    assert {str(f["masks"].dtype) for f in fr} == {"float32", "bool", "uint8"}
    assert {f["image"].shape for f in fr} == {(48, 40), (64, 64)}


@pytest.mark.parametrize("seed", range(4))
def test_ids_present_are_within_the_kept_and_label_instance_follows_the_order(seed):
    rng = np.random.default_rng(seed)
    counts = [0, 7, 1, 20, 0]
    off = np.concatenate([[0], np.cumsum(counts)])
    masks, scores = random_frame(rng, int(off[-1]), 23, 37)
    scores[3] = scores[9] = scores[10]  # ties
    scores[12] = np.nan
    out = R.paint_frames(masks, scores, off, threshold=0.3, min_pixels=30)
    for f in range(len(counts)):
        a, b = off[f], off[f + 1]
        nk = int(out["num_kept"][f])
        row = out["label_instance"][f]
        assert out["status"][f] == R.PAINT_OK and (row[nk:] == -1).all() and len(set(row[:nk])) == nk
        assert set(np.unique(out["labels"][f])) <= set(range(nk + 1))
        s, ar = scores[a:b], out["instance_area"][a:b]
        assert np.array_equal(ar, (masks[a:b] == 1).sum(axis=(1, 2)))
        kept = [i for i in range(b - a) if s[i] >= np.float32(0.3) and ar[i] >= 30]
        assert sorted(row[:nk]) == kept
        for k in range(nk - 1):  # ascending score, ties by ascending index
            i, j = row[k], row[k + 1]
            assert s[i] < s[j] or (s[i] == s[j] and i < j)
        # a pixel's label is the id of the highest kept instance covering it, or 0
        want = np.zeros((23, 37), np.uint8)
        for k in range(nk):
            want[masks[a + row[k]] == 1] = k + 1
        assert np.array_equal(out["labels"][f], want)
        image, kept1, _ = R.paint_frame(masks[a:b], s, 0.3, 30)
        assert np.array_equal(image, out["labels"][f]) and list(kept1) == list(row[:nk])


def test_only_the_value_one_is_a_set_pixel():
    vals = np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0, -1.0, np.nan], np.float32)
    m = np.tile(vals, 4).reshape(1, 4, 6)
    img, kept, area = R.paint_frame(m, [0.9], 0.5, 1)
    assert area[0] == 4 and np.array_equal(img, (m[0] == 1).astype(np.uint8))
    m8 = np.tile(np.array([0, 1, 2, 255], np.uint8), 5).reshape(1, 4, 5)
    img, kept, area = R.paint_frame(m8, [0.9], 0.5, 1)
    assert area[0] == 5 and np.array_equal(img, (m8[0] == 1).astype(np.uint8))


def test_negative_and_positive_zero_scores_tie_by_index():
    m = np.ones((4, 2, 2), np.uint8)
    kept = R.plan_frame(m, np.array([0.0, -0.0, 0.0, -0.0], np.float32), threshold=-1.0, min_pixels=1)[0]
    assert list(kept) == [0, 1, 2, 3]


def test_the_256th_kept_instance_overflows():
    m = np.ones((256, 2, 2), np.uint8)
    s = np.linspace(0.6, 0.9, 256).astype(np.float32)
    image, kept, _ = R.paint_frame(m[:255], s[:255], 0.5, 4)
    assert image.max() == 255 and len(kept) == 255
    with pytest.raises(OverflowError):
        R.paint_frame(m, s, 0.5, 4)
    # numpy itself refuses the 256th id, as for the reference
    with pytest.raises(OverflowError):
        np.zeros((2, 2), np.uint8)[np.ones((2, 2), bool)] = 256
    out = R.paint_frames(np.concatenate([m, m[:3]]), np.concatenate([s, s[:3]]), [0, 256, 259], 0.5, 4)
    assert list(out["status"]) == [R.PAINT_OVERFLOW, R.PAINT_OK] and list(out["num_kept"]) == [256, 3]
    assert not out["labels"][0].any() and (out["label_instance"][0] == -1).all() and out["labels"][1].max() == 3
