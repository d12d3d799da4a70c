"""Export and merge of the AP accumulation (mc_ev_state_info / _export / _merge, include/mcgraph.h) and
the gather over ranks built on them (SceneSweep.evaluation(group), save_evaluation / load_evaluation).

The table is a function of each cell's multiset of (score, true) examples, its hard false negative
count and its flags alone (tests/test_ap_cpu.py), so a merged accumulation's table, stats, curves
and state buffer equal the single context's exactly: every comparison here is assert_array_equal,
NaN positions included.  Against tests/ap_restatement.py the AP keeps the bound of
tests/test_gpu_ap.py (n * 2^-52); the buffer's integers are exact."""
import functools

import numpy as np
import pytest

import ap_restatement as R
import ap_state_util as U
from test_gpu_ap import CLS, begin_golden, caps, check_result, golden, lists, new_ctx

pytestmark = pytest.mark.gpu

MODES = ("ca", "nc")
SPLITS = {"01|23": ((0, 1), (2, 3)), "0|123": ((0,), (1, 2, 3)), "|0123": ((), (0, 1, 2, 3)), "0|1|23": ((0,), (1,), (2, 3))}


def scan_args(s):
    z = golden()
    return [z[f"s{s}_gt"], z[f"s{s}_off"], z[f"s{s}_pts"], z[f"s{s}_classes"], z[f"s{s}_scores"]]


def golden_ctx(mode, scans):
    ctx = new_ctx()
    begin_golden(ctx, mode)
    for s in scans:
        ctx.ev_add_scan(*scan_args(s))
    return ctx


def snapshot(ctx):
    """(ap, stats, {cell: curve}, state bytes) of a context."""
    ap, stats = ctx.ev_ap()
    C, O = ap.shape
    curves = {(c, o): ctx.ev_curve(c, o) for c in range(C) for o in range(O) if stats[c, o, 0]}
    return ap, stats, curves, ctx.ev_state()


def assert_same(got, want, msg=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{msg} ap")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{msg} stats")
    assert set(got[2]) == set(want[2]), f"{msg} cells with examples"
    for cell in want[2]:
        for a, b, k in zip(got[2][cell], want[2][cell], ("score", "tp", "fp", "fn")):
            np.testing.assert_array_equal(a, b, err_msg=f"{msg} cell {cell} {k}")
    np.testing.assert_array_equal(got[3], want[3], err_msg=f"{msg} state bytes")


@functools.lru_cache(maxsize=None)
def single(mode):
    """All four golden scans in one context: its snapshot, and the scans' tables."""
    ctx = new_ctx()
    begin_golden(ctx, mode)
    tables = []
    for s in range(4):
        ctx.ev_add_scan(*scan_args(s))
        tables.append(ctx.ev_scan())
    return snapshot(ctx), tables


@functools.lru_cache(maxsize=None)
def restatement(mode):
    z = golden()
    rs = R.APRestatement(z["class_ids"], z["overlaps"], int(z["min_region_size"]), mode == "nc")
    for s in range(4):
        rs.add_scan(*scan_args(s))
    return rs


def state_of(ctx, device):
    st = ctx.ev_state(device=device)
    if device:
        import torch
        assert st.device.type == "cuda" and st.dtype == torch.uint8 and st.numel() == ctx.ev_state_info()[2]
    return st


# ---- 1 + 3. merge equals one context, host and device buffers ---------------------------------------
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("mode", MODES)
def test_merge_equals_one_context(mode, split, device):
    want, _ = single(mode)
    parts = [golden_ctx(mode, scans) for scans in SPLITS[split]]
    states = [state_of(p, device) for p in parts]
    last = [p.ev_scan() if scans else None for p, scans in zip(parts, SPLITS[split])]
    # into the first part, which holds scans already (none for the split with an empty side)
    for st in states[1:]:
        parts[0].ev_merge_state(st)
    assert_same(snapshot(parts[0]), want, f"{mode} {split} into part 0")
    if last[0] is not None:                               # a merge is no scan
        R.assert_tables_equal(parts[0].ev_scan(), last[0], "last scan after merges")
    # into a context that has only begun
    fresh = golden_ctx(mode, ())
    for st in states:
        fresh.ev_merge_state(st)
    assert_same(snapshot(fresh), want, f"{mode} {split} into a fresh context")
    # the exporters are unchanged and go on growing
    for p, st in zip(parts[1:], states[1:]):
        np.testing.assert_array_equal(p.ev_state(), st.cpu().numpy() if device else st)
    if split == "01|23":
        for s in (0, 1):
            parts[1].ev_add_scan(*scan_args(s))
        got = snapshot(parts[1])
        np.testing.assert_array_equal(got[3], want[3])
        np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("mode", MODES)
def test_merge_equals_replaying_the_tables(mode):
    want, tables = single(mode)
    ctx = golden_ctx(mode, ())
    for t in tables:
        ctx.ev_add_matches(t)
    assert_same(snapshot(ctx), want, f"{mode} add_matches replay")


# ---- 2 + 3. the canonical form ---------------------------------------------------------------------
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("mode", MODES)
def test_state_is_canonical_and_equals_the_restatement(mode, device):
    want, _ = single(mode)
    rs = restatement(mode)
    np.testing.assert_array_equal(want[3], U.expected_state(rs))
    st = U.parse_state(want[3])
    assert st["word"] == U.STATE_WORD and st["R"] == len(st["key"]) > 0
    assert (st["n_true"].astype(np.int64) + st["n_false"] >= 1).all()
    assert (np.diff(st["run_off"]) > 1).any()             # a cell with several distinct scores
    # export -> merge into a fresh context -> export is the identity
    src = golden_ctx(mode, (0, 1, 2, 3))
    buf = state_of(src, device)
    fresh = golden_ctx(mode, ())
    assert fresh.ev_state_info() == (0, 0, len(U.build_state(dict(st, R=0, key=[], n_true=[], n_false=[]))))
    fresh.ev_merge_state(buf)
    got = state_of(fresh, device)
    np.testing.assert_array_equal(got.cpu().numpy() if device else got, want[3])
    r, e, b = fresh.ev_state_info()
    assert (r, e, b) == (st["R"], int(want[1][:, :, 0].sum()), len(want[3]))
    check_result(fresh, rs.result()[0], rs.result(), f"{mode} merged")


def test_info_and_export_sizes():
    from maskclustering_amd._native import McError
    ctx = new_ctx()
    with pytest.raises(McError) as e:
        ctx.ev_state_info()
    assert e.value.code == 3                              # MC_ERR_STATE
    ctx = golden_ctx("ca", (0,))
    n = ctx.ev_state_info()[2]
    import ctypes
    small = np.zeros(n - 8, np.uint8)
    assert ctx.L.mc_ev_state_export(ctx.h, ctypes.c_void_p(small.ctypes.data), n - 8, 0) == 1   # MC_ERR_INVALID
    t = ctx.ev_scan()
    a = ctx.ev_state()
    R.assert_tables_equal(ctx.ev_scan(), t, "export is no scan")
    np.testing.assert_array_equal(ctx.ev_state(), a)


# ---- 4. sizes where it can go wrong ------------------------------------------------------------------
def many_predictions(K, scores, ngt=40):
    """tests/test_gpu_ap.py::test_cell_with_one_more_example_than_the_lds_sort's scan: K examples per overlap."""
    return dict(gt_cls=np.full(ngt, 1, np.int32), gt_id=(CLS[1] * 1000 + 1 + np.arange(ngt)).astype(np.int32),
                gt_vert=np.full(ngt, 150, np.int64), pr_cls=np.full(K, 1, np.int32), pr_vert=np.full(K, 150, np.int64),
                pr_void=np.zeros(K, np.int64), pr_score=np.asarray(scores, np.float64),
                pair_pred=np.r_[np.arange(ngt), ngt].astype(np.int32), pair_gt=np.r_[np.arange(ngt), 0].astype(np.int32),
                pair_int=np.full(ngt + 1, 150, np.int64))


def merge_twice_and_check(t):
    """The scan in one context, exported; a second context holding the same scan merges it: the
    restatement fed the scan twice."""
    a, b = new_ctx(), new_ctx()
    rs = R.APRestatement(CLS, None, 100, False)
    for ctx in (a, b):
        ctx.ev_begin(CLS, None, 100, False)
        ctx.ev_add_matches(t)
        rs.add_tables(t)
    st = a.ev_state()
    b.ev_merge_state(st)
    res = rs.result()
    check_result(b, res[0], res)
    np.testing.assert_array_equal(b.ev_state(), U.expected_state(rs))
    return U.parse_state(st), U.parse_state(b.ev_state())


@pytest.mark.parametrize("scores", ("distinct", "equal"))
@pytest.mark.parametrize("extra", (0, 1), ids=("cap", "cap+1"))
def test_cells_at_the_lds_sort_limit(extra, scores):
    n = caps()[1] + extra
    rng = np.random.default_rng(5)
    sc = rng.permutation(n).astype(np.float64) / n if scores == "distinct" else np.ones(n)
    one, two = merge_twice_and_check(many_predictions(n, sc))
    O = one["O"]
    per_cell = np.diff(one["run_off"])[O:2 * O]           # class index 1
    assert (per_cell == (n if scores == "distinct" else 1)).all()
    cnt = one["n_true"].astype(np.int64) + one["n_false"]
    assert cnt.sum() == n * O and (two["n_true"].astype(np.int64) + two["n_false"]).sum() == 2 * n * O
    if scores == "equal":
        assert (cnt == n).all()


def test_run_boundaries_on_multiples_of_256():
    K = 600
    sc = np.r_[np.full(256, 0.2), np.full(256, 0.5), np.full(K - 512, 0.7)]
    one, two = merge_twice_and_check(many_predictions(K, sc))
    O = one["O"]
    assert (np.diff(one["run_off"])[O:2 * O] == 3).all()
    cnt = (one["n_true"].astype(np.int64) + one["n_false"]).reshape(O, 3)
    assert (cnt == (256, 256, K - 512)).all()              # run boundaries at examples 256 and 512
    assert ((two["n_true"].astype(np.int64) + two["n_false"]).reshape(O, 3) == (512, 512, 2 * (K - 512))).all()


def small_scans():
    """The scans of tests/test_gpu_ap.py::test_small_and_empty_scans."""
    P = 900
    gt = np.zeros(P, np.int32)
    gt[:300] = CLS[0] * 1000 + 1
    gt[300:500] = CLS[2] * 1000 + 2
    gt[500:560] = CLS[2] * 1000 + 3
    gt[600:700] = 999 * 1000 + 4
    none = lists()
    one = lists(np.arange(0, 280))
    c = lambda *x: np.array(x, np.int32)                 # noqa: E731
    f = lambda *x: np.array(x, np.float64)               # noqa: E731
    return [(gt, *none, c(), f()), (np.zeros(P, np.int32), *one, c(CLS[0]), f(0.5)), (gt, *one, c(CLS[0]), f(0.8)),
            (gt, *lists(np.arange(300, 399), np.arange(300, 400), np.arange(500, 700)), c(CLS[2], CLS[2], CLS[2]),
             f(0.3, 0.6, 0.9))]


@pytest.mark.parametrize("no_class", (False, True), ids=("ca", "nc"))
def test_ground_truth_on_one_side_predictions_on_the_other(no_class):
    scans = small_scans()
    rs = R.APRestatement(CLS, None, 100, no_class)
    sides = []
    for group in ((0,), (1,), (2, 3)):                   # ground truth without predictions | predictions without ground truth | the rest
        ctx = new_ctx()
        ctx.ev_begin(CLS, None, 100, no_class)
        for i in group:
            ctx.ev_add_scan(*scans[i])
        sides.append(ctx)
    for sc in scans:
        rs.add_scan(*sc)
    gt_side, pred_side = U.parse_state(sides[0].ev_state()), U.parse_state(sides[1].ev_state())
    assert gt_side["R"] == 0 and (gt_side["hard_fn"] > 0).any() and set(gt_side["flags"].tolist()) == {0, 1}
    assert (pred_side["flags"] & 2).any() and (no_class or (set(pred_side["flags"].tolist()) == {0, 2} and
                                                            not pred_side["hard_fn"].any()))
    merged = new_ctx()
    merged.ev_begin(CLS, None, 100, no_class)
    for ctx in (sides[2], sides[0], sides[1]):
        merged.ev_merge_state(ctx.ev_state())
    res = rs.result()
    check_result(merged, res[0], res, "three sides")
    np.testing.assert_array_equal(merged.ev_state(), U.expected_state(rs))
    # the pair alone: has_gt from one side and has_pred from the other meet in the cells of class index 0
    pair = new_ctx()
    pair.ev_begin(CLS, None, 100, no_class)
    pair.ev_merge_state(sides[0].ev_state())
    before = pair.ev_ap()[1]
    pair.ev_merge_state(sides[1].ev_state())
    stats = pair.ev_ap()[1]
    np.testing.assert_array_equal(stats[:, :, 3].ravel(), gt_side["flags"] | pred_side["flags"])
    np.testing.assert_array_equal(stats[:, :, 2].ravel(), gt_side["hard_fn"] + pred_side["hard_fn"])
    assert (before[:, :, 3] != 3).all() and (stats[0, :, 3] == 3).all() and (stats[0, :, 2] > 0).all()


def test_empty_state_changes_nothing():
    ctx = golden_ctx("ca", (0, 1))
    before = snapshot(ctx)
    empty = golden_ctx("ca", ()).ev_state()
    assert U.parse_state(empty)["R"] == 0
    ctx.ev_merge_state(empty)
    assert_same(snapshot(ctx), before, "after an empty state")


# ---- 5. errors leave the accumulation as it was ------------------------------------------------------
def patched(buf, **sections):
    """A valid buffer with sections (or header entries) replaced: values, or a function of the section."""
    st = U.parse_state(buf)
    for k, v in sections.items():
        st[k] = v(st[k].copy()) if callable(v) else v
    return U.build_state(st)


def first_cell_with_runs(st, n):
    return int(np.flatnonzero(np.diff(st["run_off"]) >= n)[0])


def test_rejected_merges_leave_the_accumulation():
    from maskclustering_amd._native import McError
    import torch
    z = golden()
    INVALID, STATE, UNSUPPORTED = 1, 3, 5
    ids, ov, mrs = z["class_ids"], np.asarray(z["overlaps"], np.float64), int(z["min_region_size"])
    good = golden_ctx("ca", (2, 3)).ev_state()
    st = U.parse_state(good)
    with pytest.raises(McError) as e:                     # before ev_begin
        new_ctx().ev_merge_state(good)
    assert e.value.code == STATE

    def other(**kw):
        cfg = dict(class_ids=ids, overlaps=ov, min_region_size=mrs, no_class=False)
        cfg.update(kw)
        ctx = new_ctx()
        ctx.ev_begin(cfg["class_ids"], cfg["overlaps"], cfg["min_region_size"], cfg["no_class"])
        return ctx.ev_state()

    ov_bit = ov.copy()
    ov_bit[3] = np.nextafter(ov_bit[3], 1.0)              # one overlap differing in its last bit
    c2 = first_cell_with_runs(st, 2)
    r2 = int(st["run_off"][c2])

    def swap(a):
        a[r2], a[r2 + 1] = a[r2 + 1], a[r2]
        return a

    def set_at(i, v):
        def f(a):
            a[i] = v
            return a
        return f

    def descending(a):
        a[c2 + 1] = a[c2] - 1 if a[c2] > 0 else a[-1] + 1
        return a

    nan_key = U.key_of(1.0) | 0x7FF8000000000000          # a positive NaN's bits, as ev_key would map them
    cases = {
        "class table": (other(class_ids=np.r_[ids[1], ids[0], ids[2:]]), INVALID),
        "one class fewer": (other(class_ids=ids[:-1]), INVALID),
        "overlap bit": (other(overlaps=ov_bit), INVALID),
        "min_region_size": (other(min_region_size=mrs + 1), INVALID),
        "no_class": (other(no_class=True), INVALID),
        "truncated": (good[:-8], INVALID),
        "header only half": (good[:40], INVALID),
        "magic": (patched(good, word=U.STATE_WORD ^ 1), INVALID),
        "version": (patched(good, word=U.STATE_WORD + (1 << 32)), INVALID),
        "run_off descending": (patched(good, run_off=descending), INVALID),
        "run_off not from 0": (patched(good, run_off=set_at(0, 1)), INVALID),
        "run_off not to R": (patched(good, run_off=set_at(-1, st["R"] - 1)), INVALID),
        "equal neighbouring keys": (patched(good, key=set_at(r2 + 1, st["key"][r2])), INVALID),
        "descending keys": (patched(good, key=swap), INVALID),
        "zero-count run": (patched(good, n_true=set_at(r2, 0), n_false=set_at(r2, 0)), INVALID),
        "NaN key": (patched(good, key=set_at(int(st["run_off"][c2 + 1]) - 1, nan_key)), INVALID),
        "key of -0.0": (patched(good, key=set_at(r2, 0x7FFFFFFFFFFFFFFF)), INVALID),
        "extra flag bit": (patched(good, flags=set_at(c2, 4 | 3)), INVALID),
        "negative hard_fn": (patched(good, hard_fn=set_at(c2, -1)), INVALID),
        "R larger than the buffer": (patched(good, R=st["R"] + 1), INVALID),
        "R huge": (patched(good, R=2 ** 40), INVALID),
        "R negative": (patched(good, R=-1), INVALID),
        "2^31 examples in a run": (patched(good, n_true=set_at(r2, 2 ** 31)), UNSUPPORTED),
        "2^31 examples with the accumulation's": (patched(good, n_true=set_at(r2, 2 ** 31 - 1 - int(st["n_false"][r2]))),
                                                  UNSUPPORTED),
    }
    assert np.isnan(np.uint64(nan_key & (2 ** 63 - 1)).view(np.float64))
    ctx = golden_ctx("ca", (0, 1))
    before = snapshot(ctx)
    last = ctx.ev_scan()
    for name, (buf, code) in cases.items():
        for device in (False, True):
            b = torch.from_numpy(np.ascontiguousarray(buf)).to("cuda:0") if device else buf
            with pytest.raises(McError) as e:
                ctx.ev_merge_state(b)
            assert e.value.code == code, f"{name} ({'device' if device else 'host'}): {e.value}"
        assert_same(snapshot(ctx), before, name)
    R.assert_tables_equal(ctx.ev_scan(), last, "last scan after rejected merges")
    ctx.ev_merge_state(good)                              # and the valid buffer still merges
    assert_same(snapshot(ctx), single("ca")[0], "after the rejected merges")


# ---- 6. ranks ----------------------------------------------------------------------------------------
def check_ranks(outs, want_ap, want_stats, own, overlaps):
    """Rank 0 has the table from both calls, the others None from the first and the table from the
    broadcast; every rank's own accumulation is as it was (own: rank -> (ap, stats) or None)."""
    import warnings
    with warnings.catch_warnings():                       # nanmean over classes without ground truth
        warnings.simplefilter("ignore", RuntimeWarning)
        avg = R.compute_averages(want_ap, overlaps, [])
    for r, path in enumerate(outs):
        got = np.load(path)
        assert bool(got["dst_none"]) == (r != 0) and not bool(got["bc_none"])
        for name in ("dst", "bc") if r == 0 else ("bc",):
            np.testing.assert_array_equal(got[name + "_ap"], want_ap, err_msg=f"rank {r} {name}")
            np.testing.assert_array_equal(got[name + "_stats"], want_stats, err_msg=f"rank {r} {name}")
            np.testing.assert_array_equal(got[name + "_avg"], [avg["all_ap"], avg["all_ap_50%"], avg["all_ap_25%"]])
        if own is not None:
            np.testing.assert_array_equal(got["own_stats"], own[r][1], err_msg=f"rank {r} own stats")
            np.testing.assert_array_equal(got["own_ap"], own[r][0], err_msg=f"rank {r} own ap")


@pytest.mark.parametrize("world,nscans,mode", ((2, 4, "ca"), (4, 4, "nc"), (4, 3, "ca")))
def test_evaluation_over_gloo_ranks(world, nscans, mode, tmp_path):
    from maskclustering_amd.sweep import scenes_of
    want = golden_ctx(mode, range(nscans)).ev_ap()
    own = [golden_ctx(mode, scenes_of(r, world, nscans)).ev_ap() for r in range(world)]
    if nscans < world:
        assert own[world - 1][1][:, :, 0].sum() == 0      # a rank without scans
    outs = U.run_workers(f"golden:{mode}:{nscans}", world, tmp_path)
    check_ranks(outs, want[0], want[1], own, golden()["overlaps"])


def test_sweep_evaluation_over_two_ranks(tmp_path):
    from maskclustering_amd.synthetic_frames import make_frames_shape, slab_ground_truth
    from test_gpu_ap import SCENES, _run, _sweep
    sw = _sweep()
    sw.begin_evaluation(CLS, no_class=True)
    for shape, seed in SCENES:
        fr = make_frames_shape(shape, seed=seed)
        _run(sw, fr, slab_ground_truth(fr.scene_points, CLS))
    want = sw.evaluation()
    assert want["stats"][:, :, 0].sum() > 0
    outs = U.run_workers("sweep", 2, tmp_path)
    check_ranks(outs, want["ap"], want["stats"], None, R.default_overlaps())


def test_device_tensor_transport_in_a_one_rank_rccl_group(tmp_path):
    """torch.distributed's "nccl" backend (RCCL) with one rank: the states travel as device tensors
    and are merged from device memory.  More than one GPU is not covered here."""
    want = golden_ctx("ca", range(4)).ev_ap()
    outs = U.run_workers("golden:ca:4", 1, tmp_path, backend="nccl")
    check_ranks(outs, want[0], want[1], [want], golden()["overlaps"])


# ---- 7. save and load --------------------------------------------------------------------------------
def test_save_and_load_evaluation(tmp_path):
    from test_gpu_ap import _sweep
    z = golden()
    cfg = dict(no_class=False, overlaps=z["overlaps"], min_region_size=int(z["min_region_size"]))
    a = _sweep()
    a.begin_evaluation(z["class_ids"], **cfg)
    for s in (0, 1):
        a.ctx.ev_add_scan(*scan_args(s))
    path = str(tmp_path / "sweep.evstate")
    a.save_evaluation(path)
    np.testing.assert_array_equal(np.fromfile(path, np.uint8), a.ctx.ev_state())
    b = _sweep()
    b.begin_evaluation(z["class_ids"], **cfg)
    b.load_evaluation(path)
    for s in (2, 3):
        b.ctx.ev_add_scan(*scan_args(s))
    want = single("ca")[0]
    assert_same(snapshot(b.ctx), want, "resumed sweep")
    ev = b.evaluation()
    np.testing.assert_array_equal(ev["ap"], want[0])
