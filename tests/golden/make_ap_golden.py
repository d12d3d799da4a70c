"""Golden fixture for the AP evaluation: the REFERENCE's own
``evaluation/evaluate.py`` (``assign_instances_for_scan`` :254-329, ``evaluate_matches`` :53-205,
``compute_averages`` :207-224) on four synthetic scans, class-aware and ``--no_class``.

Run ONLY where /root/reference exists:

    python tests/golden/make_ap_golden.py

The reference module is imported unmodified (its argument parsing reads the sys.argv set here;
torch's ``.cuda()`` is the identity on a CPU-only machine).  Predictions are derived from the
ground truth (noisy copies, duplicates, unions, void-heavy, too small, class 999) so that the AP
table is not trivial; the generator asserts that, and that tests/ap_restatement.py equals the
reference on the fixture.  Stored: the inputs (gt ids, predictions as point lists, scores,
classes, the scannet label table from evaluation/constants.py), each scan's two match dicts as
JSON, the ``ap`` array and the averages.  No source is copied.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import ap_restatement as R  # noqa: E402

P = 6000
NUM_SCANS = 4
USED = 8           # classes of the table the ground truth draws from


def to_json(x):
    def conv(o):
        if isinstance(o, np.integer):
            return int(o)
        if isinstance(o, np.floating):
            return float(o)
        raise TypeError(type(o))
    return json.dumps(x, default=conv)


def synthetic(seed, ids):
    """(gt ids [P], list of point-id arrays, scores, classes)."""
    rng = np.random.default_rng(100 + seed)
    gt = np.zeros(P, np.int64)
    used = [ids[i] for i in (0, 1, 2, 5, 9, 17, 40, 150)][:USED]
    runs = []                                   # (start, length, label)
    start, n = 0, 1
    fixed = [(200, used[0]), (400, used[0])] if seed == 3 else []   # overlaps of exactly 0.5 and 0.25
    while start < P - 450:
        if fixed:
            ln, lab = fixed.pop()
        else:
            ln = int(rng.integers(40, 420))
            r = rng.random()
            lab = int(rng.choice(used)) if r < 0.78 else (0 if r < 0.9 else 999)   # 999: not a class id (void)
        gt[start:start + ln] = lab * 1000 + n if lab else 0
        runs.append((start, ln, lab))
        n += 1
        start += ln + int(rng.integers(0, 25))
    inst = [r for r in runs if r[2] not in (0, 999)]
    preds, classes = [], []

    def noisy(a, ln, drop, spill):
        pts = np.arange(a, a + ln)
        pts = pts[rng.random(ln) >= drop]
        lo, hi = max(0, a - int(spill * ln)), min(P, a + ln + int(spill * ln))
        extra = np.r_[np.arange(lo, a), np.arange(a + ln, hi)]
        return np.unique(np.r_[pts, extra]).astype(np.int32)

    for a, ln, lab in inst:
        for _ in range(int(rng.choice([1, 1, 2, 3]))):                   # copies of the same instance
            preds.append(noisy(a, ln, rng.uniform(0.06, 0.6), rng.uniform(0.025, 0.3)))   # IoU < 0.9
            classes.append(lab if rng.random() < 0.9 else int(rng.choice(used)))
    for _ in range(4):                                                    # unions of two instances
        i, j = rng.choice(len(inst), 2, replace=False)
        preds.append(np.unique(np.r_[noisy(*inst[i][:2], 0.1, 0.0), noisy(*inst[j][:2], 0.1, 0.0)]).astype(np.int32))
        classes.append(inst[i][2])
    for a, ln, lab in [r for r in runs if r[2] in (0, 999)][:5]:          # mostly void / unlabelled
        preds.append(noisy(a, ln, 0.05, 0.1))
        classes.append(int(rng.choice(used)))
    for _ in range(3):                                                    # under 100 points
        a = int(rng.integers(0, P - 100))
        preds.append(np.arange(a, a + int(rng.integers(5, 100)), dtype=np.int32))
        classes.append(int(rng.choice(used)))
    for _ in range(3):                                                    # not a class
        a, ln, _ = inst[int(rng.integers(len(inst)))]
        preds.append(noisy(a, ln, 0.1, 0.1))
        classes.append(999)
    if seed == 3:
        (a4, _, _), (a2, _, _) = runs[0], runs[1]
        preds += [np.arange(a4, a4 + 100, dtype=np.int32), np.arange(a2, a2 + 100, dtype=np.int32)]
        classes += [used[0], used[0]]
    order = rng.permutation(len(preds))
    preds, classes = [preds[i] for i in order], np.array([classes[i] for i in order], np.int32)
    K = len(preds)
    scores = {0: rng.random(K), 1: np.round(rng.random(K) * 4) / 4, 2: np.ones(K), 3: rng.random(K)}[seed]
    return gt, preds, scores.astype(np.float64), classes


def load_reference(tmp, no_class):
    sys.dont_write_bytecode = True
    import torch
    torch.Tensor.cuda = lambda self, *a, **k: self
    if REF not in sys.path:
        sys.path.insert(0, REF)
    sys.argv = ["evaluate.py", "--pred_path", tmp, "--gt_path", tmp, "--dataset", "scannet"] + \
        (["--no_class"] if no_class else [])
    for m in [m for m in sys.modules if m == "evaluation.evaluate"]:
        del sys.modules[m]
    return importlib.import_module("evaluation.evaluate")


def main():
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from evaluation import constants
    ids, labels = list(constants.SCANNET_IDS), list(constants.SCANNET_LABELS)
    assert 999 not in ids
    out = {"class_ids": np.array(ids, np.int64), "class_labels": np.array(labels), "num_scans": np.array(NUM_SCANS)}
    scans = [synthetic(s, ids) for s in range(NUM_SCANS)]
    for s, (gt, preds, scores, classes) in enumerate(scans):
        off = np.concatenate([[0], np.cumsum([len(p) for p in preds])]).astype(np.int64)
        out.update({f"s{s}_gt": gt.astype(np.int32), f"s{s}_off": off, f"s{s}_pts": np.concatenate(preds).astype(np.int32),
                    f"s{s}_scores": scores, f"s{s}_classes": classes})
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for no_class in (False, True):
                mode = "nc" if no_class else "ca"
                ev = load_reference(tmp, no_class)
                rs = R.APRestatement(ids, ev.opt.overlaps, int(ev.opt.min_region_sizes[0]), no_class)
                matches = {}
                for s, (gt, preds, scores, classes) in enumerate(scans):
                    dense = np.zeros((P, len(preds)), bool)
                    for k, p in enumerate(preds):
                        dense[p, k] = True
                    np.savetxt(os.path.join(tmp, f"scene{s}.txt"), gt, fmt="%d")
                    np.savez(os.path.join(tmp, f"scene{s}.npz"), pred_masks=dense, pred_score=scores, pred_classes=classes)
                    g2p, p2g = ev.assign_instances_for_scan(os.path.join(tmp, f"scene{s}.npz"),
                                                            os.path.join(tmp, f"scene{s}.txt"))
                    matches[f"scene{s}"] = {"gt": g2p, "pred": p2g}
                    out[f"{mode}_s{s}_gt2pred"] = np.array(to_json(g2p))
                    out[f"{mode}_s{s}_pred2gt"] = np.array(to_json(p2g))
                    t = rs.add_scan(gt, out[f"s{s}_off"], out[f"s{s}_pts"], classes, scores)
                    R.assert_tables_equal(t, R.tables_from_dicts(g2p, p2g, labels), f"{mode} scan {s}")
                t0 = time.perf_counter()
                ap = ev.evaluate_matches(matches)
                dt = time.perf_counter() - t0
                avgs = ev.compute_averages(ap)
                out[f"{mode}_ap"] = ap
                out[f"{mode}_avgs"] = np.array(to_json(avgs))
                out["overlaps"] = np.asarray(ev.opt.overlaps, np.float64)
                out["min_region_size"] = np.array(int(ev.opt.min_region_sizes[0]))
                # the fixture is not vacuous, and the restatement equals the reference on it
                got, stats, curves = rs.result()
                npts = np.ones_like(got)
                for (c, o), cv in curves.items():
                    npts[c, o] = len(cv[0]) + 1
                assert R.ap_close(got, ap[0], npts), "restatement != reference"
                a = ap[0]
                inside = int(np.sum((a > 0) & (a < 1)))
                # --no_class folds every instance into the table's first class: its table has O entries that
                # are not nan, so "at least 20" can hold class-aware only; there, more than half must lie inside
                need = 20 if not no_class else len(ev.opt.overlaps) // 2 + 1
                assert inside >= need and np.any(a == 0) and np.any(np.isnan(a)), (inside,)
                assert all(v >= 1 for v in rs.counters.values()), rs.counters
                mine = R.compute_averages(got, ev.opt.overlaps, labels)
                for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
                    assert abs(mine[k] - avgs[k]) <= npts.max() * 2.0 ** -52, k
                print(f"{mode}: evaluate_matches {dt:.3f} s; entries in (0,1): {inside}, zeros {int(np.sum(a == 0))}, "
                      f"nan {int(np.isnan(a).sum())}; branches {rs.counters}; all_ap {avgs['all_ap']:.4f}")
        finally:
            os.chdir(cwd)
    path = os.path.join(HERE, "ap_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
