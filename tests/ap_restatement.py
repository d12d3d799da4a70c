"""Plain numpy/Python restatement of the reference's AP evaluation (evaluation/evaluate.py:53-205 and
:254-329, evaluation/utils_3d.py:54-65) on packed tables: test infrastructure, the yardstick of the
device route (``mc_ev_*``).  Not imported by the package.

A scan's tables (all numpy arrays):
  gt_cls / gt_id / gt_vert      ground-truth instances grouped by class index in class-table order,
                                ascending id within a class
  pr_cls / pr_vert / pr_void / pr_score
                                the kept predictions in input order
  pair_pred / pair_gt / pair_int
                                the non-zero same-class intersections, sorted by (prediction, instance)

``BRANCHES`` names the counters ``APRestatement.counters`` keeps, one per branch of the greedy pass.
"""
from __future__ import annotations

import numpy as np

BRANCHES = ("second_match", "ignored_pred", "unmatched_fp", "hard_fn", "dropped_pred")


def default_overlaps():
    return np.append(np.arange(0.5, 0.95, 0.05), 0.25)


def scan_tables(gt_ids, pred_off, pred_pts, pred_classes, pred_scores, class_ids, min_region_size=100,
                no_class=False, counters=None):
    """assign_instances_for_scan on point lists (ids within a list distinct)."""
    class_ids = [int(c) for c in class_ids]
    cidx = {c: i for i, c in enumerate(class_ids)}
    ids = np.asarray(gt_ids).astype(np.int64)
    if no_class:
        ids = ids % 1000 + class_ids[0] * 1000
    uniq, cnt = np.unique(ids, return_counts=True)
    inst = [(cidx[int(u) // 1000], int(u), int(n)) for u, n in zip(uniq, cnt) if u != 0 and int(u) // 1000 in cidx]
    inst.sort()                                  # class-table order, ascending id within the class
    index_of = {iid: g for g, (_, iid, _) in enumerate(inst)}
    void = ~np.isin(ids // 1000, class_ids)
    K = len(pred_off) - 1
    pr, pairs = [], []
    for k in range(K):
        label = class_ids[0] if no_class else (0 if pred_classes is None else int(pred_classes[k]))
        pts = np.asarray(pred_pts[int(pred_off[k]):int(pred_off[k + 1])], np.int64)
        if label not in cidx or len(pts) < min_region_size:
            if counters is not None:
                counters["dropped_pred"] += 1
            continue
        c = cidx[label]
        u, n = np.unique(ids[pts], return_counts=True)
        for iid, m in zip(u.tolist(), n.tolist()):
            g = index_of.get(iid)
            if g is not None and inst[g][0] == c:
                pairs.append((len(pr), g, m))
        pr.append((c, len(pts), int(void[pts].sum()), 1.0 if pred_scores is None else float(pred_scores[k])))
    pairs.sort()
    col = lambda rows, j, dt: np.array([r[j] for r in rows], dt)
    return dict(gt_cls=col(inst, 0, np.int32), gt_id=col(inst, 1, np.int32), gt_vert=col(inst, 2, np.int64),
                pr_cls=col(pr, 0, np.int32), pr_vert=col(pr, 1, np.int64), pr_void=col(pr, 2, np.int64),
                pr_score=col(pr, 3, np.float64), pair_pred=col(pairs, 0, np.int32), pair_gt=col(pairs, 1, np.int32),
                pair_int=col(pairs, 2, np.int64))


def tables_from_dicts(gt2pred, pred2gt, class_labels):
    """The reference's two match dicts of one scan as tables.  Asserts what the tables take for granted:
    matched_pred lists in ascending prediction order, matched_gt lists in ascending instance order."""
    gt, first = [], {}
    for c, label in enumerate(class_labels):
        first[label] = len(gt)
        for g in gt2pred[label]:
            gt.append((c, int(g["instance_id"]), int(g["vert_count"])))
    preds = sorted(((int(p["pred_id"]), c, p) for c, label in enumerate(class_labels) for p in pred2gt[label]),
                   key=lambda t: t[0])
    assert [t[0] for t in preds] == list(range(len(preds)))
    pr, pairs = [], []
    for pid, c, p in preds:
        pr.append((c, int(p["vert_count"]), int(p["void_intersection"]), float(p["confidence"])))
        ids = [g[1] for g in gt]
        last = -1
        for m in p["matched_gt"]:
            g = first[class_labels[c]] + [x["instance_id"] for x in gt2pred[class_labels[c]]].index(m["instance_id"])
            assert ids[g] == m["instance_id"] and g > last
            last = g
            pairs.append((pid, g, int(m["intersection"])))
    by_gt = {}
    for pid, g, m in pairs:
        by_gt.setdefault(g, []).append((pid, m))
    for c, label in enumerate(class_labels):
        for j, g in enumerate(gt2pred[label]):
            want = by_gt.get(first[label] + j, [])
            assert [(int(p["pred_id"]), int(p["intersection"])) for p in g["matched_pred"]] == want
    col = lambda rows, j, dt: np.array([r[j] for r in rows], dt)
    return dict(gt_cls=col(gt, 0, np.int32), gt_id=col(gt, 1, np.int32), gt_vert=col(gt, 2, np.int64),
                pr_cls=col(pr, 0, np.int32), pr_vert=col(pr, 1, np.int64), pr_void=col(pr, 2, np.int64),
                pr_score=col(pr, 3, np.float64), pair_pred=col(pairs, 0, np.int32), pair_gt=col(pairs, 1, np.int32),
                pair_int=col(pairs, 2, np.int64))


def assert_tables_equal(got, want, msg=""):
    for k in want:
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg=f"{msg} {k}")


class APRestatement:
    def __init__(self, class_ids, overlaps=None, min_region_size=100, no_class=False):
        self.class_ids = [int(c) for c in class_ids]
        self.overlaps = default_overlaps() if overlaps is None else np.asarray(overlaps, np.float64)
        self.min_region_size = int(min_region_size)
        self.no_class = bool(no_class)
        self.C, self.O = len(self.class_ids), len(self.overlaps)
        self.counters = {b: 0 for b in BRANCHES}
        self.scans = []           # per scan: {(c, o): [(score, true), ...]}
        self.hard_fn = np.zeros((self.C, self.O), np.int64)
        self.flags = np.zeros((self.C, self.O), np.int64)

    def add_scan(self, gt_ids, pred_off, pred_pts, pred_classes=None, pred_scores=None):
        t = scan_tables(gt_ids, pred_off, pred_pts, pred_classes, pred_scores, self.class_ids,
                        self.min_region_size, self.no_class, self.counters)
        self.add_tables(t)
        return t

    def add_tables(self, t):
        """The greedy pass (evaluate_matches :62-149) of one scan, per class and overlap."""
        mrs = self.min_region_size
        G, K = len(t["gt_cls"]), len(t["pr_cls"])
        by_gt = [[] for _ in range(G)]        # in the pair list's order: ascending prediction
        by_pr = [[] for _ in range(K)]
        for p, g, m in zip(t["pair_pred"].tolist(), t["pair_gt"].tolist(), t["pair_int"].tolist()):
            by_gt[g].append((p, m))
            by_pr[p].append((g, m))
        examples = {}
        for oi, th in enumerate(self.overlaps):
            visited = [False] * K
            for c in sorted(set(t["gt_cls"].tolist()) | set(t["pr_cls"].tolist())):
                ex = examples.setdefault((c, oi), [])
                gts = [g for g in range(G) if t["gt_cls"][g] == c]
                prs = [p for p in range(K) if t["pr_cls"][p] == c]
                kept = [g for g in gts if t["gt_id"][g] >= 1000 and t["gt_vert"][g] >= mrs]
                if kept:
                    self.flags[c, oi] |= 1
                if prs:
                    self.flags[c, oi] |= 2
                for g in kept:
                    matched, score = False, -np.inf
                    for p, m in by_gt[g]:
                        if visited[p]:
                            continue
                        overlap = float(m) / (int(t["gt_vert"][g]) + int(t["pr_vert"][p]) - m)
                        if overlap > th:
                            conf = float(t["pr_score"][p])
                            if matched:                  # the lower score is a false positive; p stays unvisited
                                ex.append((min(score, conf), 0))
                                score = max(score, conf)
                                self.counters["second_match"] += 1
                            else:
                                matched, score = True, conf
                                visited[p] = True
                    if matched:
                        ex.append((score, 1))
                    else:
                        self.hard_fn[c, oi] += 1
                        self.counters["hard_fn"] += 1
                for p in prs:
                    found = False
                    for g, m in by_pr[p]:
                        if float(m) / (int(t["gt_vert"][g]) + int(t["pr_vert"][p]) - m) > th:
                            found = True
                            break
                    if found:
                        continue
                    ign = int(t["pr_void"][p])
                    for g, m in by_pr[p]:
                        if t["gt_id"][g] < 1000:
                            ign += m
                        if t["gt_vert"][g] < mrs:
                            ign += m
                    if float(ign) / int(t["pr_vert"][p]) <= th:
                        ex.append((float(t["pr_score"][p]), 0))
                        self.counters["unmatched_fp"] += 1
                    else:
                        self.counters["ignored_pred"] += 1
        self.scans.append(examples)

    def result(self, rng=None):
        """(ap [C, O], stats [C, O, 4], curves {(c, o): (scores, tp, fp, fn)}).  rng: every scan's examples
        are shuffled first (the result does not depend on their order)."""
        ap = np.zeros((self.C, self.O))
        stats = np.zeros((self.C, self.O, 4), np.int64)
        curves = {}
        for c in range(self.C):
            for oi in range(self.O):
                ex = []
                for s in self.scans:
                    e = list(s.get((c, oi), []))
                    if rng is not None:
                        e = [e[i] for i in rng.permutation(len(e))]
                    ex += e
                if rng is not None:
                    ex = [ex[i] for i in rng.permutation(len(ex))]
                f, hf = int(self.flags[c, oi]), int(self.hard_fn[c, oi])
                stats[c, oi] = (len(ex), sum(t for _, t in ex), hf, f)
                if f == 3 and ex:
                    ap[c, oi], curves[(c, oi)] = ap_of(ex, hf)
                elif f & 1:
                    ap[c, oi] = 0.0
                else:
                    ap[c, oi] = np.nan
        return ap, stats, curves


def ap_of(examples, hard_fn):
    """evaluate_matches :156-198 on (score, true) pairs: one precision/recall point per distinct score."""
    score = np.array([s for s, _ in examples], np.float64)
    true = np.array([t for _, t in examples], np.int64)
    order = np.argsort(score, kind="stable")
    score, true = score[order], true[order]
    n, n_true = len(score), int(true.sum())
    first = np.flatnonzero(np.r_[True, score[1:] != score[:-1]])
    below = np.concatenate([[0], np.cumsum(true)])[first]        # true examples with a lower score
    tp = n_true - below
    fp = (n - first) - tp
    fn = below + hard_fn
    precision = np.append(tp.astype(np.float64) / (tp + fp).astype(np.float64), 1.0)
    recall = np.append(tp.astype(np.float64) / (tp + fn).astype(np.float64), 0.0)
    a = np.concatenate([[recall[0]], recall, [0.0]])
    width = 0.5 * a[:-2] - 0.5 * a[2:]
    total = 0.0
    for p, w in zip(precision.tolist(), width.tolist()):
        total += p * w
    return total, (score[first], tp, fp, fn)


def compute_averages(ap, overlaps, class_labels):
    """evaluate.py:207-224 on a [C, O] table."""
    overlaps = np.asarray(overlaps)
    o50, o25 = np.isclose(overlaps, 0.5), np.isclose(overlaps, 0.25)
    rest = ~o25
    out = {"all_ap": np.nanmean(ap[:, rest]), "all_ap_50%": np.nanmean(ap[:, o50]), "all_ap_25%": np.nanmean(ap[:, o25]),
           "classes": {}}
    for li, name in enumerate(class_labels):
        out["classes"][name] = {"ap": np.average(ap[li, rest]), "ap50%": np.average(ap[li, o50]),
                                "ap25%": np.average(ap[li, o25])}
    return out


def ap_close(got, want, npoints):
    """nan where want is nan, exactly 0 where want is 0, else within npoints * 2^-52."""
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    if not np.array_equal(got == 0, want == 0):
        return False
    ok = ~np.isnan(want)
    return bool(np.all(np.abs(got[ok] - want[ok]) <= np.asarray(npoints)[ok] * 2.0 ** -52))
