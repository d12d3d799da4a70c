"""S6 on explicit level-0 nodes, device against the dense CPU oracle: shared by test_gpu_parity.py and
test_gpu_graph_limits.py."""
import numpy as np


def set_nodes_dense(run, vf, cm, pts=None):
    from maskclustering_amd.pipeline import bool_to_bits
    N, F = vf.shape
    M = cm.shape[1]
    r, c = np.nonzero(cm)
    c_off = np.zeros(N + 1, np.int64)
    c_off[1:] = np.cumsum(np.bincount(r, minlength=N))
    if pts is None:
        pts = [np.array([i], np.int32) for i in range(N)]
    pt_off = np.zeros(N + 1, np.int64)
    pt_off[1:] = np.cumsum([len(p) for p in pts])
    P = int(max((p.max() + 1 for p in pts if len(p)), default=1))
    run.ctx.set_nodes(F, M, P, bool_to_bits(vf.astype(bool)), c_off, c.astype(np.int32), pt_off,
                      np.concatenate(pts).astype(np.int32))


def oracle_cluster_check(run, vf, cm, thr, ct):
    from oracle import oracle
    parts, sizes, final, fvf, fcm = oracle.cluster(vf.astype(np.uint8), cm.astype(np.uint8), np.asarray(thr, np.float32), ct)
    set_nodes_dense(run, vf, cm)
    run.cluster(ct, thresholds=np.asarray(thr, np.float32))
    got = run.canonical_cluster(vf.shape[1])
    assert int(got["num_iters"]) == len(parts)
    for t in range(len(parts)):
        np.testing.assert_array_equal(got[f"part_{t}"], parts[t], err_msg=f"partition {t}")
    np.testing.assert_array_equal(run.ctx.final_labels(len(vf)), final)
    from maskclustering_amd.pipeline import bits_to_bool
    K = len(fvf)
    obj = run.ctx.objects(run.ctx.cluster_info(), vf.shape[1])
    np.testing.assert_array_equal(bits_to_bool(obj["vf_bits"], vf.shape[1]), fvf.astype(bool))
    for k in range(K):
        np.testing.assert_array_equal(obj["c_idx"][obj["c_off"][k]:obj["c_off"][k + 1]], np.nonzero(fcm[k])[0])
