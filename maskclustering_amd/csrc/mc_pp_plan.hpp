// mc_pp_plan.hpp — post-processing: the decisions the host takes between the kernels.
// Pure host arithmetic (no HIP include, plain C++17), used by the steps of mc_pp_host.inl and checked
// on the CPU by tests/test_pp_plan_cpu.py (scripts/pp_plan_check.cpp).  The rules:
//  * Big nodes: the size order lists the nodes by descending point count; its leading nodes with
//    strictly more than big_min points take the split DBSCAN (k_pp_big_*), which walks each of them in
//    items of kPPItemPoints points, (node, first point of the item).
//  * Kept objects (filter_point, post_process.py:96): a DBSCAN object stays when it kept a point and
//    at least 2 masks.  At most kPPMaxKept of them: the merge indexes a Kk x Kk matrix with an int.
//  * Greedy merge (merge_overlapping_objects, post_process.py:14-29): the reference visits every pair
//    (i, j) ascending; "if invalid_object[i]: continue" is read once when row i starts (:15), so a row
//    whose own decision invalidated i still applies its later decisions; a pair whose j is already
//    invalid is skipped (:18); a decision invalidates i (coded -1 - j) or j (coded j).  Pairs without a
//    decision change nothing, so the list of the others, sorted by (i, j), gives the same flags.
//  * Final objects: the kept objects that stayed valid (state 2), in DBSCAN-object order (the
//    reference's total_*_list order after the merge), with the offsets of their point and mask lists.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mc {

// two ints laid out as the kernels' int2: (node, first point) of an item, (i, coded j) of a decision
struct PPInt2 {
    int32_t x, y;
};

constexpr int kPPItemPoints = 512;  // points per item of a big node (the workgroup size of k_pp_big_walk)
constexpr int kPPMaxKept = 46340;   // floor(sqrt(2^31 - 1)): Kk * Kk stays a 32-bit int

// Nodes of the split DBSCAN: returns nbig, the leading nodes of `order` above big_min points, and
// fills `items` with their (node, first point) items
inline int pp_big_items(const int64_t *node_pt_off, const int32_t *order, int N, int big_min, std::vector<PPInt2> &items)
{
    items.clear();
    int nbig = 0;
    while (nbig < N && node_pt_off[order[nbig] + 1] - node_pt_off[order[nbig]] > big_min) {
        const int k = order[nbig++];
        const int n = static_cast<int>(node_pt_off[k + 1] - node_pt_off[k]);
        for (int c = 0; c < n; c += kPPItemPoints) items.push_back({k, c});
    }
    return nbig;
}

// the objects filter_point keeps, with their boxes and point counts gathered for the merge
struct PPKept {
    std::vector<int32_t> kidx;  // object -> kept index, -1: dropped
    std::vector<int32_t> kept;  // kept index -> object
    std::vector<int32_t> klen;  // kept points per kept object
    std::vector<double> kbox;   // 6 doubles per kept object
};

inline PPKept pp_kept_objects(int K, const int32_t *nv, const int32_t *nm, const double *box)
{
    PPKept r;
    r.kidx.assign(K, -1);
    for (int o = 0; o < K; o++)
        if (nv[o] > 0 && nm[o] >= 2) {
            r.kidx[o] = static_cast<int32_t>(r.kept.size());
            r.kept.push_back(o);
            r.kbox.insert(r.kbox.end(), box + 6 * static_cast<size_t>(o), box + 6 * static_cast<size_t>(o) + 6);
            r.klen.push_back(nv[o]);
        }
    return r;
}

// the greedy pass over the non-zero decisions `d` (any order; sorted in place); inv: one flag per kept
// object, 0 on entry
inline void pp_greedy_merge(std::vector<PPInt2> &d, std::vector<uint8_t> &inv)
{
    auto jj = [](const PPInt2 &v) { return v.y < 0 ? -1 - v.y : v.y; };
    std::sort(d.begin(), d.end(), [&](const PPInt2 &a, const PPInt2 &b) { return a.x != b.x ? a.x < b.x : jj(a) < jj(b); });
    int row = -1;
    bool skip = false;
    for (const PPInt2 &v : d) {
        if (v.x != row) {
            row = v.x;
            skip = inv[row] != 0;
        }
        if (skip || inv[jj(v)]) continue;
        if (v.y < 0) inv[v.x] = 1;
        else inv[v.y] = 1;
    }
}

// the final-object tables: fslot (object -> final slot, -1), fin (final objects), fin_node (their
// nodes), opoff / omoff (offsets of their point and mask lists, nv / nm entries each)
inline void pp_final_tables(const std::vector<uint8_t> &state, const std::vector<int32_t> &obj_node, const int32_t *nv,
                            const int32_t *nm, std::vector<int32_t> &fslot, std::vector<int32_t> &fin,
                            std::vector<int32_t> &fin_node, std::vector<int64_t> &opoff, std::vector<int64_t> &omoff)
{
    fslot.assign(state.size(), -1);
    fin.clear();
    fin_node.clear();
    opoff.assign(1, 0);
    omoff.assign(1, 0);
    for (size_t o = 0; o < state.size(); o++)
        if (state[o] == 2) {
            fslot[o] = static_cast<int32_t>(fin.size());
            fin.push_back(static_cast<int32_t>(o));
            fin_node.push_back(obj_node[o]);
            opoff.push_back(opoff.back() + nv[o]);
            omoff.push_back(omoff.back() + nm[o]);
        }
}

}  // namespace mc
