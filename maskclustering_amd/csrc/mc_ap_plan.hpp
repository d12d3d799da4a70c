// mc_ap_plan.hpp — AP evaluation: what the host decides without the GPU.
// Pure host arithmetic (no HIP include, plain C++17), used by the steps of mc_ap_host.inl and checked
// on the CPU by tests/test_ap_plan_cpu.py (scripts/ap_plan_check.cpp).  Nothing here throws: a check
// returns nullptr, or the message the host reports with its status code.  The rules:
//  * Tables (mc_ev_add_matches, and what k_ev_compact wrote): ground-truth classes are ascending class
//    indices with positive vert counts; a prediction has a class index, 0 <= void <= vert, vert > 0
//    and a score that is no NaN; a pair joins a prediction and an instance of one class with
//    0 < intersection <= either vert count.  The first broken rule in this order gives the message.
//  * Class slots: the classes with an instance or a prediction in the scan, ascending.  A slot's pairs
//    are those of its instances (p0 = p1 = 0 without one), its region holds O times (pairs +
//    predictions) examples, and nfilt counts its instances with id >= 1000 and min_region vertices.
//  * Pair order: by ground truth, stable, so an instance keeps the order of the list.
//  * Word block: the one definition of its order is ev_words(); mc::EvScanDev points into the uploaded copy.
//  * Append limit: examples and units each stay below 2^31 (ev_check_append), for a scan and a merge.
//  * State buffer (include/mcgraph.h): ev_layout() gives the sections; the header and the per-cell
//    sections are checked here, the runs in k_ev_state_check.  Nothing is indexed before the size
//    the header claims has been compared with the byte count.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace mc {

struct EvTables {  // one scan's compact tables (include/mcgraph.h, mc_ev_get_scan)
    std::vector<int32_t> gcls, gid, pcls, ppred, pgt;
    std::vector<int64_t> gvert, pvert, pvoid, pint;
    std::vector<double> pscore;
};

// the table rules; gt_poff [G + 1]: offset of every instance's pairs in ground-truth order
inline const char *ev_check_tables(const EvTables &t, int C, std::vector<int64_t> &gt_poff)
{
    const int G = static_cast<int>(t.gcls.size()), K = static_cast<int>(t.pcls.size());
    const int64_t NP = static_cast<int64_t>(t.ppred.size());
    for (int g = 0; g < G; g++) {
        if (!(t.gcls[g] >= 0 && t.gcls[g] < C && (g == 0 || t.gcls[g] >= t.gcls[g - 1])))
            return "ground-truth classes must be ascending class indices";
        if (!(t.gvert[g] > 0)) return "ground-truth vert_count must be positive";
    }
    for (int k = 0; k < K; k++) {
        if (!(t.pcls[k] >= 0 && t.pcls[k] < C)) return "prediction class index out of range";
        if (!(t.pvert[k] > 0 && t.pvoid[k] >= 0 && t.pvoid[k] <= t.pvert[k])) return "bad prediction counts";
        if (std::isnan(t.pscore[k])) return "prediction score is NaN";
    }
    gt_poff.assign(static_cast<size_t>(G) + 1, 0);
    for (int64_t i = 0; i < NP; i++) {
        const int p = t.ppred[i], g = t.pgt[i];
        if (!(p >= 0 && p < K && g >= 0 && g < G)) return "pair index out of range";
        if (t.gcls[g] != t.pcls[p]) return "pair across classes";
        if (!(t.pint[i] > 0 && t.pint[i] <= t.gvert[g] && t.pint[i] <= t.pvert[p])) return "bad intersection";
        gt_poff[g + 1]++;
    }
    for (int g = 0; g < G; g++) gt_poff[g + 1] += gt_poff[g];
    return nullptr;
}

// The sections of a scan's word block, 2G + 4K + 3NP + 7A words from `gvert` to `end`; pscore holds
// doubles.  W is int64_t for the host block that is filled, const int64_t for its device copy.
template <typename W>
struct EvWords {
    W *gvert, *gid, *pvert, *pvoid, *pslot, *pscore, *q_gt, *q_pred, *q_int;
    W *s_p0, *s_p1, *s_nfilt, *s_npred, *s_cls, *s_exoff, *s_cap, *end;
};

template <typename W>
inline EvWords<W> ev_words(W *base, int64_t G, int64_t K, int64_t NP, int64_t A)
{
    EvWords<W> w;
    w.gvert = base, w.gid = w.gvert + G;
    w.pvert = w.gid + G, w.pvoid = w.pvert + K, w.pslot = w.pvoid + K, w.pscore = w.pslot + K;
    w.q_gt = w.pscore + K, w.q_pred = w.q_gt + NP, w.q_int = w.q_pred + NP;
    w.s_p0 = w.q_int + NP, w.s_p1 = w.s_p0 + A, w.s_nfilt = w.s_p1 + A, w.s_npred = w.s_nfilt + A, w.s_cls = w.s_npred + A;
    w.s_exoff = w.s_cls + A, w.s_cap = w.s_exoff + A, w.end = w.s_cap + A;
    return w;
}

struct EvScanPlan {
    int A = 0, U = 0;            // class slots, units (A * O)
    int64_t total = 0;           // examples the scan may append
    std::vector<int> cls_of;     // slot -> class
    std::vector<int64_t> words;  // the block of ev_words(), and one word more
};

// the plan of checked tables (t and gt_poff as ev_check_tables left them)
inline EvScanPlan ev_plan_scan(const EvTables &t, const std::vector<int64_t> &gt_poff, int C, int O, int64_t min_region)
{
    const int G = static_cast<int>(t.gcls.size()), K = static_cast<int>(t.pcls.size());
    const int64_t NP = static_cast<int64_t>(t.ppred.size());
    EvScanPlan p;
    // class slots: the classes with an instance or a prediction in this scan
    std::vector<int> slot(C, -1), g0(C, 0), g1(C, 0), npred(C, 0);
    std::vector<int64_t> nfilt(C, 0);
    for (int g = 0; g < G; g++) {
        const int c = t.gcls[g];
        if (g1[c] == 0 && (g == 0 || t.gcls[g - 1] != c)) g0[c] = g;
        g1[c] = g + 1;
        if (t.gid[g] >= 1000 && t.gvert[g] >= min_region) nfilt[c]++;
    }
    for (int k = 0; k < K; k++) npred[t.pcls[k]]++;
    for (int c = 0; c < C; c++)
        if (g1[c] > g0[c] || npred[c]) {
            slot[c] = p.A++;
            p.cls_of.push_back(c);
        }
    const int A = p.A;
    const size_t words = 2 * static_cast<size_t>(G) + 4 * static_cast<size_t>(K) + 3 * static_cast<size_t>(NP) + 7 * static_cast<size_t>(A);
    p.words.assign(words + 1, 0);
    const EvWords<int64_t> w = ev_words(p.words.data(), G, K, NP, A);
    for (int g = 0; g < G; g++) {
        w.gvert[g] = t.gvert[g];
        w.gid[g] = t.gid[g];
    }
    for (int k = 0; k < K; k++) {
        w.pvert[k] = t.pvert[k];
        w.pvoid[k] = t.pvoid[k];
        w.pslot[k] = slot[t.pcls[k]];
    }
    if (K) std::memcpy(w.pscore, t.pscore.data(), static_cast<size_t>(K) * 8);
    {
        std::vector<int64_t> at(gt_poff.begin(), gt_poff.end() - 1);  // stable: a ground truth keeps the list's order
        for (int64_t i = 0; i < NP; i++) {
            const int64_t j = at[t.pgt[i]]++;
            w.q_gt[j] = t.pgt[i];
            w.q_pred[j] = t.ppred[i];
            w.q_int[j] = t.pint[i];
        }
    }
    for (int a = 0; a < A; a++) {
        const int c = p.cls_of[a];
        const bool has = g1[c] > g0[c];
        w.s_p0[a] = has ? gt_poff[g0[c]] : 0;
        w.s_p1[a] = has ? gt_poff[g1[c]] : 0;
        w.s_nfilt[a] = nfilt[c];
        w.s_npred[a] = npred[c];
        w.s_cls[a] = c;
        w.s_cap[a] = (w.s_p1[a] - w.s_p0[a]) + npred[c];
        w.s_exoff[a] = p.total;
        p.total += w.s_cap[a] * O;
    }
    p.U = A * O;
    return p;
}

// may `add` examples in U units join an accumulation of ex_used examples in `units` units?
inline const char *ev_check_append(int64_t ex_used, int units, unsigned long long add, int U)
{
    constexpr int64_t lim = int64_t(1) << 31;
    if (!(add < (1ull << 31) && ex_used + static_cast<int64_t>(add) < lim && static_cast<int64_t>(units) + U < lim))
        return "more than 2^31 examples";
    return nullptr;
}

// the compact tables k_ev_compact wrote, 3G + 4K + 3NP words: per instance class, id, vert; per kept
// prediction class, vert, void, score (a double); per pair prediction, instance, intersection
inline size_t ev_compact_words(int G, int K, int NP)
{
    return 3 * static_cast<size_t>(G) + 4 * static_cast<size_t>(K) + 3 * static_cast<size_t>(NP);
}

inline EvTables ev_unpack_tables(const int64_t *w, int G, int K, int NP)
{
    EvTables t;
    t.gcls.assign(w, w + G), t.gid.assign(w + G, w + 2 * G), t.gvert.assign(w + 2 * G, w + 3 * G);
    w += 3 * static_cast<size_t>(G);
    t.pcls.assign(w, w + K), t.pvert.assign(w + K, w + 2 * K), t.pvoid.assign(w + 2 * K, w + 3 * K);
    t.pscore.resize(K);
    if (K) std::memcpy(t.pscore.data(), w + 3 * static_cast<size_t>(K), static_cast<size_t>(K) * 8);
    w += 4 * static_cast<size_t>(K);
    t.ppred.assign(w, w + NP), t.pgt.assign(w + NP, w + 2 * NP), t.pint.assign(w + 2 * NP, w + 3 * NP);
    return t;
}

// ---- the accumulation as a state buffer (include/mcgraph.h, mc_ev_state_*) -----------------------
constexpr int64_t kEvStateWord = (int64_t(1) << 32) | 0x5645434d;  // version 1, "MCEV"
constexpr size_t kEvStateHeader = 48;

struct EvLayout {  // byte offsets of the sections
    size_t ids, ov, roff, hf, fl, key, nt, nf, bytes;
};

inline EvLayout ev_layout(int C, int O, int64_t R)
{
    auto up = [](size_t b) { return (b + 7) & ~size_t(7); };
    const size_t NC = static_cast<size_t>(C) * O, r = static_cast<size_t>(R);
    EvLayout L;
    L.ids = kEvStateHeader;
    L.ov = L.ids + up(4 * static_cast<size_t>(C));
    L.roff = L.ov + 8 * static_cast<size_t>(O);
    L.hf = L.roff + 8 * (NC + 1);
    L.fl = L.hf + 8 * NC;
    L.key = L.fl + up(4 * NC);
    L.nt = L.key + 8 * r;
    L.nf = L.nt + up(4 * r);
    L.bytes = L.nf + up(4 * r);
    return L;
}

// The header of a buffer of `bytes` bytes against the context's configuration; hdr: its six words,
// nullptr when the buffer is too short to hold them.  R: the run count, with ev_layout(C, O, R).bytes <= bytes.
inline const char *ev_check_state_header(const int64_t *hdr, int64_t bytes, int C, int O, int64_t min_region, bool no_class,
                                         int64_t &R)
{
    if (!hdr || bytes < static_cast<int64_t>(kEvStateHeader)) return "state buffer is truncated";
    if (hdr[0] != kEvStateWord) return "not a state buffer of this version";
    if (!(hdr[1] == C && hdr[2] == O && hdr[3] == min_region && hdr[4] == (no_class ? 1 : 0)))
        return "state buffer of another configuration";
    R = hdr[5];
    if (!(R >= 0 && R < (int64_t(1) << 31))) return "bad run count";
    if (static_cast<int64_t>(ev_layout(C, O, R).bytes) > bytes) return "state buffer is truncated";
    return nullptr;
}

// The configuration and per-cell sections; mid: the buffer's bytes from L.ids to L.key.  cells: the
// cells with runs, ascending.
inline const char *ev_check_state_sections(const int64_t *mid, const EvLayout &L, const std::vector<int32_t> &class_ids,
                                           const std::vector<double> &overlaps, std::vector<int> &cells)
{
    const int NC = static_cast<int>(class_ids.size() * overlaps.size());
    const int64_t R = static_cast<int64_t>((L.nt - L.key) / 8);
    const char *mb = reinterpret_cast<const char *>(mid) - L.ids;
    if (!(std::memcmp(mb + L.ids, class_ids.data(), class_ids.size() * 4) == 0 &&
          std::memcmp(mb + L.ov, overlaps.data(), overlaps.size() * 8) == 0))
        return "state buffer of another configuration";
    const int64_t *roff = reinterpret_cast<const int64_t *>(mb + L.roff), *hf = reinterpret_cast<const int64_t *>(mb + L.hf);
    const uint32_t *fl = reinterpret_cast<const uint32_t *>(mb + L.fl);
    if (!(roff[0] == 0 && roff[NC] == R)) return "run offsets must ascend from 0 to the run count";
    cells.clear();
    for (int c = 0; c < NC; c++) {
        if (!(roff[c + 1] >= roff[c])) return "run offsets must ascend from 0 to the run count";
        if (!(hf[c] >= 0)) return "negative hard false negative count";
        if (!(fl[c] <= 3u)) return "unknown flag bits";
        if (roff[c + 1] > roff[c]) cells.push_back(c);
    }
    return nullptr;
}

}  // namespace mc
