// AP evaluation host decisions (maskclustering_amd/csrc/mc_ap_plan.hpp) on the CPU: a worked scan with
// its word block written out, every table rejection and the precedence among them, random tables
// against a restatement (stable sort by ground truth, classes grouped by a map), the word order, the
// 2^31 limit, the compact-tables unpack, and the state buffer's layout and checks on a buffer built here.
// Built and run by tests/test_ap_plan_cpu.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -I maskclustering_amd/csrc scripts/ap_plan_check.cpp -o ap_plan_check && ./ap_plan_check
#include <algorithm>
#include <cstdio>
#include <functional>
#include <limits>
#include <map>
#include <random>
#include <string>

#include "mc_ap_plan.hpp"

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("line %d: %s\n", __LINE__, #cond);                \
            bad++;                                                   \
        }                                                            \
    } while (0)

using namespace mc;
using vec64 = std::vector<int64_t>;

static bool is(const char *got, const char *want) { return got && want ? std::string(got) == want : got == want; }

static int64_t bits(double x)
{
    int64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}

// The worked scan (tests/test_gpu_ap.py::test_rejected_tables_leave_the_accumulation adds the same one):
// class 0 has instances 0 (id 3001) and 1 (id 500 < 1000: a group) and predictions 0 and 1; class 1 has
// prediction 2 and no instance; class 2 has instances 2 and 3 (60 vertices < min_region) and no prediction.
// The pairs (prediction, instance, intersection) are listed shuffled.
static EvTables worked()
{
    EvTables t;
    t.gcls = {0, 0, 2, 2}, t.gid = {3001, 500, 8002, 8003}, t.gvert = {300, 200, 150, 60};
    t.pcls = {0, 0, 1}, t.pvert = {280, 120, 90}, t.pvoid = {10, 0, 5}, t.pscore = {0.9, 0.4, 0.7};
    t.ppred = {1, 1, 0, 0}, t.pgt = {1, 0, 1, 0}, t.pint = {20, 90, 15, 250};
    return t;
}

static void worked_scan()
{
    const EvTables t = worked();
    vec64 poff{7};
    CHECK(is(ev_check_tables(t, 3, poff), nullptr));
    CHECK((poff == vec64{0, 2, 4, 4, 4}));
    const EvScanPlan p = ev_plan_scan(t, poff, 3, 2, 100);
    CHECK(p.A == 3 && p.U == 6 && p.total == 14);
    CHECK((p.cls_of == std::vector<int>{0, 1, 2}));
    const vec64 want{300, 200, 150, 60,  3001, 500, 8002, 8003,                       // gvert, gid
                     280, 120, 90,  10, 0, 5,  0, 0, 1,  bits(0.9), bits(0.4), bits(0.7),  // pvert, pvoid, pslot, pscore
                     0, 0, 1, 1,  1, 0, 1, 0,  90, 250, 20, 15,                        // q_gt, q_pred, q_int: list order within an instance
                     0, 0, 4,  4, 0, 4,                                                // s_p0, s_p1: the class without instance has 0, 0
                     1, 0, 1,  2, 1, 0,  0, 1, 2,                                      // s_nfilt (not the group, not the small one), s_npred, s_cls
                     0, 12, 14,  6, 1, 0,                                              // s_exoff, s_cap
                     0};                                                               // the word behind the block
    CHECK(want.size() == 2 * 4 + 4 * 3 + 3 * 4 + 7 * 3 + 1);
    CHECK(p.words == want);
    // a slot is not its class: without class 0, class 1 is slot 0 and class 2 slot 1
    EvTables u;
    u.gcls = {2}, u.gid = {8001}, u.gvert = {100};
    u.pcls = {1, 2}, u.pvert = {50, 100}, u.pvoid = {0, 0}, u.pscore = {0.5, 0.25};
    u.ppred = {1}, u.pgt = {0}, u.pint = {100};
    CHECK(is(ev_check_tables(u, 3, poff), nullptr));
    const EvScanPlan q = ev_plan_scan(u, poff, 3, 5, 100);
    CHECK(q.A == 2 && q.U == 10 && q.total == 5 * 1 + 5 * 2 && (q.cls_of == std::vector<int>{1, 2}));
    const EvWords<const int64_t> w = ev_words<const int64_t>(q.words.data(), 1, 2, 1, 2);
    CHECK(w.pslot[0] == 0 && w.pslot[1] == 1 && w.s_cls[0] == 1 && w.s_cls[1] == 2);
    CHECK(w.s_p0[0] == 0 && w.s_p1[0] == 0 && w.s_p0[1] == 0 && w.s_p1[1] == 1 && w.s_exoff[1] == 5 && w.s_nfilt[1] == 1);
    // the empty scan
    const EvTables e;
    CHECK(is(ev_check_tables(e, 3, poff), nullptr) && (poff == vec64{0}));
    const EvScanPlan z = ev_plan_scan(e, poff, 3, 2, 100);
    CHECK(z.A == 0 && z.U == 0 && z.total == 0 && z.cls_of.empty() && z.words.size() == 1);
}

static void rejections()
{
    const char *m_cls = "ground-truth classes must be ascending class indices", *m_vert = "ground-truth vert_count must be positive",
               *m_pcls = "prediction class index out of range", *m_cnt = "bad prediction counts", *m_nan = "prediction score is NaN",
               *m_idx = "pair index out of range", *m_across = "pair across classes", *m_int = "bad intersection";
    auto broken = [](const std::function<void(EvTables &)> &f) {
        EvTables t = worked();
        f(t);
        vec64 poff;
        return ev_check_tables(t, 3, poff);
    };
    // the eleven rules, one field broken each
    CHECK(is(broken([](EvTables &t) { t.gcls[3] = 3; }), m_cls));     // no class index
    CHECK(is(broken([](EvTables &t) { t.gcls[0] = -1; }), m_cls));
    CHECK(is(broken([](EvTables &t) { t.gcls[0] = 2; }), m_cls));     // descending
    CHECK(is(broken([](EvTables &t) { t.gvert[2] = 0; }), m_vert));
    CHECK(is(broken([](EvTables &t) { t.pcls[1] = -1; }), m_pcls));
    CHECK(is(broken([](EvTables &t) { t.pcls[2] = 3; }), m_pcls));
    CHECK(is(broken([](EvTables &t) { t.pvert[0] = 0; }), m_cnt));
    CHECK(is(broken([](EvTables &t) { t.pvoid[2] = -1; }), m_cnt));
    CHECK(is(broken([](EvTables &t) { t.pvoid[2] = 91; }), m_cnt));   // more void than vertices
    CHECK(is(broken([](EvTables &t) { t.pscore[1] = std::numeric_limits<double>::quiet_NaN(); }), m_nan));
    CHECK(is(broken([](EvTables &t) { t.ppred[0] = 3; }), m_idx));
    CHECK(is(broken([](EvTables &t) { t.ppred[3] = -1; }), m_idx));
    CHECK(is(broken([](EvTables &t) { t.pgt[2] = 4; }), m_idx));
    CHECK(is(broken([](EvTables &t) { t.pgt[1] = -1; }), m_idx));
    CHECK(is(broken([](EvTables &t) { t.pgt[0] = 2; }), m_across));   // prediction 1 of class 0, instance 2 of class 2
    CHECK(is(broken([](EvTables &t) { t.ppred[0] = 2; }), m_across));
    CHECK(is(broken([](EvTables &t) { t.pint[3] = 0; }), m_int));
    CHECK(is(broken([](EvTables &t) { t.pint[3] = 281; }), m_int));   // above the prediction's 280, below the instance's 300
    CHECK(is(broken([](EvTables &t) { t.pint[1] = 121; }), m_int));   // above the prediction's 120
    CHECK(is(broken([](EvTables &t) { t.pint[2] = 201; }), m_int));   // above the instance's 200, below the prediction's 280
    // an infinite score is a score
    CHECK(is(broken([](EvTables &t) { t.pscore[0] = std::numeric_limits<double>::infinity(); }), nullptr));
    // precedence: ground truth before predictions before pairs; within an entry the rules' order; entries in order
    CHECK(is(broken([](EvTables &t) { t.gvert[0] = 0, t.pint[0] = 0; }), m_vert));
    CHECK(is(broken([](EvTables &t) { t.gcls[3] = 3, t.pcls[0] = -1; }), m_cls));
    CHECK(is(broken([](EvTables &t) { t.pvert[2] = 0, t.ppred[0] = 7; }), m_cnt));
    CHECK(is(broken([](EvTables &t) { t.gvert[0] = 0, t.gcls[1] = 5; }), m_vert));   // instance 0's vert before instance 1's class
    CHECK(is(broken([](EvTables &t) { t.gvert[1] = 0, t.gcls[1] = 5; }), m_cls));    // one instance: class before vert
    CHECK(is(broken([](EvTables &t) { t.pscore[0] = std::nan(""), t.pcls[1] = 9; }), m_nan));
    CHECK(is(broken([](EvTables &t) { t.pscore[1] = std::nan(""), t.pvoid[1] = -1; }), m_cnt));
    CHECK(is(broken([](EvTables &t) { t.pint[0] = 0, t.pgt[1] = 9; }), m_int));      // pair 0 before pair 1
    CHECK(is(broken([](EvTables &t) { t.pgt[0] = 2, t.pint[0] = 0; }), m_across));   // one pair: classes before intersection
    CHECK(is(broken([](EvTables &t) { t.pcls[1] = 1; }), m_across));                 // a valid class that no longer is its pairs'
}

// the plan, restated: pairs stable-sorted by ground truth, classes grouped by a map
static void restated(const EvTables &t, int O, int64_t min_region, vec64 &words, int &A, int64_t &total)
{
    struct Cls {
        std::vector<int> inst, pred;
    };
    std::map<int, Cls> by;
    for (size_t g = 0; g < t.gcls.size(); g++) by[t.gcls[g]].inst.push_back(static_cast<int>(g));
    for (size_t k = 0; k < t.pcls.size(); k++) by[t.pcls[k]].pred.push_back(static_cast<int>(k));
    std::vector<size_t> order(t.ppred.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return t.pgt[a] < t.pgt[b]; });
    std::map<int, int> slot;
    for (const auto &kv : by) slot.emplace(kv.first, static_cast<int>(slot.size()));
    A = static_cast<int>(by.size());
    words.clear();
    for (int64_t v : t.gvert) words.push_back(v);
    for (int32_t v : t.gid) words.push_back(v);
    for (int64_t v : t.pvert) words.push_back(v);
    for (int64_t v : t.pvoid) words.push_back(v);
    for (int32_t c : t.pcls) words.push_back(slot[c]);
    for (double v : t.pscore) words.push_back(bits(v));
    for (size_t i : order) words.push_back(t.pgt[i]);
    for (size_t i : order) words.push_back(t.ppred[i]);
    for (size_t i : order) words.push_back(t.pint[i]);
    vec64 p0, p1, nfilt, npred, cls, exoff, cap;
    total = 0;
    for (const auto &kv : by) {
        const Cls &c = kv.second;
        int64_t first = 0, last = 0, nf = 0;
        if (!c.inst.empty()) {
            first = std::count_if(t.pgt.begin(), t.pgt.end(), [&](int g) { return g < c.inst.front(); });
            last = std::count_if(t.pgt.begin(), t.pgt.end(), [&](int g) { return g <= c.inst.back(); });
        }
        for (int g : c.inst) nf += t.gid[g] >= 1000 && t.gvert[g] >= min_region;
        p0.push_back(first), p1.push_back(last), nfilt.push_back(nf), npred.push_back(static_cast<int64_t>(c.pred.size()));
        cls.push_back(kv.first), exoff.push_back(total), cap.push_back(last - first + static_cast<int64_t>(c.pred.size()));
        total += cap.back() * O;
    }
    for (const vec64 *v : {&p0, &p1, &nfilt, &npred, &cls, &exoff, &cap}) words.insert(words.end(), v->begin(), v->end());
    words.push_back(0);
}

static void random_tables()
{
    std::mt19937 rng(20240911);
    auto upto = [&](int n) { return static_cast<int>(rng() % static_cast<unsigned>(n + 1)); };
    int differ = 0, rejected = 0, fewer_slots = 0, pred_only = 0;
    int64_t pairs = 0;
    for (int it = 0; it < 2000; it++) {
        const int C = 1 + upto(4), G = upto(12), K = upto(10), O = 1 + upto(3);
        const int64_t min_region = 50 + upto(100);
        EvTables t;
        for (int g = 0; g < G; g++) {
            t.gcls.push_back(upto(C - 1));
            t.gid.push_back(upto(3) ? 1000 * (t.gcls[g] + 1) + g : upto(999));
            t.gvert.push_back(1 + upto(200));
        }
        std::sort(t.gcls.begin(), t.gcls.end());
        for (int k = 0; k < K; k++) {
            t.pcls.push_back(upto(C - 1));
            t.pvert.push_back(1 + upto(200));
            t.pvoid.push_back(upto(static_cast<int>(t.pvert[k])));
            t.pscore.push_back(upto(8) / 8.0);
        }
        std::vector<std::pair<int, int>> pg;  // a random subset of the same-class pairs, in random order
        for (int k = 0; k < K; k++)
            for (int g = 0; g < G; g++)
                if (t.pcls[k] == t.gcls[g] && upto(2)) pg.push_back({k, g});
        std::shuffle(pg.begin(), pg.end(), rng);
        for (const auto &e : pg) {
            t.ppred.push_back(e.first), t.pgt.push_back(e.second);
            t.pint.push_back(1 + upto(static_cast<int>(std::min(t.pvert[e.first], t.gvert[e.second])) - 1));
        }
        vec64 poff, want;
        if (ev_check_tables(t, C, poff)) {
            rejected++;
            continue;
        }
        const EvScanPlan p = ev_plan_scan(t, poff, C, O, min_region);
        int A;
        int64_t total;
        restated(t, O, min_region, want, A, total);
        differ += !(p.words == want && p.A == A && p.total == total && p.U == A * O && static_cast<int>(p.cls_of.size()) == A);
        const EvWords<const int64_t> w = ev_words<const int64_t>(p.words.data(), G, K, static_cast<int64_t>(pg.size()), A);
        for (int a = 0; a < A; a++) {
            differ += p.cls_of[a] != w.s_cls[a];
            pred_only += w.s_p1[a] == 0 && w.s_npred[a] > 0;
        }
        fewer_slots += A < C;
        pairs += static_cast<int64_t>(pg.size());
    }
    CHECK(differ == 0 && rejected == 0);
    CHECK(fewer_slots > 100 && pred_only > 100 && pairs > 10000);  // the cases have classes without a slot, slots without pairs
}

static void word_order()
{
    const int64_t G = 5, K = 3, NP = 7, A = 2;
    vec64 block(2 * G + 4 * K + 3 * NP + 7 * A);
    int64_t *base = block.data();
    const EvWords<int64_t> w = ev_words(base, G, K, NP, A);
    int64_t *const sec[] = {w.gvert, w.gid,    w.pvert, w.pvoid,   w.pslot,   w.pscore, w.q_gt,    w.q_pred, w.q_int,
                            w.s_p0,  w.s_p1,   w.s_nfilt, w.s_npred, w.s_cls, w.s_exoff, w.s_cap,  w.end};
    const int64_t len[] = {G, G, K, K, K, K, NP, NP, NP, A, A, A, A, A, A, A};
    CHECK(sec[0] == base);
    for (int i = 0; i < 16; i++) CHECK(sec[i + 1] - sec[i] == len[i]);
    CHECK(w.end - base == 2 * G + 4 * K + 3 * NP + 7 * A);
}

static void append_limit()
{
    const char *m = "more than 2^31 examples";
    const int64_t lim = int64_t(1) << 31;
    CHECK(is(ev_check_append(0, 0, 0, 0), nullptr));
    CHECK(is(ev_check_append(lim - 11, 0, 10, 1), nullptr));   // 2^31 - 1 examples
    CHECK(is(ev_check_append(lim - 10, 0, 10, 1), m));         // 2^31
    CHECK(is(ev_check_append(10, 0, lim - 11, 1), nullptr));
    CHECK(is(ev_check_append(10, 0, lim - 10, 1), m));
    CHECK(is(ev_check_append(5, INT32_MAX - 3, 5, 3), nullptr));   // 2^31 - 1 units
    CHECK(is(ev_check_append(5, INT32_MAX - 3, 5, 4), m));         // 2^31
    CHECK(is(ev_check_append(0, INT32_MAX, 0, 0), nullptr));
    CHECK(is(ev_check_append(0, INT32_MAX, 0, 1), m));
    // a merge's unsigned total
    CHECK(is(ev_check_append(0, 0, (1ull << 31) - 1, 0), nullptr));
    CHECK(is(ev_check_append(0, 0, 1ull << 31, 0), m));
    CHECK(is(ev_check_append(0, 0, 1ull << 63, 0), m));        // negative as int64_t
    CHECK(is(ev_check_append(0, 0, ~0ull, 0), m));
}

static void compact_unpack()
{
    const double nz = -0.0;  // a score whose bits matter
    const vec64 w{1, 2,  5001, 8002,  120, 70,                      // G = 2: class, id, vert
                  2, 1, 1,  90, 80, 60,  3, 0, 9,  bits(0.75), bits(nz), bits(1e-300),  // K = 3: class, vert, void, score
                  2, 0,  1, 0,  55, 66,                              // NP = 2: prediction, instance, intersection
                  -1};
    CHECK(ev_compact_words(2, 3, 2) == w.size() - 1);
    const EvTables t = ev_unpack_tables(w.data(), 2, 3, 2);
    CHECK((t.gcls == std::vector<int32_t>{1, 2}) && (t.gid == std::vector<int32_t>{5001, 8002}) && (t.gvert == vec64{120, 70}));
    CHECK((t.pcls == std::vector<int32_t>{2, 1, 1}) && (t.pvert == vec64{90, 80, 60}) && (t.pvoid == vec64{3, 0, 9}));
    CHECK(t.pscore.size() == 3 && t.pscore[0] == 0.75 && bits(t.pscore[1]) == bits(nz) && t.pscore[2] == 1e-300);
    CHECK((t.ppred == std::vector<int32_t>{2, 0}) && (t.pgt == std::vector<int32_t>{1, 0}) && (t.pint == vec64{55, 66}));
    const int64_t none[1] = {-1};
    const EvTables e = ev_unpack_tables(none, 0, 0, 0);
    CHECK(ev_compact_words(0, 0, 0) == 0 && e.gcls.empty() && e.pscore.empty() && e.pint.empty());
}

// ---- the state buffer -----------------------------------------------------------------------------
struct Cfg {
    std::vector<int32_t> ids{3, 5, 8};
    std::vector<double> ov{0.5, 0.25};
    int64_t min_region = 100;
    bool no_class = false;
};

// C = 3, O = 2, 5 runs over the 6 cells (cell 3 is empty), in exactly-sized storage so that a read past
// any section's end is a heap overflow
static std::vector<int64_t> valid_state(const Cfg &c, EvLayout &L)
{
    const int64_t R = 5;
    L = ev_layout(3, 2, R);
    std::vector<int64_t> b(L.bytes / 8, 0);
    char *p = reinterpret_cast<char *>(b.data());
    const int64_t hdr[6] = {kEvStateWord, 3, 2, c.min_region, c.no_class ? 1 : 0, R};
    const int64_t roff[7] = {0, 1, 2, 3, 3, 4, 5}, hf[6] = {0, 2, 0, 0, 7, 0};
    const uint32_t fl[6] = {3, 3, 1, 2, 3, 0}, nt[5] = {1, 0, 2, 1, 1}, nf[5] = {0, 4, 0, 1, 0};
    const uint64_t key[5] = {10, 20, 30, 40, 50};
    std::memcpy(p, hdr, 48), std::memcpy(p + L.ids, c.ids.data(), 12), std::memcpy(p + L.ov, c.ov.data(), 16);
    std::memcpy(p + L.roff, roff, 56), std::memcpy(p + L.hf, hf, 48), std::memcpy(p + L.fl, fl, 24);
    std::memcpy(p + L.key, key, 40), std::memcpy(p + L.nt, nt, 20), std::memcpy(p + L.nf, nf, 20);
    return b;
}

// what the host does with the first `bytes` bytes of a buffer: header, then the middle sections, each
// copied out at its exact size before it is checked
static const char *parse(const std::vector<int64_t> &buf, int64_t bytes, const Cfg &c, std::vector<int> &cells)
{
    const bool has = bytes >= static_cast<int64_t>(kEvStateHeader);
    std::vector<int64_t> hdr(buf.begin(), buf.begin() + (has ? 6 : 0));
    int64_t R = -7;
    const int C = static_cast<int>(c.ids.size()), O = static_cast<int>(c.ov.size());
    if (const char *m = ev_check_state_header(has ? hdr.data() : nullptr, bytes, C, O, c.min_region, c.no_class, R)) return m;
    const EvLayout L = ev_layout(C, O, R);
    if (L.bytes > buf.size() * 8) return "the check program's buffer is smaller than the accepted size";
    std::vector<int64_t> mid(buf.begin() + L.ids / 8, buf.begin() + L.key / 8);
    return ev_check_state_sections(mid.data(), L, c.ids, c.ov, cells);
}

static void state_buffer()
{
    const char *m_trunc = "state buffer is truncated", *m_ver = "not a state buffer of this version",
               *m_cfg = "state buffer of another configuration", *m_runs = "bad run count",
               *m_roff = "run offsets must ascend from 0 to the run count", *m_hf = "negative hard false negative count",
               *m_fl = "unknown flag bits";
    const Cfg cfg;
    EvLayout L;
    const std::vector<int64_t> good = valid_state(cfg, L);
    // the sections of include/mcgraph.h: 48 header bytes, int32 ids [C] padded to 8, double overlaps [O], int64 run_off
    // [C * O + 1], int64 hard_fn [C * O], uint32 flags [C * O] padded, uint64 key [R], uint32 n_true, n_false [R] padded
    CHECK(L.ids == 48 && L.ov == 48 + 16 && L.roff == 64 + 16 && L.hf == 80 + 56 && L.fl == 136 + 48 && L.key == 184 + 24);
    CHECK(L.nt == 208 + 40 && L.nf == 248 + 24 && L.bytes == 272 + 24);
    const EvLayout L0 = ev_layout(1, 1, 0);
    CHECK(L0.ov == 56 && L0.roff == 64 && L0.hf == 80 && L0.fl == 88 && L0.key == 96 && L0.nt == 96 && L0.bytes == 96);
    const int64_t bytes = static_cast<int64_t>(L.bytes);
    std::vector<int> cells{9};
    CHECK(is(parse(good, bytes, cfg, cells), nullptr) && (cells == std::vector<int>{0, 1, 2, 4, 5}));
    CHECK(is(parse(good, bytes + 64, cfg, cells), nullptr));  // a longer byte count is no error

    auto with = [&](const std::function<void(char *)> &f) {
        std::vector<int64_t> b = good;
        f(reinterpret_cast<char *>(b.data()));
        return b;
    };
    auto word = [](size_t at, int64_t v) { return [=](char *p) { std::memcpy(p + at, &v, 8); }; };
    auto refused = [&](const std::vector<int64_t> &b, int64_t n, const Cfg &c, const char *msg) {
        std::vector<int> cl;
        return is(parse(b, n, c, cl), msg);
    };
    CHECK(refused(good, 40, cfg, m_trunc));          // header only half
    CHECK(refused(good, 0, cfg, m_trunc));
    CHECK(refused(good, bytes - 8, cfg, m_trunc));   // truncated
    CHECK(refused(std::vector<int64_t>(good.begin(), good.end() - 1), bytes - 8, cfg, m_trunc));
    CHECK(refused(with(word(0, kEvStateWord ^ 1)), bytes, cfg, m_ver));                  // magic
    CHECK(refused(with(word(0, kEvStateWord + (int64_t(1) << 32))), bytes, cfg, m_ver)); // version
    for (int i = 1; i <= 4; i++) {                   // C, O, min_region_size, no_class
        int64_t v;
        std::memcpy(&v, reinterpret_cast<const char *>(good.data()) + 8 * i, 8);
        CHECK(refused(with(word(8 * i, v + 1)), bytes, cfg, m_cfg));
    }
    Cfg other = cfg;
    other.ids = {5, 3, 8};                           // class table permuted
    CHECK(refused(good, bytes, other, m_cfg));
    other = cfg, other.ov[1] = std::nextafter(other.ov[1], 1.0);   // an overlap one ulp off
    CHECK(refused(good, bytes, other, m_cfg));
    other = cfg, other.min_region = 101;
    CHECK(refused(good, bytes, other, m_cfg));
    other = cfg, other.no_class = true;
    CHECK(refused(good, bytes, other, m_cfg));
    other = cfg, other.ids.pop_back();               // one class fewer
    CHECK(refused(good, bytes, other, m_cfg));
    CHECK(refused(with(word(40, -1)), bytes, cfg, m_runs));
    CHECK(refused(with(word(40, int64_t(1) << 40)), bytes, cfg, m_runs));
    CHECK(refused(with(word(40, int64_t(1) << 31)), bytes, cfg, m_runs));
    CHECK(refused(with(word(40, 6)), bytes, cfg, m_trunc));        // one run more than the buffer holds
    // new: the largest run count with a byte count far too small is refused by size, before anything is indexed
    CHECK(refused(with(word(40, (int64_t(1) << 31) - 1)), bytes, cfg, m_trunc));
    CHECK(ev_layout(3, 2, (int64_t(1) << 31) - 1).bytes == 200 + 16 * (size_t(1) << 31));
    CHECK(refused(with(word(40, 4)), bytes, cfg, m_roff));         // fits, but run_off ends at 5
    CHECK(refused(with(word(L.roff, 1)), bytes, cfg, m_roff));     // not from 0
    CHECK(refused(with(word(L.roff + 8 * 6, 4)), bytes, cfg, m_roff));   // not to R
    CHECK(refused(with(word(L.roff + 8 * 2, 0)), bytes, cfg, m_roff));   // descending
    CHECK(refused(with(word(L.roff + 8 * 3, 9)), bytes, cfg, m_roff));   // past R and back
    CHECK(refused(with(word(L.hf + 8 * 2, -1)), bytes, cfg, m_hf));
    auto flag = [&](int cell, uint32_t v) { return [=](char *p) { std::memcpy(p + L.fl + 4 * cell, &v, 4); }; };
    CHECK(refused(with(flag(2, 4 | 3)), bytes, cfg, m_fl));        // flag bit 4
    CHECK(refused(with(flag(5, 0x80000000u)), bytes, cfg, m_fl));
    // today's order within a cell and over the cells: run_off, hard_fn, flags
    auto both = [](std::function<void(char *)> a, std::function<void(char *)> b) { return [=](char *p) { a(p), b(p); }; };
    CHECK(refused(with(both(word(L.hf + 8 * 1, -1), flag(1, 8))), bytes, cfg, m_hf));
    CHECK(refused(with(both(word(L.hf + 8 * 4, -1), flag(1, 8))), bytes, cfg, m_fl));
    CHECK(refused(with(both(word(L.roff + 8 * 5, 2), flag(0, 8))), bytes, cfg, m_fl));
    CHECK(refused(with(both(word(L.roff, 1), word(0, 0))), bytes, cfg, m_ver));
    // an empty buffer of a context that has only begun
    const EvLayout Le = ev_layout(3, 2, 0);
    std::vector<int64_t> empty(good.begin(), good.begin() + Le.bytes / 8);
    std::memset(reinterpret_cast<char *>(empty.data()) + L.roff, 0, Le.bytes - L.roff);
    empty[5] = 0;
    CHECK(is(parse(empty, static_cast<int64_t>(Le.bytes), cfg, cells), nullptr) && cells.empty());
}

int main()
{
    worked_scan();
    rejections();
    random_tables();
    word_order();
    append_limit();
    compact_unpack();
    state_buffer();
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
