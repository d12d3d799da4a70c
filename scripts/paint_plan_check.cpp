// paint_plan_check.cpp — the host decisions and the bit arithmetic of the label painter
// (maskclustering_amd/csrc/mc_paint_plan.hpp) checked on the CPU: the refusals with their messages, the
// rounds of frames against a budget (every frame once, in order, each round within the budget, a frame
// that alone does not fit refused), the selection and order rule at its edges, four mask bytes -> four
// bits for every byte pattern that matters, the bit-sliced fold and the 8 x 8 transpose against the
// plain per-pixel loop.  A stand-alone program (tests/test_paint_plan_cpu.py builds it with the address
// and undefined-behaviour sanitizers); prints bad=<failures>.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "mc_paint_plan.hpp"

static int bad = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            bad++;                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                         \
    } while (0)

using Rounds = std::vector<std::pair<int, int>>;

int main()
{
    std::string why;
    // the refusals
    {
        const int64_t ok[4] = {0, 3, 3, 1027}, down[3] = {0, 5, 4}, from1[2] = {1, 2}, many[3] = {0, 1, 1026};
        CHECK(mc::paint_check_args(3, 48, 40, ok, mc::kPaintU8, 400, &why) == mc::kPaintAccept);
        CHECK(mc::paint_check_args(0, 48, 40, ok, mc::kPaintF32, 0, &why) == mc::kPaintAccept);
        CHECK(mc::paint_check_args(2, 48, 40, down, 0, 400, &why) == mc::kPaintInvalid && why.find("non-decreasing") != std::string::npos);
        CHECK(mc::paint_check_args(1, 48, 40, from1, 0, 400, &why) == mc::kPaintInvalid && why.find("inst_off[0]") != std::string::npos);
        CHECK(mc::paint_check_args(2, 48, 40, many, 0, 400, &why) == mc::kPaintInvalid && why.find("frame 1") != std::string::npos &&
              why.find("MC_PAINT_MAX_INSTANCES") != std::string::npos);
        CHECK(mc::paint_check_args(3, 48, 40, ok, 2, 400, &why) == mc::kPaintInvalid && why.find("mask_dtype") != std::string::npos);
        CHECK(mc::paint_check_args(3, 48, 40, ok, -1, 400, &why) == mc::kPaintInvalid);
        CHECK(mc::paint_check_args(3, 0, 40, ok, 0, 400, &why) == mc::kPaintInvalid && why.find("H or W") != std::string::npos);
        CHECK(mc::paint_check_args(3, 48, -1, ok, 0, 400, &why) == mc::kPaintInvalid);
        CHECK(mc::paint_check_args(3, 46341, 46341, ok, 0, 400, &why) == mc::kPaintInvalid && why.find("2^31") != std::string::npos);
        CHECK(mc::paint_check_args(3, 2147483647, 1, ok, 0, 400, &why) == mc::kPaintAccept);
        CHECK(mc::paint_check_args(3, 48, 40, ok, 0, -1, &why) == mc::kPaintInvalid && why.find("min_pixels") != std::string::npos);
        CHECK(mc::paint_check_args(-1, 48, 40, ok, 0, 400, &why) == mc::kPaintInvalid);
        CHECK(mc::paint_check_args(3, 48, 40, nullptr, 0, 400, &why) == mc::kPaintInvalid);
    }
    // bytes and rounds
    CHECK(mc::paint_words(1) == 1 && mc::paint_words(64) == 1 && mc::paint_words(65) == 2 && mc::paint_words(851) == 14);
    CHECK(mc::paint_round_bytes(3, 851, mc::kPaintU8, false) == 3 * 14 * 8);
    CHECK(mc::paint_round_bytes(3, 851, mc::kPaintU8, true) == 3 * (14 * 8 + 851));
    CHECK(mc::paint_round_bytes(3, 851, mc::kPaintF32, true) == 3 * (14 * 8 + 4 * 851));
    CHECK(mc::paint_byte_budget(0) == (1ll << 30) && mc::paint_byte_budget(12345) == 12345);
    {
        const int64_t off[8] = {0, 0, 4, 4, 9, 10, 10, 10};  // 0, 4, 0, 5, 1, 0, 0 instances
        Rounds r;
        const int64_t one = mc::paint_round_bytes(1, 1920, mc::kPaintU8, false);
        CHECK(mc::paint_rounds(7, off, 1920, 0, false, 10 * one, &r, &why) == mc::kPaintAccept && (r == Rounds{{0, 7}}));
        CHECK(mc::paint_rounds(7, off, 1920, 0, false, 9 * one, &r, &why) == mc::kPaintAccept && (r == Rounds{{0, 4}, {4, 7}}));
        CHECK(mc::paint_rounds(7, off, 1920, 0, false, 5 * one, &r, &why) == mc::kPaintAccept && (r == Rounds{{0, 3}, {3, 4}, {4, 7}}));
        CHECK(mc::paint_rounds(7, off, 1920, 0, false, 5 * one - 1, &r, &why) == mc::kPaintUnsupported && r.empty() &&
              why.find("frame 3") != std::string::npos && why.find(std::to_string(5 * one) + " bytes") != std::string::npos);
        CHECK(mc::paint_rounds(0, off, 1920, 0, false, 1, &r, &why) == mc::kPaintAccept && r.empty());
        const int64_t none[3] = {0, 0, 0};
        CHECK(mc::paint_rounds(2, none, 1920, 0, true, 1, &r, &why) == mc::kPaintAccept && (r == Rounds{{0, 2}}));
        // any budget: the rounds tile the frames in order and each fits
        std::mt19937 rng(3);
        for (int rep = 0; rep < 200; rep++) {
            const int F = 1 + rng() % 12;
            std::vector<int64_t> o(F + 1, 0);
            int64_t most = 0;
            for (int f = 0; f < F; f++) {
                const int64_t n = rng() % 7;
                o[f + 1] = o[f] + n, most = std::max(most, n);
            }
            const bool staged = rep & 1;
            const int dt = (rep >> 1) & 1;
            const int64_t budget = mc::paint_round_bytes(most + rng() % 9, 851, dt, staged);
            CHECK(mc::paint_rounds(F, o.data(), 851, dt, staged, budget, &r, &why) == mc::kPaintAccept);
            int at = 0;
            for (auto &x : r) {
                CHECK(x.first == at && x.second > x.first);
                CHECK(mc::paint_round_bytes(o[x.second] - o[x.first], 851, dt, staged) <= budget);
                at = x.second;
            }
            CHECK(at == F);
        }
    }
    // selection and order
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
        const float t = 0.7f;  // float32(0.7) < 0.7: the comparison is float32 against float32
        CHECK(static_cast<double>(t) < 0.7 && mc::paint_selected(t, t));
        CHECK(!mc::paint_selected(std::nextafterf(t, 0.f), t) && mc::paint_selected(std::nextafterf(t, 1.f), t));
        CHECK(!mc::paint_selected(nan, t) && !mc::paint_selected(nan, -inf) && mc::paint_selected(inf, t) && !mc::paint_selected(-inf, t));
        CHECK(mc::paint_before(0.5f, 3, 0.6f, 1) && !mc::paint_before(0.6f, 1, 0.5f, 3));
        CHECK(mc::paint_before(0.5f, 1, 0.5f, 3) && !mc::paint_before(0.5f, 3, 0.5f, 1) && !mc::paint_before(0.5f, 2, 0.5f, 2));
        CHECK(mc::paint_before(0.0f, 1, -0.0f, 2) && mc::paint_before(-0.0f, 1, 0.0f, 2) && !mc::paint_before(-0.0f, 2, 0.0f, 1));
        CHECK(mc::paint_before(inf, 0, inf, 1) && !mc::paint_before(inf, 1, inf, 0));
    }
    // four bytes -> four bits: every combination of the byte values at which the trick could slip
    {
        const unsigned v[8] = {0x00, 0x01, 0x02, 0x03, 0x7f, 0x80, 0x81, 0xff};
        for (int a = 0; a < 8; a++)
            for (int b = 0; b < 8; b++)
                for (int c = 0; c < 8; c++)
                    for (int d = 0; d < 8; d++) {
                        const uint32_t x = v[a] | (v[b] << 8) | (v[c] << 16) | (v[d] << 24);
                        const uint32_t want = (v[a] == 1) | ((v[b] == 1) << 1) | ((v[c] == 1) << 2) | ((v[d] == 1) << 3);
                        CHECK(mc::paint_bits4_u8(x) == want);
                    }
        std::mt19937 rng(11);
        for (int rep = 0; rep < 100000; rep++) {
            uint32_t x = rng();
            if (rep & 1) x &= 0x03030303u;
            uint32_t want = 0;
            for (int k = 0; k < 4; k++) want |= static_cast<uint32_t>(((x >> (8 * k)) & 0xff) == 1) << k;
            CHECK(mc::paint_bits4_u8(x) == want);
        }
    }
    // the transpose, and the fold + label bytes against the per-pixel loop
    {
        std::mt19937_64 rng(5);
        for (int rep = 0; rep < 2000; rep++) {
            const uint64_t x = rng();
            const uint64_t y = mc::paint_transpose8(x);
            for (int r = 0; r < 8; r++)
                for (int c = 0; c < 8; c++) CHECK(((x >> (8 * r + c)) & 1) == ((y >> (8 * c + r)) & 1));
            CHECK(mc::paint_transpose8(y) == x);
        }
        for (int rep = 0; rep < 300; rep++) {
            const int nk = 1 + static_cast<int>(rng() % 255);
            const int left = rep % 3 ? 64 : 1 + static_cast<int>(rng() % 63);
            uint64_t done = left >= 64 ? 0ull : ~0ull << left, lab[8] = {};
            unsigned char want[64] = {};
            for (int k = 0; k < nk && done != ~0ull; k++) {
                uint64_t w = rng() & rng() & rng();
                if (left < 64) w &= ~(~0ull << left);  // a plane's unused bits are zero
                const uint64_t newly = w & ~done;
                for (int p = 0; p < 64; p++)
                    if ((newly >> p) & 1) want[p] = static_cast<unsigned char>(nk - k);
                mc::paint_fold(lab, newly, nk - k);
                done |= newly;
            }
            for (int g = 0; g < 8; g++) {
                const uint64_t bytes = mc::paint_label_bytes(lab, g);
                for (int p = 0; p < 8; p++) CHECK(static_cast<unsigned char>(bytes >> (8 * p)) == want[8 * g + p]);
            }
        }
    }
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
