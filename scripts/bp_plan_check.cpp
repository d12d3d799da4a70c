// S1 batch planning (maskclustering_amd/csrc/mc_bp_plan.hpp) on the CPU: worked cases of every rule
// and the termination of the grow-and-redo loop.  Built and run by tests/test_bp_plan_cpu.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/bp_plan_check.cpp -o bp_plan_check && ./bp_plan_check
#include <cstdio>

#include "mc_bp_plan.hpp"

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("line %d: %s\n", __LINE__, #cond);                \
            bad++;                                                   \
        }                                                            \
    } while (0)

using namespace mc;

static void frames_per_batch()
{
    const size_t HW = 4800;
    CHECK(bp_frames_per_batch(10, HW, 4 * HW, 0) == 4);  // three batches: 4, 4, 2
    CHECK(bp_frames_per_batch(9, HW, 4 * HW + 17, 0) == 3);  // dealt equally: 3, 3, 3
    for (size_t budget : {size_t(1), HW, 1000 * HW}) CHECK(bp_frames_per_batch(0, HW, budget, 0) == 1);
    CHECK(bp_frames_per_batch(5, HW, 1, 0) == 1);  // a budget of one pixel still takes a frame
    CHECK(bp_frames_per_batch(10, HW, 10 * HW, 3) == 4);
    CHECK(bp_frames_per_batch(10, HW, 64 * HW, 3) == 4);
    CHECK(bp_frames_per_batch(10, HW, 10 * HW, 1) == 10);
    CHECK(bp_frames_per_batch(10, HW, 10 * HW, 16) == 1);
}

static void pixel_budget()
{
    for (size_t HW : {size_t(48) * 64, size_t(480) * 640}) {
        // the budget test_two_contexts_share_a_device_under_budgets sets: 198 B per frame pixel at share 1
        const size_t px = bp_pixel_budget(224 * 3 * HW, 1.0, HW);
        CHECK(px == 224 * 3 * HW / 198);
        CHECK(px / HW == 3);
        CHECK(bp_frames_per_batch(10, HW, px, 0) == 3);
        CHECK(bp_pixel_budget(0, 1.0, HW) == HW);                  // never below a frame
        CHECK(bp_pixel_budget(HW, 0.5, HW) == HW);
        CHECK(bp_pixel_budget(~size_t(0) >> 1, 1e-4, HW) == (size_t(1) << 31) - 1);  // never above 2^31 - 1
        CHECK(bp_pixel_budget(size_t(300) << 30, 1e-4, HW) == (size_t(1) << 31) - 1);
    }
    CHECK(kBpBytesPerFramePixel + kBpBytesPerMaskPixel == 198);
}

static void mask_cap()
{
    CHECK(bp_mask_cap(4, 1000, 0.25) == 3086);
    CHECK(bp_mask_cap(4, 1000, 1.0) == 5024);
    for (double frac : {0.0, 1e-4, 0.3, 0.95, 1.0, 7.0})
        for (int FB : {1, 4, 300}) CHECK(bp_mask_cap(FB, 1000, frac) <= size_t(FB) * 1000 + 1024);
}

static void byte_budget()
{
    const size_t G = size_t(1) << 30;
    CHECK(bp_byte_budget(12345, 100 * G, 288 * G, 7 * G) == 12345);
    CHECK(bp_byte_budget(0, 280 * G, 288 * G, 0) == 288 * G / 100 * 40);            // 40 % of the device
    CHECK(bp_byte_budget(0, 20 * G, 288 * G, 10 * G) == (20 * G + 10 * G) / 100 * 65);  // 65 % of free + held
    CHECK(bp_byte_budget(0, 0, 0, 7 * G) == 7 * G);
    CHECK(bp_held_bytes(10, 100) == 10 * kBpBytesPerMaskPixel + 100 * kBpBytesPerFramePixel);
}

static void shrink()
{
    for (size_t HW : {size_t(4800), size_t(307200)})
        for (int FB : {1, 3, 64})
            for (double frac : {1e-4, 0.3, 1.0})
                for (size_t frames_worth : {size_t(0), size_t(1), size_t(3), size_t(1000)}) {
                    const size_t bud = frames_worth * HW * 198;
                    const int fb = bp_shrink_after_overflow(FB, HW, frac, bud, false);
                    CHECK(fb >= 1 && fb <= FB);
                    CHECK(bp_shrink_after_overflow(FB, HW, frac, bud, true) == FB);
                }
    CHECK(bp_shrink_after_overflow(64, 4800, 1.0, 3 * 4800 * 198, false) == 3);
    CHECK(bp_redo_mask_cap(3, 64, 4800, 0.5, 1 << 20) == bp_mask_cap(3, 4800, 0.5));  // fewer frames: the share's room
    CHECK(bp_redo_mask_cap(4, 4, 1000, 0.25, 4000) == 5024);                          // the same frames: every pixel listed
}

// bp_run's redo loop with the header's functions: every batch shows `share` of its frame pixels as
// mask pixels; it must get through all F frames with at most F + 2 redos
static int redos(int F, size_t HW, double share, double mfrac0, size_t bud_bytes)
{
    const double mfrac = std::min(1.0, std::max(mfrac0, 1e-4));
    int FB = bp_frames_per_batch(F, HW, bp_pixel_budget(bud_bytes, mfrac, HW), 0);
    size_t cap = bp_mask_cap(FB, HW, mfrac) + 1;
    int n = 0;
    for (int b0 = 0; b0 < F && n <= F + 2;) {
        const int fb = std::min(FB, F - b0);
        const size_t npx = static_cast<size_t>(share * fb * HW);
        if (npx > cap) {
            const double frac = static_cast<double>(npx) / (static_cast<double>(fb) * HW);
            const int fb_was = FB;
            FB = bp_shrink_after_overflow(FB, HW, frac, bud_bytes, false);
            cap = std::max(cap, bp_redo_mask_cap(FB, fb_was, HW, frac, npx) + 1);
            n++;
            continue;
        }
        b0 += fb;
    }
    return n;
}

static void termination()
{
    for (int F : {1, 7, 64})
        for (size_t HW : {size_t(4800), size_t(307200)})
            for (double share : {0.01, 0.3, 1.0})
                for (double mfrac0 : {1e-4, 0.02, 1.0})
                    for (int admits : {1, 3, F}) {
                        const int n = redos(F, HW, share, mfrac0, size_t(admits) * HW * 198);
                        if (n > F + 2) printf("F=%d HW=%zu share=%g mfrac=%g admits=%d: %d redos\n", F, HW, share, mfrac0, admits, n);
                        CHECK(n <= F + 2);
                    }
}

int main()
{
    frames_per_batch();
    pixel_budget();
    mask_cap();
    byte_budget();
    shrink();
    termination();
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
