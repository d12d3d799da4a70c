// S1 denoise list packing (maskclustering_amd/csrc/mc_bp_nbpack.hpp) on the CPU: a list builder written
// as lds_eps_own (mc_bp_denoise_lds.inl) is, run for every count 0 .. 66 and read back as nb_load / nb_ent
// read it.  Built and run by tests/test_bp_nbpack_cpu.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/bp_nbpack_check.cpp -o bp_nbpack_check && ./bp_nbpack_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "mc_bp_nbpack.hpp"

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("line %d: %s\n", __LINE__, #cond);                \
            bad++;                                                   \
        }                                                            \
    } while (0)

using namespace mc;

constexpr int kCap = 64;        // kBpNbCap
constexpr int kWords = kCap / kNbWordSlots;
constexpr uint32_t kFill = 0xA5A5A5A5u;  // what the region holds before the build

// entry k of the list of position q: 16 bits, never zero, different in every slot
static uint32_t entry(int q, int k) { return ((static_cast<uint32_t>(k) * 2654435761u + 40503u * q) >> 7 & 0xFFFFu) | 1u; }

// the builder: cnt entries of position q into a region of N positions (uint4 index u * N + q, as four
// 32-bit words each); returns the count and the number of stores
static int build(std::vector<uint32_t> &region, int N, int q, int cnt, int &stores)
{
    NbPack acc;
    int c = 0;
    stores = 0;
    auto put = [&](int count) {
        const size_t w = (static_cast<size_t>(nb_store_word(count)) * N + q) * 4;
        CHECK(nb_store_word(count) >= 0 && nb_store_word(count) < kWords);
        region[w] = acc.a0, region[w + 1] = acc.a1, region[w + 2] = acc.a2, region[w + 3] = acc.a3;
        stores++;
    };
    for (int k = 0; k < cnt; k++) {
        acc.push(entry(q, k));
        c++;
        if (nb_store_full(c, kCap)) put(c);
    }
    if (nb_store_tail(c, kCap)) {
        acc.flush(c & (kNbWordSlots - 1));
        put(c);
    }
    return c;
}

// nb_load: the words of the first cnt slots, the others zero
static void load(const std::vector<uint32_t> &region, int N, int q, int cnt, uint32_t (&w)[4 * kWords])
{
    for (int u = 0; u < kWords; u++)
        for (int j = 0; j < 4; j++) w[4 * u + j] = kNbWordSlots * u < cnt ? region[(static_cast<size_t>(u) * N + q) * 4 + j] : 0u;
}

static void counts()
{
    const int N = 3;
    for (int cnt = 0; cnt <= 66; cnt++)
        for (int q = 0; q < N; q++) {
            std::vector<uint32_t> region(static_cast<size_t>(kWords) * N * 4, kFill);
            int stores = 0;
            const int c = build(region, N, q, cnt, stores);
            CHECK(c == cnt);  // entries past the cap are counted
            const int kept = cnt < kCap ? cnt : kCap;
            const int words = (kept + kNbWordSlots - 1) / kNbWordSlots;
            CHECK(stores == words);  // one store per word: a flush at every multiple of 8, one partial word
            // every word of q up to the last is written, nothing else in the region is
            for (int u = 0; u < kWords; u++)
                for (int p = 0; p < N; p++)
                    for (int j = 0; j < 4; j++) {
                        const uint32_t v = region[(static_cast<size_t>(u) * N + p) * 4 + j];
                        if (p != q || u >= words) CHECK(v == kFill);
                    }
            // half-word order within the words, and zeros after the last entry of a partial word
            for (int k = 0; k < words * kNbWordSlots; k++) {
                const uint32_t word32 = region[(static_cast<size_t>(k / kNbWordSlots) * N + q) * 4 + (k % kNbWordSlots) / 2];
                const uint32_t h = (word32 >> (16 * (k & 1))) & 0xFFFFu;
                CHECK(h == (k < kept ? entry(q, k) : 0u));
            }
            // round trip through the consumers' load and extraction (a list within the cap)
            if (cnt <= kCap) {
                uint32_t w[4 * kWords];
                load(region, N, q, cnt, w);
                for (int k = 0; k < cnt; k++) CHECK(nb_slot(w, k) == entry(q, k));
                for (int k = cnt; k < kCap; k++) CHECK(nb_slot(w, k) == 0u);
            }
        }
}

static void store_rules()
{
    for (int cnt = 1; cnt <= 66; cnt++) {
        CHECK(nb_store_full(cnt, kCap) == (cnt % 8 == 0 && cnt <= 64));
        CHECK(nb_store_tail(cnt, kCap) == (cnt % 8 != 0 && cnt < 64));
        CHECK(!(nb_store_full(cnt, kCap) && nb_store_tail(cnt, kCap)));
    }
    CHECK(!nb_store_tail(0, kCap));  // an empty list stores nothing (nb_store_full only follows a push)
    CHECK(nb_store_word(1) == 0 && nb_store_word(8) == 0 && nb_store_word(9) == 1 && nb_store_word(64) == 7);
}

static void pack_steps()
{
    // push: eight entries land in half-words 0 .. 7 in order; a ninth starts over on top
    NbPack a;
    for (uint32_t k = 1; k <= 8; k++) a.push(k);
    CHECK(a.a0 == 0x00020001u && a.a1 == 0x00040003u && a.a2 == 0x00060005u && a.a3 == 0x00080007u);
    a.push(9);
    CHECK(a.a3 == 0x00090008u && a.a0 == 0x00030002u);
    // flush after r pushes on top of a full earlier word: nothing of the earlier word survives
    for (int r = 1; r <= 7; r++) {
        NbPack b;
        for (uint32_t k = 0; k < 8; k++) b.push(0xF000u + k);
        for (int k = 0; k < r; k++) b.push(0x100u + static_cast<uint32_t>(k));
        b.flush(r);
        const uint32_t w[4] = {b.a0, b.a1, b.a2, b.a3};
        for (int k = 0; k < 8; k++) CHECK(nb_slot(w, k) == (k < r ? 0x100u + static_cast<uint32_t>(k) : 0u));
    }
    // an entry with bits above 16 would spill into the next slot: the builder passes 16 bits
    // (position 14 bits | class << 14), which push() relies on
    NbPack c;
    c.push(0xFFFFu);
    c.push(0x0001u);
    CHECK(c.a3 == 0x0001FFFFu);
}

int main()
{
    pack_steps();
    store_rules();
    counts();
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
