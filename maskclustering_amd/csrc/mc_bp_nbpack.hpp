// mc_bp_nbpack.hpp — S1 denoise: how the entries of an eps-neighbour list reach their 16-byte words.
// Plain C++17 without a HIP include, usable from host and device: the own-walk list builder of the LDS
// denoise classes (lds_eps_own, mc_bp_denoise_lds.inl) packs with it, every class reads slots with it
// (nb_ent), and scripts/bp_nbpack_check.cpp checks it on the CPU (tests/test_bp_nbpack_cpu.py).
// The layout (mc_bp_denoise_lds.inl, "Per-workgroup eps-neighbour lists"): slot k of sorted position q is
// half-word k % 8 of the 16-byte word (k / 8) * N + q; the low half of a 32-bit register is the even slot.
//  * NbPack holds the word being filled in four 32-bit registers.  push() shifts the whole 128 bits
//    down by one half-word and puts the new entry on top, so after eight pushes entry j of the word
//    sits in half-word j: static register names only, no indexed register array.
//  * A list of cnt entries fills words 0 .. (cnt - 1) / 8.  The builder stores a word after every
//    eighth push while the count is within the cap (nb_store_full), and once after the walk the last,
//    partial word (nb_store_tail) with its unused half-words zero (flush()).  Entries past the cap
//    are counted and not stored: the count alone tells the consumers that the list is not complete.
//  * nb_slot() is the consumers' extraction (nb_ent) of slot k from the 32-bit words of a list.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MC_NB_HD __host__ __device__ __forceinline__
#else
#define MC_NB_HD inline
#endif

namespace mc {

constexpr int kNbWordSlots = 8;  // u16 entries per 16-byte word

struct NbPack {
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;  // half-words 0-1, 2-3, 4-5, 6-7 of the word

    // the 128 bits move down one half-word; e (16 bits) becomes half-word 7
    MC_NB_HD void push(uint32_t e)
    {
        a0 = (a0 >> 16) | (a1 << 16);
        a1 = (a1 >> 16) | (a2 << 16);
        a2 = (a2 >> 16) | (a3 << 16);
        a3 = (a3 >> 16) | (e << 16);
    }

    // after r = 1 .. 7 pushes into a word: the r entries move to half-words 0 .. r - 1, the rest zero
    // (8 - r half-words down, by the bits of that shift: selects, no loop and no indexed registers)
    MC_NB_HD void flush(int r)
    {
        const int s = (kNbWordSlots - r) & (kNbWordSlots - 1);
        if (s & 4) {
            a0 = a2;
            a1 = a3;
            a2 = 0;
            a3 = 0;
        }
        if (s & 2) {
            a0 = a1;
            a1 = a2;
            a2 = a3;
            a3 = 0;
        }
        if (s & 1) push(0);
    }
};

// after the push that made the count cnt (1-based): is a word complete and within the cap?
MC_NB_HD bool nb_store_full(int cnt, int cap) { return (cnt & (kNbWordSlots - 1)) == 0 && cnt <= cap; }
// after the walk: does a partial last word remain to be stored?
MC_NB_HD bool nb_store_tail(int cnt, int cap) { return (cnt & (kNbWordSlots - 1)) != 0 && cnt < cap; }
// the word (index within the point's list) that the store after count cnt writes
MC_NB_HD int nb_store_word(int cnt) { return (cnt - 1) / kNbWordSlots; }

// slot k of a list's 32-bit words w[0 ..] (word u of the list = w[4 u .. 4 u + 3])
MC_NB_HD uint32_t nb_slot(const uint32_t *w, int k) { return (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu; }

}  // namespace mc
