// BC7 block dedupe: the hash, the table walk and the equality rule (bc7_encode.hip: bc7_dedupe_insert_kernel / bc7_dedupe_resolve_kernel).
//
// D3DX_BC7::Encode is a pure function of a block's sixteen texels and the flags, so two blocks of a pass with the same input get the same
// sixteen bytes and only one of them - the LEADER, the smallest pass-local block index of the group - has to be searched. The KEY of a
// block is what Encode reads: the 64 float bit patterns load_block_texel returns (after the format conversion and the partial-block
// replication); the packed RGBA8 words are a function of those floats. Two blocks pair up only when all 64 words are equal - the hash
// finds the candidates, the comparison decides - so a pair is exact whatever the source format and whatever the hash does.
//
// The table: open addressing, linear probing from slot_start, at most kProbeBound probes; a slot is claimed with a compare-and-swap on its
// key word and the leader is folded in with a minimum on its value word, so the table's content does not depend on who came first. A
// block that finds no slot within the bound is simply encoded. The table is cleared to 0xFF bytes: key kEmptyKey, leader 0xFFFFFFFF.
//
// Plain C++ as well as HIP: tests/cpp/bc7_dedupe_check.cpp mirrors the two kernels serially on the host with these functions.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define DXTEX_DD_HD __host__ __device__
#else
#define DXTEX_DD_HD
#endif

namespace dxtex
{
namespace bc7dd
{
constexpr uint32_t kKeyWords = 64;                 // sixteen texels x the bit patterns of four floats
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kProbeBound = 32;
constexpr uint32_t kSlotsPerBlock = 2;             // table slots per block of the pass

struct Slot { unsigned long long key; uint32_t leader; uint32_t pad; };    // 16 bytes: one probe touches one slot

DXTEX_DD_HD inline uint64_t mix64(uint64_t x)      // splitmix64's finaliser
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the running hash over the key's words, in order
DXTEX_DD_HD inline uint64_t hash_word(uint64_t h, uint32_t w)
{
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

// `bits` < 64 keeps only that many bits (a development knob: unequal blocks then share a hash and the comparison has to tell them apart)
DXTEX_DD_HD inline unsigned long long hash_finish(uint64_t h, uint32_t bits)
{
    h = mix64(h);
    if (bits < 64u) h &= (1ull << bits) - 1ull;
    return (h == kEmptyKey) ? 0ull : h;
}

DXTEX_DD_HD inline unsigned long long hash_key(const uint32_t* words, uint32_t bits)
{
    uint64_t h = 0;
    for (uint32_t i = 0; i < kKeyWords; ++i) h = hash_word(h, words[i]);
    return hash_finish(h, bits);
}

DXTEX_DD_HD inline uint32_t slot_start(unsigned long long h, uint32_t slots)
{
    return uint32_t(((mix64(h ^ 0xD6E8FEB86659FD93ull) >> 32) * uint64_t(slots)) >> 32);       // < slots
}
DXTEX_DD_HD inline uint32_t slot_at(uint32_t start, uint32_t i, uint32_t slots) { return (start + i) % slots; }

// Puts block `nb` under hash `h`: the slot that holds h afterwards, or kNoSlot when the bound ran out. cas(slot, h) stores h into an empty
// slot's key word and returns what the word held before; amin(slot, nb) folds nb into the slot's leader. Never waits for anybody.
template<class Cas, class Amin>
DXTEX_DD_HD inline uint32_t insert(unsigned long long h, uint32_t nb, uint32_t slots, Cas cas, Amin amin)
{
    const uint32_t start = slot_start(h, slots);
    const uint32_t bound = (slots < kProbeBound) ? slots : kProbeBound;
    for (uint32_t i = 0; i < bound; ++i)
    {
        const uint32_t s = slot_at(start, i, slots);
        const unsigned long long prev = cas(s, h);
        if (prev == kEmptyKey || prev == h) { amin(s, nb); return s; }
    }
    return kNoSlot;
}

// The block `nb` may copy, by its hash alone: the leader of its slot when that is an earlier block, else nb itself.
DXTEX_DD_HD inline uint32_t candidate_leader(const Slot* table, uint32_t slot, uint32_t nb)
{
    if (slot == kNoSlot) return nb;
    const uint32_t l = table[slot].leader;
    return (l < nb) ? l : nb;
}

// The equality rule: every word of the key. A hash match alone is never enough.
DXTEX_DD_HD inline bool keys_equal(const uint32_t* x, const uint32_t* y)
{
    uint32_t diff = 0;
    for (uint32_t i = 0; i < kKeyWords; ++i) diff |= x[i] ^ y[i];
    return diff == 0;
}
} // namespace bc7dd
} // namespace dxtex
