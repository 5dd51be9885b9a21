// Host mirror of the BC7 block dedupe (directxtex_amd/csrc/dxtex_bc7_dedupe.h; the kernels are bc7_dedupe_insert_kernel and
// bc7_dedupe_resolve_kernel in bc7_encode.hip): insert and resolve run serially over random tiles with the header's own hash, table
// walk and equality rule, and the outcome is compared with counts made without any hash (std::map over the whole key).
//   - every block resolve calls a duplicate has, word for word, the key of its leader; a leader is earlier and is itself encoded;
//   - at full hash width and a table of 2 x blocks slots the duplicates are exactly blocks - distinct keys;
//   - with the hash cut to a few bits (unequal keys collide) the duplicates are exactly the blocks equal to the first block of their
//     hash value - never a block that only shares the hash;
//   - with a table far too small most inserts run out of probes: those blocks are encoded, the others still pair up correctly.
// A stand-alone program (plain C++, no device): the Makefile builds it with AddressSanitizer and UndefinedBehaviorSanitizer.
// usage: bc7_dedupe_check [tiles]
#include "dxtex_bc7_dedupe.h"
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

using namespace dxtex::bc7dd;
typedef std::array<uint32_t, kKeyWords> Key;

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 32);
}

static int g_failures = 0;
#define CHECK(COND, ...) do { if (!(COND)) { if (++g_failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Outcome { std::vector<uint32_t> dupOf; uint32_t dups = 0, noSlot = 0; };

// what the two kernels do, one block after the other
static Outcome run(const std::vector<Key>& blocks, uint32_t bits, uint32_t slots)
{
    const uint32_t n = uint32_t(blocks.size());
    std::vector<Slot> table(slots);
    std::memset(table.data(), 0xFF, table.size() * sizeof(Slot));
    Outcome o; o.dupOf.assign(n, 0);
    std::vector<uint32_t> slotOf(n);
    auto cas = [&](uint32_t s, unsigned long long h) { const unsigned long long prev = table.at(s).key; if (prev == kEmptyKey) table[s].key = h; return prev; };
    auto amin = [&](uint32_t s, uint32_t nb) { if (nb < table.at(s).leader) table[s].leader = nb; };
    // insert, in an order that is not the block order: the leader must come out as the minimum all the same
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; ++i) perm[i] = i;
    for (uint32_t i = n; i > 1; --i) { const uint32_t j = rnd() % i; std::swap(perm[i - 1], perm[j]); }
    for (uint32_t k = 0; k < n; ++k)
    {
        const uint32_t nb = perm[k];
        slotOf[nb] = insert(hash_key(blocks[nb].data(), bits), nb, slots, cas, amin);
        CHECK(slotOf[nb] == kNoSlot || slotOf[nb] < slots, "slot %u of %u", slotOf[nb], slots);
    }
    for (uint32_t nb = 0; nb < n; ++nb)
    {
        if (slotOf[nb] == kNoSlot) ++o.noSlot;
        const uint32_t l = candidate_leader(table.data(), slotOf[nb], nb);
        o.dupOf[nb] = (l != nb && keys_equal(blocks[nb].data(), blocks[l].data())) ? l : nb;
        if (o.dupOf[nb] != nb) ++o.dups;
    }
    return o;
}

// the properties that hold for every hash width and table size
static void check_pairs(const std::vector<Key>& blocks, const Outcome& o, const char* what)
{
    for (uint32_t nb = 0; nb < uint32_t(blocks.size()); ++nb)
    {
        const uint32_t l = o.dupOf[nb];
        CHECK(l <= nb, "%s: block %u has the later leader %u", what, nb, l);
        if (l == nb || l > nb) continue;
        CHECK(std::memcmp(blocks[nb].data(), blocks[l].data(), sizeof(Key)) == 0, "%s: block %u is not bit-equal to its leader %u", what, nb, l);
        CHECK(o.dupOf[l] == l, "%s: the leader %u of block %u is a duplicate itself", what, l, nb);
    }
}

int main(int argc, char** argv)
{
    const uint32_t n = (argc > 1) ? uint32_t(std::strtoul(argv[1], nullptr, 10)) : 4096u;
    // a pool of distinct tiles: noise, one-colour tiles (several sharing a word in all but one texel), tiles that differ from another in
    // one bit of one word; every block is a draw from the pool, so most keys come several times
    std::vector<Key> pool;
    const uint32_t poolSize = n / 3 + 1;
    while (pool.size() < poolSize)
    {
        Key k;
        const uint32_t kind = rnd() % 4;
        if (kind == 0 || pool.empty()) for (uint32_t& w : k) w = rnd();
        else if (kind == 1) { const uint32_t w0 = rnd() % 64; k.fill(w0); }
        else if (kind == 2) { const uint32_t w0 = rnd() % 64; k.fill(w0); k[rnd() % kKeyWords] ^= 1u << (rnd() % 32); }
        else { k = pool[rnd() % pool.size()]; k[rnd() % kKeyWords] ^= 1u << (rnd() % 32); }
        pool.push_back(k);
    }
    std::vector<Key> blocks(n);
    for (Key& b : blocks) b = pool[rnd() % pool.size()];

    // counts made without a hash
    std::map<Key, uint32_t> firstOf;
    for (uint32_t nb = 0; nb < n; ++nb) firstOf.emplace(blocks[nb], nb);
    const uint32_t distinct = uint32_t(firstOf.size());

    {
        const Outcome o = run(blocks, 64, kSlotsPerBlock * n);
        check_pairs(blocks, o, "full width");
        CHECK(o.noSlot == 0, "full width: %u blocks found no slot in a table of %u slots", o.noSlot, kSlotsPerBlock * n);
        CHECK(o.dups == n - distinct, "full width: %u duplicates, blocks - distinct = %u", o.dups, n - distinct);
        for (uint32_t nb = 0; nb < n; ++nb) CHECK(o.dupOf[nb] == firstOf[blocks[nb]], "full width: block %u -> %u, first equal block %u", nb, o.dupOf[nb], firstOf[blocks[nb]]);
        std::printf("full width: %u blocks, %u distinct, %u duplicates\n", n, distinct, o.dups);
    }
    for (uint32_t bits : { 0u, 2u, 5u, 9u })
    {
        const Outcome o = run(blocks, bits, kSlotsPerBlock * n);
        check_pairs(blocks, o, "forced collisions");
        // expected: per hash value the first block leads, and exactly the blocks with its key copy it
        std::map<unsigned long long, uint32_t> lead;
        for (uint32_t nb = 0; nb < n; ++nb) lead.emplace(hash_key(blocks[nb].data(), bits), nb);
        uint32_t expect = 0;
        for (uint32_t nb = 0; nb < n; ++nb)
        {
            const uint32_t l = lead[hash_key(blocks[nb].data(), bits)];
            const bool dup = l != nb && blocks[l] == blocks[nb];
            expect += dup ? 1u : 0u;
            CHECK(o.dupOf[nb] == (dup ? l : nb), "%u hash bits: block %u -> %u, expected %u", bits, nb, o.dupOf[nb], dup ? l : nb);
        }
        CHECK(o.dups == expect && o.dups <= n - distinct, "%u hash bits: %u duplicates, expected %u", bits, o.dups, expect);
        CHECK(lead.size() <= (1ull << bits), "%u hash bits: %zu hash values", bits, lead.size());
        std::printf("%u hash bits: %zu hash values, %u duplicates\n", bits, lead.size(), o.dups);
    }
    for (uint32_t slots : { 1u, 7u, kProbeBound, distinct / 2 + 1, distinct, distinct + distinct / 16 })
    {
        const Outcome o = run(blocks, 64, slots);
        check_pairs(blocks, o, "small table");
        CHECK(o.dups <= n - distinct, "table of %u slots: %u duplicates of at most %u", slots, o.dups, n - distinct);
        if (slots < distinct) CHECK(o.noSlot > 0, "table of %u slots holds %u distinct keys", slots, distinct);
        std::printf("table of %u slots for %u distinct keys: %u blocks without a slot, %u duplicates\n", slots, distinct, o.noSlot, o.dups);
    }
    std::printf("%u tiles: %d failures\n", n, g_failures);
    return g_failures ? 1 : 0;
}
