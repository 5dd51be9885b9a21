// The inflater of the host layer's codecs (DirectXTexAMD_PNG.cpp: IDAT; DirectXTexAMD_EXR.cpp: ZIP and ZIPS chunks): a zlib stream (RFC 1950 /
// 1951) into a buffer whose size the caller knows, and Adler-32. No library is linked. Not part of the public interface. Header-only, and
// every definition has internal linkage, as in DirectXTexAMD_Internal.h: a translation unit compiled on its own, as the sanitised test
// programs compile one codec each, calls its own copy.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>

namespace DirectXTexAMD
{
namespace
{
    uint32_t Adler32(const uint8_t* p, size_t n) noexcept
    {
        uint32_t a = 1, b = 0;
        while (n)
        {
            const size_t k = std::min<size_t>(n, 5552);          // the most steps before b can pass 2^32
            for (size_t i = 0; i < k; ++i) { a += p[i]; b += a; }
            a %= 65521u; b %= 65521u;
            p += k; n -= k;
        }
        return (b << 16) | a;
    }

    // ---- inflate (RFC 1950 / 1951): stored, fixed and dynamic blocks into one contiguous buffer, which is also the window -------------------
    // A canonical Huffman code: codes of up to kFast bits through a table, longer ones counted down bit by bit. The rules for a set of
    // lengths are zlib's: over-subscribed is an error, incomplete is an error unless the set is empty or its longest code is one bit.
    constexpr int kFast = 10;
    struct Huffman
    {
        uint16_t fast[1 << kFast];          // symbol << 4 | length; 0: not a code of up to kFast bits
        uint16_t count[16];
        uint16_t symbol[288];
        bool Build(const uint8_t* lengths, int n, bool codeLengthCode) noexcept
        {
            std::memset(count, 0, sizeof(count));
            std::memset(fast, 0, sizeof(fast));
            for (int i = 0; i < n; ++i) ++count[lengths[i]];
            count[0] = 0;
            int left = 1, max = 0;
            for (int len = 1; len <= 15; ++len)
            {
                left <<= 1; left -= count[len];
                if (left < 0) return false;
                if (count[len]) max = len;
            }
            if (max && left > 0 && (codeLengthCode || max != 1)) return false;
            uint16_t offs[16]; offs[1] = 0;
            for (int len = 1; len < 15; ++len) offs[len + 1] = uint16_t(offs[len] + count[len]);
            for (int i = 0; i < n; ++i) if (lengths[i]) symbol[offs[lengths[i]]++] = uint16_t(i);
            // the table: the code of every symbol of up to kFast bits, bit-reversed (the stream holds codes first bit first), at every index
            // whose low bits are that code
            uint32_t code = 0; int index = 0;
            for (int len = 1; len <= kFast; ++len)
            {
                for (int k = 0; k < count[len]; ++k, ++code, ++index)
                {
                    uint32_t rev = 0;
                    for (int b = 0; b < len; ++b) rev |= ((code >> b) & 1u) << (len - 1 - b);
                    for (uint32_t j = rev; j < (1u << kFast); j += 1u << len) fast[j] = uint16_t((symbol[index] << 4) | len);
                }
                code <<= 1;
            }
            return true;
        }
    };

    struct BitReader
    {
        const uint8_t* p; const uint8_t* end;
        uint64_t buf = 0; int cnt = 0;
        void Fill() noexcept { while (cnt <= 56 && p < end) { buf |= uint64_t(*p++) << cnt; cnt += 8; } }
        // n <= 16 bits; false when the stream holds fewer
        bool Bits(int n, uint32_t& v) noexcept
        {
            if (cnt < n) { Fill(); if (cnt < n) return false; }
            v = uint32_t(buf & ((uint64_t(1) << n) - 1)); buf >>= n; cnt -= n;
            return true;
        }
        // one symbol; -1 for a code that is not in the set or a stream that ends inside one
        int Decode(const Huffman& h) noexcept
        {
            if (cnt < 15) Fill();
            const uint16_t e = h.fast[buf & ((1u << kFast) - 1)];
            if (e)
            {
                const int len = e & 15;
                if (len > cnt) return -1;
                buf >>= len; cnt -= len;
                return e >> 4;
            }
            int code = 0, first = 0, index = 0;
            for (int len = 1; len <= 15; ++len)
            {
                if (cnt < len) return -1;
                code |= int((buf >> (len - 1)) & 1u);
                const int c = h.count[len];
                if (code - c < first) { buf >>= len; cnt -= len; return h.symbol[index + (code - first)]; }
                index += c; first += c; first <<= 1; code <<= 1;
            }
            return -1;
        }
    };

    constexpr uint16_t kLenBase[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
    constexpr uint8_t kLenExtra[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
    constexpr uint16_t kDistBase[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
    constexpr uint8_t kDistExtra[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };

    // The zlib stream at [z, z + zn) into out[0, cap). True when cap bytes came out: either the stream ended there and its Adler-32 holds,
    // or it goes on - the surplus is not decoded. False for every defect, a stream that ends short of cap included.
    bool Inflate(const uint8_t* z, size_t zn, uint8_t* out, size_t cap) noexcept
    {
        if (zn < 2) return false;
        if ((z[0] & 0x0F) != 8 || (z[0] >> 4) > 7 || ((uint32_t(z[0]) << 8) | z[1]) % 31u != 0 || (z[1] & 0x20)) return false;          // deflate, a window of up to 32 KiB, no dictionary
        BitReader br{ z + 2, z + zn };
        size_t pos = 0;
        std::unique_ptr<Huffman> lit(new (std::nothrow) Huffman), dist(new (std::nothrow) Huffman);
        if (!lit || !dist) return false;
        for (;;)
        {
            uint32_t last, type;
            if (!br.Bits(1, last) || !br.Bits(2, type)) return false;
            if (type == 0)
            {
                br.buf >>= br.cnt & 7; br.cnt &= ~7;          // to the next byte
                uint32_t len, nlen;
                if (!br.Bits(16, len) || !br.Bits(16, nlen)) return false;
                if ((len ^ 0xFFFFu) != nlen) return false;
                const bool surplus = len > cap - pos;
                if (surplus) len = uint32_t(cap - pos);
                // whole bytes: first what the bit buffer holds, then the rest from the stream
                while (len && br.cnt) { out[pos++] = uint8_t(br.buf); br.buf >>= 8; br.cnt -= 8; --len; }
                if (size_t(br.end - br.p) < len) return false;
                if (len) std::memcpy(out + pos, br.p, len);
                br.p += len; pos += len;
                if (surplus) return true;
            }
            else if (type == 1 || type == 2)
            {
                uint8_t lengths[320];
                if (type == 1)
                {
                    for (int i = 0; i < 288; ++i) lengths[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
                    lit->Build(lengths, 288, false);
                    for (int i = 0; i < 32; ++i) lengths[i] = 5;
                    dist->Build(lengths, 32, false);          // symbols 30 and 31 complete the code; a stream that uses one is refused below
                }
                else
                {
                    uint32_t nlen, ndist, ncode;
                    if (!br.Bits(5, nlen) || !br.Bits(5, ndist) || !br.Bits(4, ncode)) return false;
                    nlen += 257; ndist += 1; ncode += 4;
                    if (nlen > 286 || ndist > 30) return false;
                    static constexpr uint8_t order[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };
                    uint8_t cl[19] = {};
                    for (uint32_t i = 0; i < ncode; ++i) { uint32_t v; if (!br.Bits(3, v)) return false; cl[order[i]] = uint8_t(v); }
                    if (!lit->Build(cl, 19, true)) return false;          // lit serves as the code length code first
                    uint32_t i = 0;
                    while (i < nlen + ndist)
                    {
                        const int sym = br.Decode(*lit);
                        if (sym < 0) return false;
                        if (sym < 16) { lengths[i++] = uint8_t(sym); continue; }
                        uint32_t rep, prev = 0;
                        if (sym == 16)
                        {
                            if (i == 0) return false;
                            prev = lengths[i - 1];
                            if (!br.Bits(2, rep)) return false;
                            rep += 3;
                        }
                        else if (sym == 17) { if (!br.Bits(3, rep)) return false; rep += 3; }
                        else { if (!br.Bits(7, rep)) return false; rep += 11; }
                        if (i + rep > nlen + ndist) return false;
                        while (rep--) lengths[i++] = uint8_t(prev);
                    }
                    if (lengths[256] == 0) return false;          // no end-of-block code
                    if (!lit->Build(lengths, int(nlen), false) || !dist->Build(lengths + nlen, int(ndist), false)) return false;
                }
                for (;;)
                {
                    const int sym = br.Decode(*lit);
                    if (sym < 0) return false;
                    if (sym < 256)
                    {
                        if (pos == cap) return true;          // surplus
                        out[pos++] = uint8_t(sym);
                        continue;
                    }
                    if (sym == 256) break;
                    if (sym > 285) return false;
                    uint32_t extra;
                    if (!br.Bits(kLenExtra[sym - 257], extra)) return false;
                    size_t len = kLenBase[sym - 257] + extra;
                    const int ds = br.Decode(*dist);
                    if (ds < 0 || ds > 29) return false;
                    if (!br.Bits(kDistExtra[ds], extra)) return false;
                    const size_t d = kDistBase[ds] + extra;
                    if (d > pos) return false;          // before the start
                    const bool surplus = len > cap - pos;
                    if (surplus) len = cap - pos;
                    // byte by byte where the copy overlaps itself (a run), in one piece otherwise
                    if (d >= len) std::memcpy(out + pos, out + pos - d, len);
                    else for (size_t k = 0; k < len; ++k) out[pos + k] = out[pos + k - d];
                    pos += len;
                    if (surplus) return true;
                }
            }
            else return false;
            if (last) break;
        }
        if (pos != cap) return false;
        // the check value sits behind the last block, from the next byte on
        br.buf >>= br.cnt & 7; br.cnt &= ~7;
        uint32_t hi, lo;
        if (!br.Bits(16, hi) || !br.Bits(16, lo)) return false;
        const uint32_t stored = (((hi & 0xFFu) << 8 | (hi >> 8)) << 16) | ((lo & 0xFFu) << 8 | (lo >> 8));
        return stored == Adler32(out, cap);
    }
}
} // namespace DirectXTexAMD
