// JPEG reader and writer of the host layer (the writer begins at SaveJPEGRaw). Behaviour follows Auxiliary/DirectXTexJPEG.cpp, the reference's codec over libjpeg with its defaults
// (JDCT_ISLOW, fancy upsampling); DirectXTexAMD.h states the four departures. No library is linked: the marker walk, the Huffman decoder and
// the four passes of a progressive file are below. The yardstick is tests/jpeg_ref.py, a numpy restatement that reproduces libjpeg-turbo's
// decode byte for byte.
// The reader is split in two. LoadFromJPEGMemoryRaw does what is byte-serial - markers, tables, the Huffman walk of every scan, every
// refusal - and hands back the frame and its quantised coefficients, which a progressive file needs stored whole anyway. What happens to a
// coefficient after that is dxtex_jpeg.h's, which the GPU kernels share: the host loader runs it here one block and one texel at a time, the
// resident forms at the end of this file run it on the device, so that a file crosses PCIe as its coefficients and is never downloaded.
#include "DirectXTexAMD_Internal.h"
#include "../csrc/dxtex_jpeg.h"

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

namespace DirectXTexAMD
{
namespace
{
    inline uint32_t Be16(const uint8_t* p) noexcept { return (uint32_t(p[0]) << 8) | p[1]; }

    // A Huffman table as the decoder reads it: codes of up to kLook bits through one lookup, longer ones through the largest code of each
    // length (the walk of Annex F.2.2.3)
    constexpr uint32_t kLook = 9;
    struct HuffTable
    {
        bool present = false;
        uint16_t look[1u << kLook];          // length << 8 | symbol; 0 = the code is longer than kLook bits
        int32_t maxCode[18];                 // of each length, -1 where a length has none; [17] ends the walk
        int32_t valOffset[17];               // symbol index of a length's first code minus that code
        uint8_t symbols[256];
    };

    // counts[16] and the symbols behind them; false for a table whose codes do not fit their lengths
    bool BuildTable(const uint8_t* counts, const uint8_t* symbols, uint32_t total, HuffTable& t) noexcept
    {
        std::memset(t.look, 0, sizeof(t.look));
        std::memset(t.symbols, 0, sizeof(t.symbols));
        std::memcpy(t.symbols, symbols, total);
        uint32_t code = 0, k = 0;
        for (uint32_t len = 1; len <= 16; ++len)
        {
            t.valOffset[len] = int32_t(k) - int32_t(code);
            for (uint32_t i = 0; i < counts[len - 1]; ++i, ++code, ++k)
            {
                if (code >= (1u << len)) return false;
                if (len <= kLook)
                {
                    const uint32_t first = code << (kLook - len);
                    for (uint32_t f = 0; f < (1u << (kLook - len)); ++f) t.look[first + f] = uint16_t((len << 8) | symbols[k]);
                }
            }
            t.maxCode[len] = counts[len - 1] ? int32_t(code) - 1 : -1;
            code <<= 1;
        }
        t.maxCode[17] = 0x7FFFFFFF;
        t.present = true;
        return true;
    }

    // The bits of an entropy-coded segment, stuffing removed. Behind the segment's last byte - a marker or the end of the file - zeros are
    // fed so that the lookup always has its bits, and `real` counts the file's own: a decode that consumed a fed bit has run past the data.
    struct BitReader
    {
        const uint8_t* data; size_t size, at;
        uint64_t acc = 0; uint32_t bits = 0; int64_t real = 0;
        BitReader(const uint8_t* d, size_t n, size_t start) noexcept : data(d), size(n), at(start) {}

        void Fill() noexcept
        {
            while (bits <= 56)
            {
                uint32_t byte = 0; bool have = false;
                if (at < size)
                {
                    if (data[at] != 0xFF) { byte = data[at++]; have = true; }
                    else
                    {
                        size_t k = at + 1;
                        while (k < size && data[k] == 0xFF) ++k;
                        if (k < size && data[k] == 0) { byte = 0xFF; at = k + 1; have = true; }          // a stuffed 0xFF
                    }
                }
                acc |= uint64_t(byte) << (56 - bits);
                bits += 8;
                if (have) real += 8;
            }
        }
        uint32_t Peek(uint32_t n) noexcept { if (bits < n) Fill(); return uint32_t(acc >> (64 - n)); }
        void Drop(uint32_t n) noexcept { acc <<= n; bits -= n; real -= n; }
        uint32_t Get(uint32_t n) noexcept { if (!n) return 0; const uint32_t v = Peek(n); Drop(n); return v; }
        bool Overrun() const noexcept { return real < 0; }
        // what is left of an interval is dropped; the position moves to the marker behind it (or the end)
        void ToMarker() noexcept
        {
            acc = 0; bits = 0; real = 0;
            while (at < size)
            {
                if (data[at] != 0xFF) { ++at; continue; }
                size_t k = at + 1;
                while (k < size && data[k] == 0xFF) ++k;
                if (k >= size) { at = size; return; }
                if (data[k] == 0) { at = k + 1; continue; }
                return;
            }
        }
    };

    // -1 for a code no length of the table has
    inline int32_t Decode(BitReader& br, const HuffTable& t) noexcept
    {
        const uint32_t peek = br.Peek(16);
        const uint16_t e = t.look[peek >> (16 - kLook)];
        if (e) { br.Drop(e >> 8); return e & 0xFF; }
        uint32_t len = kLook + 1;
        while (len <= 16 && int32_t(peek >> (16 - len)) > t.maxCode[len]) ++len;
        if (len > 16) return -1;
        br.Drop(len);
        const int32_t index = int32_t(peek >> (16 - len)) + t.valOffset[len];
        return (index < 0 || index > 255) ? -1 : t.symbols[index];
    }

    inline int32_t Extend(uint32_t v, uint32_t s) noexcept { return (s && v < (1u << (s - 1))) ? int32_t(v) - int32_t(1u << s) + 1 : int32_t(v); }

    struct Component
    {
        uint32_t id = 0, h = 0, v = 0, tq = 0, blocksPerRow = 0, blockRows = 0, dw = 0, dh = 0;
        size_t offset = 0;
        int8_t bits[64];          // progressive: the Al each coefficient has reached, -1 before its first scan
        bool seen = false;
    };

    struct Decoder
    {
        const uint8_t* data = nullptr; size_t size = 0;
        uint16_t quant[4][64] = {}; bool quantPresent[4] = {};
        std::unique_ptr<HuffTable[]> dc, ac;          // four each
        bool haveFrame = false, progressive = false, jfif = false, adobe = false, scans = false;
        uint32_t adobeTransform = 0, restart = 0;
        uint32_t width = 0, height = 0, ncomp = 0, hmax = 1, vmax = 1;
        Component comp[3];
        Blob storage; int16_t* coef = nullptr; size_t coefCount = 0;
    };

    HRESULT ParseFrame(Decoder& d, const uint8_t* body, size_t n, bool progressive) noexcept
    {
        if (d.haveFrame || n < 6) return E_FAIL;
        const uint32_t precision = body[0], height = Be16(body + 1), width = Be16(body + 3), ncomp = body[5];
        if (precision == 12) return HRESULT_E_NOT_SUPPORTED;
        if (precision != 8) return E_FAIL;
        if (ncomp == 4) return E_FAIL;          // CMYK / YCCK: the reference translates them to DXGI_FORMAT_UNKNOWN and throws
        if ((ncomp != 1 && ncomp != 3) || n != 6 + 3 * size_t(ncomp)) return E_FAIL;
        if (!width) return E_FAIL;
        if (!height) return HRESULT_E_NOT_SUPPORTED;          // the height comes in a DNL segment behind the first scan
        for (uint32_t i = 0; i < ncomp; ++i)
        {
            Component& c = d.comp[i];
            c.id = body[6 + 3 * i]; c.h = body[7 + 3 * i] >> 4; c.v = body[7 + 3 * i] & 15; c.tq = body[8 + 3 * i];
            if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4 || c.tq > 3) return E_FAIL;
            for (uint32_t k = 0; k < i; ++k) if (d.comp[k].id == c.id) return E_FAIL;
        }
        if (ncomp == 1) d.comp[0].h = d.comp[0].v = 1;
        else
        {
            const Component& y = d.comp[0];
            const bool luma = (y.h == 1 && y.v == 1) || (y.h == 2 && y.v == 1) || (y.h == 2 && y.v == 2);
            if (!luma || d.comp[1].h != 1 || d.comp[1].v != 1 || d.comp[2].h != 1 || d.comp[2].v != 1) return HRESULT_E_NOT_SUPPORTED;
        }
        d.width = width; d.height = height; d.ncomp = ncomp; d.hmax = d.comp[0].h; d.vmax = d.comp[0].v; d.progressive = progressive;
        size_t at = 0;
        for (uint32_t i = 0; i < ncomp; ++i)
        {
            Component& c = d.comp[i];
            c.blocksPerRow = dxtex::jpeg_padded_blocks(width, c.h, d.hmax); c.blockRows = dxtex::jpeg_padded_blocks(height, c.v, d.vmax);
            c.dw = dxtex::jpeg_downsampled(width, c.h, d.hmax); c.dh = dxtex::jpeg_downsampled(height, c.v, d.vmax);
            c.offset = at;
            at += size_t(c.blocksPerRow) * c.blockRows * 64;
            std::memset(c.bits, -1, sizeof(c.bits));
        }
        d.coefCount = at;
        d.haveFrame = true;
        return S_OK;
    }

    struct ScanComponent { Component* c; const HuffTable* dc; const HuffTable* ac; int32_t pred; };

    // one block of a baseline scan; false for a defect
    inline bool BaselineBlock(BitReader& br, int16_t* blk, ScanComponent& sc) noexcept
    {
        int32_t s = Decode(br, *sc.dc);
        if (s < 0 || s > 15) return false;
        sc.pred = int32_t(uint32_t(sc.pred) + uint32_t(Extend(br.Get(uint32_t(s)), uint32_t(s))));
        std::memset(blk, 0, 64 * sizeof(int16_t));
        blk[0] = int16_t(uint16_t(uint32_t(sc.pred)));
        for (uint32_t k = 1; k < 64;)
        {
            const int32_t rs = Decode(br, *sc.ac);
            if (rs < 0) return false;
            const uint32_t r = uint32_t(rs) >> 4;
            s = rs & 15;
            if (s)
            {
                k += r;
                if (k > 63) return false;
                blk[dxtex::kJpegNatural[k]] = int16_t(uint16_t(uint32_t(Extend(br.Get(uint32_t(s)), uint32_t(s)))));
                ++k;
            }
            else if (r == 15)
            {
                if (k + 16 > 64) return false;
                k += 16;
            }
            else break;
        }
        return true;
    }

    inline bool AcFirst(BitReader& br, int16_t* blk, const HuffTable& ac, uint32_t ss, uint32_t se, uint32_t al, uint32_t& eobrun) noexcept
    {
        if (eobrun > 0) { --eobrun; return true; }
        for (uint32_t k = ss; k <= se;)
        {
            const int32_t rs = Decode(br, ac);
            if (rs < 0) return false;
            const uint32_t r = uint32_t(rs) >> 4, s = uint32_t(rs) & 15;
            if (s)
            {
                k += r;
                if (k > se) return false;
                blk[dxtex::kJpegNatural[k]] = int16_t(uint16_t(uint32_t(Extend(br.Get(s), s)) << al));
                ++k;
            }
            else if (r == 15)
            {
                if (k + 16 > se + 1) return false;
                k += 16;
            }
            else { eobrun = (1u << r) + br.Get(r) - 1; return true; }
        }
        return true;
    }

    inline void Correct(BitReader& br, int16_t& v, int32_t p1, int32_t m1) noexcept
    {
        if (br.Get(1) && (int32_t(v) & p1) == 0) v = int16_t(uint16_t(uint32_t(int32_t(v) + (v >= 0 ? p1 : m1))));
    }

    inline bool AcRefine(BitReader& br, int16_t* blk, const HuffTable& ac, uint32_t ss, uint32_t se, uint32_t al, uint32_t& eobrun) noexcept
    {
        const int32_t p1 = int32_t(1u << al), m1 = -p1;
        uint32_t k = ss;
        if (eobrun == 0)
        {
            while (k <= se)
            {
                const int32_t rs = Decode(br, ac);
                if (rs < 0) return false;
                int32_t r = rs >> 4;
                const uint32_t s = uint32_t(rs) & 15;
                int32_t value = 0;
                if (s)
                {
                    if (s != 1) return false;
                    value = br.Get(1) ? p1 : m1;
                }
                else if (r != 15)
                {
                    eobrun = (1u << r) + br.Get(uint32_t(r));
                    break;
                }
                while (k <= se)
                {
                    int16_t& v = blk[dxtex::kJpegNatural[k]];
                    if (v != 0) Correct(br, v, p1, m1);
                    else if (--r < 0) break;
                    ++k;
                }
                if (value)
                {
                    if (k > se) return false;
                    blk[dxtex::kJpegNatural[k]] = int16_t(value);
                }
                ++k;
            }
        }
        if (eobrun > 0)
        {
            for (; k <= se; ++k)
            {
                int16_t& v = blk[dxtex::kJpegNatural[k]];
                if (v != 0) Correct(br, v, p1, m1);
            }
            --eobrun;
        }
        return true;
    }

    // The scan whose header is `body`, its data at `at`; on success `at` is the marker behind the data (or the end of the file)
    HRESULT DecodeScan(Decoder& d, const uint8_t* body, size_t n, size_t& at) noexcept
    {
        if (n < 1) return E_FAIL;
        const uint32_t ns = body[0];
        if (ns < 1 || ns > d.ncomp || n != 4 + 2 * size_t(ns)) return E_FAIL;
        ScanComponent sc[3];
        for (uint32_t i = 0; i < ns; ++i)
        {
            const uint32_t id = body[1 + 2 * i], t = body[2 + 2 * i];
            Component* c = nullptr;
            for (uint32_t k = 0; k < d.ncomp; ++k) if (d.comp[k].id == id) c = &d.comp[k];
            if (!c || (t >> 4) > 3 || (t & 15) > 3) return E_FAIL;
            for (uint32_t k = 0; k < i; ++k) if (sc[k].c == c) return E_FAIL;
            sc[i] = ScanComponent{ c, &d.dc[t >> 4], &d.ac[t & 15], 0 };
        }
        uint32_t ss = body[1 + 2 * ns], se = body[2 + 2 * ns], ah = body[3 + 2 * ns] >> 4, al = body[3 + 2 * ns] & 15;
        if (d.progressive)
        {
            if (ss > se || se > 63 || (ss == 0 && se != 0) || (ss > 0 && ns != 1) || ah > 13 || al > 13 || (ah && al != ah - 1)) return E_FAIL;
            for (uint32_t i = 0; i < ns; ++i)
            {
                for (uint32_t k = ss; k <= se; ++k)
                {
                    const int32_t cur = sc[i].c->bits[k];
                    if (ah == 0 ? cur >= 0 : cur != int32_t(ah)) return E_FAIL;          // a scan out of its order
                }
                if (ss > 0 && sc[i].c->bits[0] < 0) return E_FAIL;                       // an AC scan in front of the DC scan
            }
        }
        else { ss = 0; se = 63; ah = 0; al = 0; }
        for (uint32_t i = 0; i < ns; ++i)
        {
            if ((!d.progressive || (ss == 0 && ah == 0)) && !sc[i].dc->present) return E_FAIL;
            if ((!d.progressive || ss > 0) && !sc[i].ac->present) return E_FAIL;
        }
        // the units the restart interval counts: MCUs of an interleaved scan, the component's own blocks otherwise
        uint32_t unitsX, unitsY;
        if (ns > 1)
        {
            uint32_t blocks = 0;
            for (uint32_t i = 0; i < ns; ++i) blocks += sc[i].c->h * sc[i].c->v;
            if (blocks > 10) return E_FAIL;
            unitsX = (d.width + 8 * d.hmax - 1) / (8 * d.hmax); unitsY = (d.height + 8 * d.vmax - 1) / (8 * d.vmax);
        }
        else { unitsX = (sc[0].c->dw + 7) / 8; unitsY = (sc[0].c->dh + 7) / 8; }
        if (!d.coef)
        {
            // every block takes at least one bit of some scan, and padding at most doubles a component's blocks: a file far too short for
            // its frame is refused before memory is asked for
            if (d.coefCount / 64 > (d.size - at) * 32 + 64) return E_FAIL;
            const HRESULT hr = d.storage.Initialize(d.coefCount * sizeof(int16_t));
            if (FAILED(hr)) return hr;
            d.coef = reinterpret_cast<int16_t*>(d.storage.GetBufferPointer());
            std::memset(d.coef, 0, d.coefCount * sizeof(int16_t));
        }
        BitReader br(d.data, d.size, at);
        uint32_t eobrun = 0, expect = 0;
        uint64_t done = 0;
        for (uint32_t uy = 0; uy < unitsY; ++uy)
            for (uint32_t ux = 0; ux < unitsX; ++ux, ++done)
            {
                if (d.restart && done && done % d.restart == 0)
                {
                    br.ToMarker();
                    size_t k = br.at;
                    if (k >= d.size) return E_FAIL;
                    while (k < d.size && d.data[k] == 0xFF) ++k;
                    if (k >= d.size || d.data[k] != 0xD0 + expect) return E_FAIL;
                    expect = (expect + 1) & 7;
                    br.at = k + 1;
                    for (uint32_t i = 0; i < ns; ++i) sc[i].pred = 0;
                    eobrun = 0;
                }
                for (uint32_t i = 0; i < ns; ++i)
                {
                    Component& c = *sc[i].c;
                    const uint32_t bw = ns > 1 ? c.h : 1, bh = ns > 1 ? c.v : 1;
                    for (uint32_t vv = 0; vv < bh; ++vv)
                        for (uint32_t hh = 0; hh < bw; ++hh)
                        {
                            int16_t* blk = d.coef + c.offset + (size_t(uy * bh + vv) * c.blocksPerRow + (ux * bw + hh)) * 64;
                            bool ok = true;
                            if (!d.progressive) ok = BaselineBlock(br, blk, sc[i]);
                            else if (ss == 0)
                            {
                                if (ah == 0)
                                {
                                    const int32_t s = Decode(br, *sc[i].dc);
                                    if (s < 0 || s > 15) ok = false;
                                    else
                                    {
                                        sc[i].pred = int32_t(uint32_t(sc[i].pred) + uint32_t(Extend(br.Get(uint32_t(s)), uint32_t(s))));
                                        blk[0] = int16_t(uint16_t(uint32_t(sc[i].pred) << al));
                                    }
                                }
                                else if (br.Get(1)) blk[0] = int16_t(uint16_t(uint32_t(blk[0]) | (1u << al)));
                            }
                            else if (ah == 0) ok = AcFirst(br, blk, *sc[i].ac, ss, se, al, eobrun);
                            else ok = AcRefine(br, blk, *sc[i].ac, ss, se, al, eobrun);
                            if (!ok || br.Overrun()) return E_FAIL;
                        }
                }
            }
        br.ToMarker();
        at = br.at;
        for (uint32_t i = 0; i < ns; ++i)
        {
            for (uint32_t k = ss; k <= se; ++k) sc[i].c->bits[k] = int8_t(al);
            sc[i].c->seen = true;
        }
        return S_OK;
    }

    // The marker walk. headerOnly stops at the first scan (GetMetadata*); otherwise every scan is decoded and the file must end in EOI.
    HRESULT Walk(Decoder& d, bool headerOnly) noexcept
    {
        const uint8_t* p = d.data; const size_t n = d.size;
        if (n < 2 || p[0] != 0xFF || p[1] != 0xD8) return E_FAIL;
        d.dc.reset(new (std::nothrow) HuffTable[4]); d.ac.reset(new (std::nothrow) HuffTable[4]);
        if (!d.dc || !d.ac) return E_OUTOFMEMORY;
        size_t at = 2;
        for (;;)
        {
            if (at >= n) return E_FAIL;          // no EOI
            if (p[at] != 0xFF)
            {
                if (!d.scans) return E_FAIL;
                ++at;          // bytes between a scan's data and the next marker are skipped
                continue;
            }
            while (at < n && p[at] == 0xFF) ++at;
            if (at >= n) return E_FAIL;
            const uint32_t m = p[at++];
            if (m == 0 && d.scans) continue;
            if (m == 0xD9) break;
            if (m == 0x01) continue;
            if (m == 0xD8 || m == 0 || (m >= 0xD0 && m <= 0xD7)) return E_FAIL;
            if (at + 2 > n) return E_FAIL;
            const size_t length = Be16(p + at);
            if (length < 2 || at + length > n) return E_FAIL;
            const uint8_t* body = p + at + 2; const size_t bodyBytes = length - 2;
            at += length;
            switch (m)
            {
            case 0xE0: if (bodyBytes >= 5 && !std::memcmp(body, "JFIF\0", 5)) d.jfif = true; break;
            case 0xEE: if (bodyBytes >= 12 && !std::memcmp(body, "Adobe", 5)) { d.adobe = true; d.adobeTransform = body[11]; } break;
            case 0xDB:
                for (size_t k = 0; k < bodyBytes;)
                {
                    const uint32_t pq = body[k] >> 4, tq = body[k] & 15;
                    ++k;
                    if (pq > 1 || tq > 3) return E_FAIL;
                    const size_t bytes = pq ? 128 : 64;
                    if (k + bytes > bodyBytes) return E_FAIL;
                    for (uint32_t i = 0; i < 64; ++i) d.quant[tq][dxtex::kJpegNatural[i]] = uint16_t(pq ? Be16(body + k + 2 * i) : body[k + i]);
                    d.quantPresent[tq] = true;
                    k += bytes;
                }
                break;
            case 0xC4:
                for (size_t k = 0; k < bodyBytes;)
                {
                    if (k + 17 > bodyBytes) return E_FAIL;
                    const uint32_t tc = body[k] >> 4, th = body[k] & 15;
                    uint32_t total = 0;
                    for (uint32_t i = 0; i < 16; ++i) total += body[k + 1 + i];
                    if (tc > 1 || th > 3 || total > 256 || k + 17 + total > bodyBytes) return E_FAIL;
                    if (!BuildTable(body + k + 1, body + k + 17, total, (tc ? d.ac : d.dc)[th])) return E_FAIL;
                    k += 17 + total;
                }
                break;
            case 0xDD:
                if (bodyBytes != 2) return E_FAIL;
                d.restart = Be16(body);
                break;
            case 0xC0: case 0xC1: case 0xC2:
            {
                const HRESULT hr = ParseFrame(d, body, bodyBytes, m == 0xC2);
                if (FAILED(hr)) return hr;
                break;
            }
            case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
                return HRESULT_E_NOT_SUPPORTED;
            case 0xDA:
            {
                if (!d.haveFrame) return E_FAIL;
                if (headerOnly) return S_OK;
                const HRESULT hr = DecodeScan(d, body, bodyBytes, at);
                if (FAILED(hr)) return hr;
                d.scans = true;
                break;
            }
            case 0xC8: case 0xDC: return E_FAIL;
            default: break;          // every other segment (APPn, COM, DAC, ...) is skipped
            }
        }
        if (!d.haveFrame || !d.scans) return E_FAIL;
        for (uint32_t i = 0; i < d.ncomp; ++i)
        {
            const Component& c = d.comp[i];
            if (!d.quantPresent[c.tq]) return E_FAIL;
            if (d.progressive)
            {
                for (uint32_t k = 0; k < 64; ++k) if (c.bits[k] != 0) return HRESULT_E_NOT_SUPPORTED;          // libjpeg would smooth these blocks
            }
            else if (!c.seen) return E_FAIL;
        }
        return S_OK;
    }

    uint32_t ColourOf(const Decoder& d) noexcept
    {
        if (d.ncomp == 1) return DXTEX_JPEG_GREY;
        if (d.jfif) return DXTEX_JPEG_YCBCR;          // libjpeg asks for the JFIF marker first: with it, an Adobe marker's transform is not looked at
        if (d.adobe) return d.adobeTransform == 0 ? DXTEX_JPEG_RGB : DXTEX_JPEG_YCBCR;
        return (d.comp[0].id == 'R' && d.comp[1].id == 'G' && d.comp[2].id == 'B') ? DXTEX_JPEG_RGB : DXTEX_JPEG_YCBCR;
    }

    void FillMetadata(const Decoder& d, JPEG_FLAGS flags, TexMetadata& m) noexcept
    {
        m = TexMetadata();
        m.width = d.width; m.height = d.height; m.depth = 1; m.arraySize = 1; m.mipLevels = 1; m.dimension = TEX_DIMENSION_TEXTURE2D;
        if (d.ncomp == 1) m.format = DXGI_FORMAT_R8_UNORM;
        else
        {
            m.format = (flags & JPEG_FLAGS_DEFAULT_LINEAR) ? DXGI_FORMAT_R8G8B8A8_UNORM : DXGI_FORMAT_R8G8B8A8_UNORM_SRGB;
            m.SetAlphaMode(TEX_ALPHA_MODE_OPAQUE);
        }
    }

    HRESULT ReadJPEGFile(const char* szFile, Blob& buf) noexcept
    {
        FILE* f = std::fopen(szFile, "rb");
        if (!f) return errno == ENOENT ? HRESULT_ERROR_FILE_NOT_FOUND : E_FAIL;
        std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
        if (n < 1) { std::fclose(f); return E_FAIL; }
        const HRESULT hr = buf.Initialize(size_t(n));
        if (FAILED(hr)) { std::fclose(f); return hr; }
        const size_t got = std::fread(buf.GetBufferPointer(), 1, buf.GetBufferSize(), f);
        std::fclose(f);
        return got == buf.GetBufferSize() ? S_OK : E_FAIL;
    }

    dxtex_jpeg_frame FrameOf(const JPEGRawImage& raw) noexcept
    {
        dxtex_jpeg_frame f = {};
        f.width = raw.width; f.height = raw.height; f.components = raw.components; f.colour = raw.colour;
        for (uint32_t c = 0; c < raw.components && c < 3; ++c)
        {
            const JPEGRawImage::Component& k = raw.component[c];
            f.component[c] = dxtex_jpeg_component{ k.h, k.v, k.quant, k.blocksPerRow, k.blockRows, 0u, uint64_t(k.offset) };
        }
        std::memcpy(f.quant, raw.quant, sizeof(f.quant));
        return f;
    }
}

void JPEGRawImage::Release() noexcept
{
    storage.Release();
    width = height = components = colour = 0;
    for (Component& c : component) c = Component();
    std::memset(quant, 0, sizeof(quant));
    coefficients = nullptr;
    coefficientCount = 0;
}

HRESULT LoadFromJPEGMemoryRaw(const void* pSource, size_t size, JPEG_FLAGS flags, TexMetadata* metadata, JPEGRawImage& raw) noexcept
{
    raw.Release();
    if (!pSource) return E_INVALIDARG;
    Decoder d;
    d.data = static_cast<const uint8_t*>(pSource); d.size = size;
    const HRESULT hr = Walk(d, false);
    if (FAILED(hr)) return hr;
    raw.width = d.width; raw.height = d.height; raw.components = d.ncomp; raw.colour = ColourOf(d);
    for (uint32_t i = 0; i < d.ncomp; ++i)
    {
        const Component& c = d.comp[i];
        JPEGRawImage::Component& o = raw.component[i];
        o.h = c.h; o.v = c.v; o.quant = c.tq; o.blocksPerRow = c.blocksPerRow; o.blockRows = c.blockRows; o.offset = c.offset;
    }
    std::memcpy(raw.quant, d.quant, sizeof(raw.quant));
    raw.storage.Swap(d.storage);
    raw.coefficients = reinterpret_cast<const int16_t*>(raw.storage.GetBufferPointer());
    raw.coefficientCount = d.coefCount;
    if (metadata) FillMetadata(d, flags, *metadata);
    return S_OK;
}

HRESULT LoadFromJPEGFileRaw(const char* szFile, JPEG_FLAGS flags, TexMetadata* metadata, JPEGRawImage& raw) noexcept
{
    raw.Release();
    return LoadFile(szFile, ReadJPEGFile, [&](const uint8_t* p, size_t n) { return LoadFromJPEGMemoryRaw(p, n, flags, metadata, raw); });
}

HRESULT GetMetadataFromJPEGMemory(const void* pSource, size_t size, JPEG_FLAGS flags, TexMetadata& metadata) noexcept
{
    if (!pSource) return E_INVALIDARG;
    Decoder d;
    d.data = static_cast<const uint8_t*>(pSource); d.size = size;
    const HRESULT hr = Walk(d, true);
    if (FAILED(hr)) return hr;
    FillMetadata(d, flags, metadata);
    return S_OK;
}

HRESULT GetMetadataFromJPEGFile(const char* szFile, JPEG_FLAGS flags, TexMetadata& metadata) noexcept
{
    return LoadFile(szFile, ReadJPEGFile, [&](const uint8_t* p, size_t n) { return GetMetadataFromJPEGMemory(p, n, flags, metadata); });
}

HRESULT LoadFromJPEGMemory(const void* pSource, size_t size, JPEG_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    TexMetadata mdata; JPEGRawImage raw;
    HRESULT hr = LoadFromJPEGMemoryRaw(pSource, size, flags, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = image.Initialize2D(mdata.format, mdata.width, mdata.height, 1, 1);
    if (FAILED(hr)) return hr;
    const Image* img = image.GetImage(0, 0, 0);
    if (!img) { image.Release(); return E_POINTER; }
    // the planes, block-padded, one component after another
    size_t planeAt[3] = {}, total = 0;
    for (uint32_t c = 0; c < raw.components; ++c) { planeAt[c] = total; total += size_t(raw.component[c].blocksPerRow) * 8 * raw.component[c].blockRows * 8; }
    Blob planes;
    hr = planes.Initialize(total);
    if (FAILED(hr)) { image.Release(); return hr; }
    dxtex::JpegPlane plane[3] = {};
    for (uint32_t c = 0; c < raw.components; ++c)
    {
        const JPEGRawImage::Component& k = raw.component[c];
        uint8_t* out = planes.GetBufferPointer() + planeAt[c];
        const uint32_t pitch = k.blocksPerRow * 8;
        for (uint32_t by = 0; by < k.blockRows; ++by)
            for (uint32_t bx = 0; bx < k.blocksPerRow; ++bx)
            {
                uint8_t samples[64];
                dxtex::jpeg_idct_block(raw.coefficients + k.offset + (size_t(by) * k.blocksPerRow + bx) * 64, raw.quant[k.quant], samples);
                for (uint32_t r = 0; r < 8; ++r) std::memcpy(out + size_t(by * 8 + r) * pitch + bx * 8, samples + r * 8, 8);
            }
        const uint32_t hmax = raw.component[0].h, vmax = raw.component[0].v;
        plane[c] = dxtex::JpegPlane{ out, pitch, dxtex::jpeg_downsampled(raw.width, k.h, hmax), dxtex::jpeg_downsampled(raw.height, k.v, vmax), hmax / k.h, vmax / k.v };
    }
    for (size_t y = 0; y < img->height; ++y)
    {
        uint8_t* d = img->pixels + y * img->rowPitch;
        if (raw.components == 1) std::memcpy(d, plane[0].samples + y * plane[0].pitch, img->width);
        else
            for (size_t x = 0; x < img->width; ++x)
                dxtex::le_store32(d + 4 * x, dxtex::jpeg_texel(int(raw.colour), dxtex::jpeg_upsample(plane[0], uint32_t(x), uint32_t(y)), dxtex::jpeg_upsample(plane[1], uint32_t(x), uint32_t(y)),
                                                                dxtex::jpeg_upsample(plane[2], uint32_t(x), uint32_t(y))), 4);
    }
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromJPEGFile(const char* szFile, JPEG_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadJPEGFile, [&](const uint8_t* p, size_t n) { return LoadFromJPEGMemory(p, n, flags, metadata, image); });
}

// ---- resident forms: the coefficients travel as the file has them, everything behind them runs on the device (dxtex_jpeg_decode_device) ----
HRESULT UploadJPEGRaw(Device& device, const TexMetadata& metadata, const JPEGRawImage& raw, DeviceScratchImage& image) noexcept
{
    image.Release();
    if (!device) return E_POINTER;
    if (!raw.coefficients || !raw.coefficientCount || metadata.arraySize != 1 || metadata.mipLevels != 1 || metadata.depth != 1) return E_INVALIDARG;
    if (metadata.width != raw.width || metadata.height != raw.height) return E_INVALIDARG;
    return InitializeAndFill(device, metadata, image, [&](const Image& img)
    {
        // the coefficients start an allocation of their own: every block is one aligned 128-byte read
        const size_t bytes = raw.coefficientCount * sizeof(int16_t);
        return UploadAndUnpack(device, raw.coefficients, bytes, [&](void* p)
        {
            const dxtex_jpeg_frame f = FrameOf(raw);
            const dxtex_image d = ImageOf(img);
            return dxtex_jpeg_decode_device(device.Get(), p, bytes, &f, &d);
        });
    });
}

HRESULT LoadFromJPEGMemory(Device& device, const void* pSource, size_t size, JPEG_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    TexMetadata mdata; JPEGRawImage raw;
    HRESULT hr = LoadFromJPEGMemoryRaw(pSource, size, flags, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = UploadJPEGRaw(device, mdata, raw, image);
    if (FAILED(hr)) return hr;
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromJPEGFile(Device& device, const char* szFile, JPEG_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadJPEGFile, [&](const uint8_t* p, size_t n) { return LoadFromJPEGMemory(device, p, n, flags, metadata, image); });
}

// ---- the writer. The same split run backwards: SaveJPEGRaw is the byte-serial half - markers, tables, baseline Huffman coding of a frame's
// quantised coefficients - and what makes the coefficients is dxtex_jpeg.h's, run here serially by the host forms and on the device
// (dxtex_jpeg_encode_device) by the resident ones. The files are the reference's, which leaves libjpeg at jpeg_set_defaults and quality 100:
// JFIF 1.01, quantiser tables of ones, the standard Huffman tables of Annex K.3 to K.6, grey as one 1 x 1 component, colour as 4:2:0 YCbCr
// in one interleaved scan; tests/golden/jpeg_write holds libjpeg-turbo's own bytes. ------------------------------------------------------------
namespace
{
    // Annex K.3 - K.6: the codes of each length and the symbols in code order; [0] luminance, [1] chrominance
    const uint8_t kDcCounts[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
    const uint8_t kDcSymbols[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
    const uint8_t kAcCounts[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125 }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119 } };
    const uint8_t kAcSymbols[2][162] = {
        { 0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1,
          0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
          0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A,
          0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
          0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
          0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA },
        { 0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1,
          0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
          0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
          0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
          0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
          0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA } };

    // a table as the coder reads it: the code and its length of every symbol (length 0: the table has no such symbol)
    struct CodeTable { uint16_t code[256]; uint8_t length[256]; };
    void BuildCodes(const uint8_t* counts, const uint8_t* symbols, CodeTable& t) noexcept
    {
        std::memset(&t, 0, sizeof(t));
        uint32_t code = 0, k = 0;
        for (uint32_t len = 1; len <= 16; ++len, code <<= 1)
            for (uint32_t i = 0; i < counts[len - 1]; ++i, ++code, ++k) { t.code[symbols[k]] = uint16_t(code); t.length[symbols[k]] = uint8_t(len); }
    }

    // The file as it grows: bytes on the heap, and the entropy coder's bits with their 0xFF stuffing. A failed allocation is remembered and
    // everything after it dropped; the caller asks once at the end.
    struct Writer
    {
        uint8_t* data = nullptr; size_t size = 0, capacity = 0; bool failed = false;
        uint64_t acc = 0; uint32_t bits = 0;
        ~Writer() { std::free(data); }
        bool Reserve(size_t more) noexcept
        {
            if (failed) return false;
            if (size + more <= capacity) return true;
            const size_t want = (capacity * 2 > size + more ? capacity * 2 : size + more) + 4096;
            uint8_t* grown = static_cast<uint8_t*>(std::realloc(data, want));
            if (!grown) { failed = true; return false; }
            data = grown; capacity = want;
            return true;
        }
        void Byte(uint32_t b) noexcept { if (Reserve(1)) data[size++] = uint8_t(b); }
        void Word(uint32_t w) noexcept { Byte(w >> 8); Byte(w & 0xFFu); }
        void Bytes(const uint8_t* p, size_t n) noexcept { if (Reserve(n)) { std::memcpy(data + size, p, n); size += n; } }
        void Marker(uint32_t m, size_t bodyBytes) noexcept { Byte(0xFF); Byte(m); Word(uint32_t(bodyBytes + 2)); }
        // n <= 16 bits, the value's low n
        void Put(uint32_t value, uint32_t n) noexcept
        {
            acc = (acc << n) | (value & ((1u << n) - 1u)); bits += n;
            if (bits < 8) return;
            if (!Reserve(2 * (bits / 8))) { bits &= 7u; return; }
            while (bits >= 8)
            {
                const uint8_t b = uint8_t(acc >> (bits - 8));
                data[size++] = b;
                if (b == 0xFF) data[size++] = 0;
                bits -= 8;
            }
        }
        void Flush() noexcept { if (bits) Put(0x7Fu, 8u - bits); }          // the last byte is padded with 1-bits
    };

    inline uint32_t BitsOf(uint32_t magnitude) noexcept { uint32_t n = 0; while (magnitude) { ++n; magnitude >>= 1; } return n; }

    // encode_one_block of jchuff.c: false where a DC difference needs more than 11 bits or an AC value more than 10 (JERR_BAD_DCT_COEF)
    bool EncodeBlock(Writer& w, const int16_t* block, int32_t& predictor, const CodeTable& dc, const CodeTable& ac) noexcept
    {
        const int32_t diff = int32_t(block[0]) - predictor;
        predictor = block[0];
        uint32_t n = BitsOf(uint32_t(diff < 0 ? -diff : diff));
        if (n > 11) return false;
        w.Put(dc.code[n], dc.length[n]);
        if (n) w.Put(uint32_t(diff < 0 ? diff - 1 : diff), n);
        uint32_t run = 0;
        for (uint32_t k = 1; k < 64; ++k)
        {
            const int32_t v = block[dxtex::kJpegNatural[k]];
            if (!v) { ++run; continue; }
            for (; run > 15; run -= 16) w.Put(ac.code[0xF0], ac.length[0xF0]);
            n = BitsOf(uint32_t(v < 0 ? -v : v));
            if (n > 10) return false;
            w.Put(ac.code[(run << 4) | n], ac.length[(run << 4) | n]);
            w.Put(uint32_t(v < 0 ? v - 1 : v), n);
            run = 0;
        }
        if (run) w.Put(ac.code[0], ac.length[0]);
        return true;
    }

    // the frame of an image as the reference writes it: quality 100, grey 1 x 1, colour 2 x 2 luma over 1 x 1 chroma
    HRESULT FrameFor(const Image& image, dxtex_jpeg_frame& f) noexcept
    {
        if (!image.pixels) return E_POINTER;
        const int texel = dxtex::jpeg_texel_of(int(image.format));          // the coder's table
        if (texel < 0) return HRESULT_E_NOT_SUPPORTED;
        const bool grey = texel == dxtex::JPEG_TEXEL_GREY;
        if (!image.width || !image.height || image.width > 65535 || image.height > 65535) return E_INVALIDARG;          // SOF0 holds 16 bits
        f = dxtex_jpeg_frame();
        f.width = uint32_t(image.width); f.height = uint32_t(image.height);
        f.components = grey ? 1u : 3u; f.colour = grey ? DXTEX_JPEG_GREY : DXTEX_JPEG_YCBCR;
        const uint32_t hmax = grey ? 1u : 2u, vmax = hmax;
        uint64_t at = 0;
        for (uint32_t c = 0; c < f.components; ++c)
        {
            dxtex_jpeg_component& k = f.component[c];
            k.h = c ? 1u : hmax; k.v = c ? 1u : vmax; k.quant = c ? 1u : 0u;
            k.blocksPerRow = dxtex::jpeg_padded_blocks(f.width, k.h, hmax); k.blockRows = dxtex::jpeg_padded_blocks(f.height, k.v, vmax);
            k.offset = at;
            at += uint64_t(k.blocksPerRow) * k.blockRows * 64u;
        }
        for (uint32_t t = 0; t < 2; ++t) for (uint32_t k = 0; k < 64; ++k) f.quant[t][k] = 1;
        return S_OK;
    }

    // `raw` takes the frame and `coefficientCount` coefficients of storage of its own
    HRESULT RawFor(const dxtex_jpeg_frame& f, JPEGRawImage& raw) noexcept
    {
        raw.Release();
        size_t count = 0;
        for (uint32_t c = 0; c < f.components; ++c) count += size_t(f.component[c].blocksPerRow) * f.component[c].blockRows * 64u;
        const HRESULT hr = raw.storage.Initialize(count * sizeof(int16_t));
        if (FAILED(hr)) return hr;
        raw.width = f.width; raw.height = f.height; raw.components = f.components; raw.colour = f.colour;
        for (uint32_t c = 0; c < f.components; ++c)
        {
            const dxtex_jpeg_component& k = f.component[c];
            JPEGRawImage::Component& o = raw.component[c];
            o.h = k.h; o.v = k.v; o.quant = k.quant; o.blocksPerRow = k.blocksPerRow; o.blockRows = k.blockRows; o.offset = size_t(k.offset);
        }
        std::memcpy(raw.quant, f.quant, sizeof(raw.quant));
        raw.coefficients = reinterpret_cast<const int16_t*>(raw.storage.GetBufferPointer());
        raw.coefficientCount = count;
        return S_OK;
    }
}

HRESULT SaveJPEGRaw(const JPEGRawImage& raw, Blob& blob) noexcept
{
    blob.Release();
    if (!raw.coefficients || !raw.width || !raw.height || raw.width > 65535u || raw.height > 65535u) return E_INVALIDARG;
    if (raw.components != (raw.colour == DXTEX_JPEG_GREY ? 1u : 3u) || raw.colour > DXTEX_JPEG_YCBCR) return raw.colour == DXTEX_JPEG_RGB ? HRESULT_E_NOT_SUPPORTED : E_INVALIDARG;
    const uint32_t hmax = raw.component[0].h, vmax = raw.component[0].v;
    size_t count = 0;
    bool wide = false;          // a table with an entry above 255 is written with 16-bit entries, and the frame as SOF1: baseline has none
    for (uint32_t c = 0; c < raw.components; ++c)
    {
        const JPEGRawImage::Component& k = raw.component[c];
        if (k.quant > 3u || k.h < 1u || k.h > 4u || k.v < 1u || k.v > 4u || k.h > hmax || k.v > vmax || hmax % k.h || vmax % k.v) return E_INVALIDARG;
        if (k.blocksPerRow != dxtex::jpeg_padded_blocks(raw.width, k.h, hmax) || k.blockRows != dxtex::jpeg_padded_blocks(raw.height, k.v, vmax) || k.offset != count) return E_INVALIDARG;
        count += size_t(k.blocksPerRow) * k.blockRows * 64u;
        for (uint32_t i = 0; i < 64; ++i) { if (!raw.quant[k.quant][i]) return E_INVALIDARG; wide = wide || raw.quant[k.quant][i] > 255u; }
    }
    if (raw.coefficientCount < count) return E_INVALIDARG;

    Writer w;
    w.Byte(0xFF); w.Byte(0xD8);
    static const uint8_t jfif[14] = { 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 };
    w.Marker(0xE0, sizeof(jfif)); w.Bytes(jfif, sizeof(jfif));
    bool sent[4] = {};
    for (uint32_t c = 0; c < raw.components; ++c)
    {
        const uint32_t t = raw.component[c].quant;
        if (sent[t]) continue;
        sent[t] = true;
        bool wideTable = false;
        for (uint32_t i = 0; i < 64; ++i) wideTable = wideTable || raw.quant[t][i] > 255u;
        w.Marker(0xDB, wideTable ? 129 : 65); w.Byte((wideTable ? 0x10u : 0u) | t);
        for (uint32_t i = 0; i < 64; ++i) { const uint32_t q = raw.quant[t][dxtex::kJpegNatural[i]]; if (wideTable) w.Word(q); else w.Byte(q); }
    }
    w.Marker(wide ? 0xC1 : 0xC0, 6 + 3 * raw.components);
    w.Byte(8); w.Word(raw.height); w.Word(raw.width); w.Byte(raw.components);
    for (uint32_t c = 0; c < raw.components; ++c) { w.Byte(c + 1); w.Byte((raw.component[c].h << 4) | raw.component[c].v); w.Byte(raw.component[c].quant); }
    // luma codes with tables 0, chroma with tables 1
    std::unique_ptr<CodeTable[]> codes(new (std::nothrow) CodeTable[4]);
    if (!codes) return E_OUTOFMEMORY;
    for (uint32_t t = 0; t < (raw.components == 1 ? 1u : 2u); ++t)
    {
        w.Marker(0xC4, 17 + 12); w.Byte(t); w.Bytes(kDcCounts[t], 16); w.Bytes(kDcSymbols, 12);
        w.Marker(0xC4, 17 + 162); w.Byte(0x10u | t); w.Bytes(kAcCounts[t], 16); w.Bytes(kAcSymbols[t], 162);
        BuildCodes(kDcCounts[t], kDcSymbols, codes[2 * t]);
        BuildCodes(kAcCounts[t], kAcSymbols[t], codes[2 * t + 1]);
    }
    w.Marker(0xDA, 4 + 2 * raw.components); w.Byte(raw.components);
    for (uint32_t c = 0; c < raw.components; ++c) { w.Byte(c + 1); w.Byte(c ? 0x11 : 0x00); }
    w.Byte(0); w.Byte(63); w.Byte(0);
    // one scan: a grey frame's blocks in raster order, a colour frame's MCU by MCU, each component's h x v blocks in raster order
    int32_t predictor[3] = {};
    const uint32_t mcusAcross = raw.component[0].blocksPerRow / hmax, mcusDown = raw.component[0].blockRows / vmax;
    for (uint32_t my = 0; my < mcusDown; ++my)
        for (uint32_t mx = 0; mx < mcusAcross; ++mx)
            for (uint32_t c = 0; c < raw.components; ++c)
            {
                const JPEGRawImage::Component& k = raw.component[c];
                for (uint32_t v = 0; v < k.v; ++v)
                    for (uint32_t h = 0; h < k.h; ++h)
                    {
                        const int16_t* block = raw.coefficients + k.offset + (size_t(my * k.v + v) * k.blocksPerRow + (mx * k.h + h)) * 64u;
                        if (!EncodeBlock(w, block, predictor[c], codes[c ? 2 : 0], codes[c ? 3 : 1])) return E_FAIL;
                    }
            }
    w.Flush();
    w.Byte(0xFF); w.Byte(0xD9);
    if (w.failed) return E_OUTOFMEMORY;
    const HRESULT hr = blob.Initialize(w.size);
    if (FAILED(hr)) return hr;
    std::memcpy(blob.GetBufferPointer(), w.data, w.size);
    return S_OK;
}

HRESULT SaveToJPEGMemory(const Image& image, JPEG_FLAGS, Blob& blob) noexcept
{
    blob.Release();          // on any failure the result is empty
    dxtex_jpeg_frame f;
    HRESULT hr = FrameFor(image, f);
    if (FAILED(hr)) return hr;
    const size_t texel = f.components == 1 ? 1u : 4u;
    if (image.rowPitch < image.width * texel) return E_INVALIDARG;
    JPEGRawImage raw;
    hr = RawFor(f, raw);
    if (FAILED(hr)) return hr;
    const bool bgr = dxtex::jpeg_texel_of(int(image.format)) == dxtex::JPEG_TEXEL_BGRX;
    const dxtex::JpegSource source = { image.pixels, image.rowPitch, f.width, f.height, f.components == 1, bgr };
    int16_t* coefficients = reinterpret_cast<int16_t*>(raw.storage.GetBufferPointer());
    const uint32_t hmax = f.component[0].h, vmax = f.component[0].v;
    for (uint32_t c = 0; c < f.components; ++c)
    {
        const dxtex_jpeg_component& k = f.component[c];
        const uint32_t rw = dxtex::jpeg_real_blocks(f.width, k.h, hmax), rh = dxtex::jpeg_real_blocks(f.height, k.v, vmax);
        for (uint32_t by = 0; by < k.blockRows; ++by)
            for (uint32_t bx = 0; bx < k.blocksPerRow; ++bx)
            {
                uint32_t sx = bx, sy = by;
                const bool dummy = dxtex::jpeg_dummy_block(bx, by, rw, rh, k.h, sx, sy);
                uint8_t samples[64];
                for (uint32_t y = 0; y < 8; ++y)
                    for (uint32_t x = 0; x < 8; ++x) samples[y * 8 + x] = uint8_t(dxtex::jpeg_plane_sample(source, c, hmax / k.h, vmax / k.v, sx * 8 + x, sy * 8 + y));
                int16_t* out = coefficients + k.offset + (size_t(by) * k.blocksPerRow + bx) * 64u;
                dxtex::jpeg_fdct_block(samples, 8, f.quant[k.quant], out);
                if (dummy) std::memset(out + 1, 0, 63 * sizeof(int16_t));
            }
    }
    return SaveJPEGRaw(raw, blob);
}

HRESULT SaveToJPEGFile(const Image& image, JPEG_FLAGS flags, const char* szFile) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveToJPEGMemory(image, flags, blob); });
}

// ---- resident forms: both kernels run on the device image, the coefficients come down once - 2 bytes a texel for grey, 3 for colour - and
// nothing goes up ------------------------------------------------------------------------------------------------------------------------------
HRESULT SaveToJPEGMemory(Device& device, const Image& deviceImage, JPEG_FLAGS, Blob& blob) noexcept
{
    blob.Release();
    dxtex_jpeg_frame f;
    HRESULT hr = FrameFor(deviceImage, f);
    if (FAILED(hr)) return hr;
    if (!device) return E_POINTER;
    JPEGRawImage raw;
    hr = RawFor(f, raw);
    if (FAILED(hr)) return hr;
    const size_t bytes = raw.coefficientCount * sizeof(int16_t);
    const dxtex_image s = ImageOf(deviceImage);
    hr = PackAndDownload(device, bytes, raw.storage.GetBufferPointer(), [&](void* p) { return dxtex_jpeg_encode_device(device.Get(), &s, &f, p, bytes); });
    return FAILED(hr) ? hr : SaveJPEGRaw(raw, blob);
}

HRESULT SaveToJPEGFile(Device& device, const Image& deviceImage, JPEG_FLAGS flags, const char* szFile) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveToJPEGMemory(device, deviceImage, flags, blob); });
}
} // namespace DirectXTexAMD
