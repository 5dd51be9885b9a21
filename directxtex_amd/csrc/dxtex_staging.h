// The traffic of one host-pointer C ABI call through the context's two staging buffers, as plain data: which parts of the input and the
// output staging the call needs, which of the caller's bytes go up before its kernels and which come down after them. capi.cpp's run_plan
// executes a plan; nothing here touches a device, so tests/cpp/staging_check.cpp builds the same plans on the host.
//   - a part is a run of bytes of one buffer; parts get consecutive 256-byte aligned offsets, and a part may be reserved without being
//     uploaded (an output, or a mip level the kernels fill);
//   - a copy moves `rows` rows of `rowBytes` between host memory (hostPitch apart) and a part (from `offset`, devPitch apart); a flat copy is
//     one row. A download may read either buffer: a chain that works in place comes down from the input staging;
//   - every size is added up with overflow checks, and a copy has to lie inside its part: a plan that fails either is not ok() and moves nothing.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace dxtex
{
enum StageBuf : uint8_t { STAGE_IN = 0, STAGE_OUT = 1 };

struct StagePart { StageBuf buf; size_t at, bytes; };        // `bytes` bytes at offset `at` of the buffer

struct StageCopy
{
    void* host; size_t hostPitch;                            // (an upload only reads it)
    StagePart part; size_t offset, devPitch;
    size_t rowBytes, rows;
    size_t at() const { return part.at + offset; }           // where the device side starts in its buffer
};

// false where the sum or product does not fit a size_t
inline bool stage_add(size_t a, size_t b, size_t* r) { *r = a + b; return *r >= a; }
inline bool stage_mul(size_t a, size_t b, size_t* r) { *r = a * b; return !a || *r / a == b; }
// the bytes from the first of `rows` rows `pitch` apart to the end of the last
inline bool stage_span(size_t pitch, size_t rowBytes, size_t rows, size_t* r)
{
    if (!rows || !rowBytes) { *r = 0; return true; }
    return stage_mul(pitch, rows - 1, r) && stage_add(*r, rowBytes, r);
}

class StagingPlan
{
public:
    // the next part of a buffer: rows * rowBytes bytes (a product that overflows is as fatal as a sum that does)
    StagePart reserve(StageBuf buf, size_t rowBytes, size_t rows = 1)
    {
        size_t bytes, padded;
        if (!stage_mul(rowBytes, rows, &bytes)) { ok_ = false; bytes = 0; }
        const StagePart p = { buf, total_[buf], bytes };
        if (!stage_add(bytes, 255, &padded) || !stage_add(total_[buf], padded & ~size_t(255), &total_[buf])) ok_ = false;
        return p;
    }
    StagePart in(size_t rowBytes, size_t rows = 1) { return reserve(STAGE_IN, rowBytes, rows); }
    StagePart out(size_t rowBytes, size_t rows = 1) { return reserve(STAGE_OUT, rowBytes, rows); }

    void upload(const void* host, size_t hostPitch, const StagePart& part, size_t offset, size_t devPitch, size_t rowBytes, size_t rows)
    {
        if (part.buf != STAGE_IN) ok_ = false;
        add(up_, { const_cast<void*>(host), hostPitch, part, offset, devPitch, rowBytes, rows }, &moved_[0]);
    }
    void download(void* host, size_t hostPitch, const StagePart& part, size_t offset, size_t devPitch, size_t rowBytes, size_t rows)
    {
        add(down_, { host, hostPitch, part, offset, devPitch, rowBytes, rows }, &moved_[1]);
    }
    // flat: `bytes` from the start of the part
    void upload(const void* host, const StagePart& part, size_t bytes) { upload(host, bytes, part, 0, bytes, bytes, 1); }
    void download(void* host, const StagePart& part, size_t bytes) { download(host, bytes, part, 0, bytes, bytes, 1); }

    bool ok() const { return ok_; }
    size_t need(StageBuf buf) const { return total_[buf]; }      // bytes the buffer has to hold
    size_t up_bytes() const { return moved_[0]; }
    size_t down_bytes() const { return moved_[1]; }
    const std::vector<StageCopy>& uploads() const { return up_; }
    const std::vector<StageCopy>& downloads() const { return down_; }

private:
    void add(std::vector<StageCopy>& list, const StageCopy& c, size_t* moved)
    {
        size_t span, end, bytes;
        if (!stage_span(c.devPitch, c.rowBytes, c.rows, &span) || !stage_add(c.offset, span, &end) || end > c.part.bytes ||
            !stage_span(c.hostPitch, c.rowBytes, c.rows, &span) ||        // (the host side's end must be an address too)
            !stage_mul(c.rowBytes, c.rows, &bytes) || !stage_add(*moved, bytes, moved))
        {
            ok_ = false;
            return;
        }
        if (bytes) list.push_back(c);
    }

    std::vector<StageCopy> up_, down_;
    size_t total_[2] = { 0, 0 }, moved_[2] = { 0, 0 };
    bool ok_ = true;
};
} // namespace dxtex
