// The staging plans of the host-pointer C ABI calls (directxtex_amd/csrc/dxtex_staging.h) on the host: every traffic shape capi.cpp builds
// is built here at small sizes - width 1 and 5, padded and tight pitches, a row longer than the pitch, 1 and 6 images, an image of no rows
// in the middle of a DDS batch - and checked:
//   - parts start on 256 bytes, lie behind one another and inside the bytes the plan asks the buffer to hold;
//   - every copy names a reserved part and lies inside it; the up and down totals are the closed forms the GPU tests assert;
//   - the plan then runs on host memory the way run_plan runs it (two vectors of exactly need() bytes for the staging, the caller's
//     images in vectors of exactly their size), rows longer than a pitch one by one, so a copy that leaves either side is an
//     AddressSanitizer report;
//   - sizes that do not fit a size_t, and a copy that leaves its part, make the plan not ok() instead of wrapping.
// A stand-alone program (plain C++, no device): the Makefile builds it with AddressSanitizer and UndefinedBehaviorSanitizer.
#include "dxtex_staging.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace dxtex;
typedef std::vector<uint8_t> Bytes;

static int g_failures = 0;
#define CHECK(COND, ...) do { if (!(COND)) { if (++g_failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static size_t align16(size_t n) { return (n + 15) & ~size_t(15); }
static size_t span(size_t pitch, size_t rowBytes, size_t rows) { return rows && rowBytes ? (rows - 1) * pitch + rowBytes : 0; }

// a plan and the parts it reserved, in order
struct Built
{
    StagingPlan plan;
    std::vector<StagePart> parts;
    StagePart in(size_t bytes) { parts.push_back(plan.in(bytes)); return parts.back(); }
    StagePart out(size_t bytes) { parts.push_back(plan.out(bytes)); return parts.back(); }
};

static bool same_part(const StagePart& a, const StagePart& b) { return a.buf == b.buf && a.at == b.at && a.bytes == b.bytes; }

static void verify(const char* what, const Built& b, size_t up, size_t down)
{
    CHECK(b.plan.ok(), "%s: plan refused", what);
    size_t end[2] = { 0, 0 };
    for (const StagePart& p : b.parts)
    {
        CHECK(p.at % 256 == 0, "%s: part at %zu", what, p.at);
        CHECK(p.at >= end[p.buf], "%s: part at %zu starts inside the one before it (ends %zu)", what, p.at, end[p.buf]);
        end[p.buf] = p.at + p.bytes;
        CHECK(end[p.buf] <= b.plan.need(p.buf), "%s: part ends at %zu, buffer holds %zu", what, end[p.buf], b.plan.need(p.buf));
    }
    for (int dir = 0; dir < 2; ++dir)
        for (const StageCopy& c : dir ? b.plan.downloads() : b.plan.uploads())
        {
            bool known = false;
            for (const StagePart& p : b.parts) known = known || same_part(p, c.part);
            CHECK(known, "%s: a copy names a part the plan did not reserve", what);
            CHECK(dir || c.part.buf == STAGE_IN, "%s: an upload into the output staging", what);
            const size_t last = c.offset + span(c.devPitch, c.rowBytes, c.rows);
            CHECK(last <= c.part.bytes, "%s: a copy ends at %zu of a part of %zu bytes", what, last, c.part.bytes);
            CHECK(c.at() + span(c.devPitch, c.rowBytes, c.rows) <= b.plan.need(c.part.buf), "%s: a copy leaves the buffer", what);
        }
    CHECK(b.plan.up_bytes() == up, "%s: %zu bytes up, expected %zu", what, b.plan.up_bytes(), up);
    CHECK(b.plan.down_bytes() == down, "%s: %zu bytes down, expected %zu", what, b.plan.down_bytes(), down);
}

// run_plan's copies with memcpy: rows longer than a pitch travel one by one, in order
static void copy_rows(uint8_t* dst, size_t dstPitch, const uint8_t* src, size_t srcPitch, size_t rowBytes, size_t rows)
{
    for (size_t y = 0; y < rows; ++y) std::memmove(dst + y * dstPitch, src + y * srcPitch, rowBytes);
}
// uploads, then `kernel(in, out)`, then downloads, on staging of exactly the bytes the plan asks for
template<class Kernel>
static void run(const StagingPlan& plan, Kernel&& kernel)
{
    Bytes in(plan.need(STAGE_IN), 0xEE), out(plan.need(STAGE_OUT), 0xEE);
    uint8_t* base[2] = { in.data(), out.data() };
    for (const StageCopy& c : plan.uploads()) copy_rows(base[STAGE_IN] + c.at(), c.devPitch, static_cast<const uint8_t*>(c.host), c.hostPitch, c.rowBytes, c.rows);
    kernel(base[STAGE_IN], base[STAGE_OUT]);
    for (const StageCopy& c : plan.downloads()) copy_rows(static_cast<uint8_t*>(c.host), c.hostPitch, base[c.part.buf] + c.at(), c.devPitch, c.rowBytes, c.rows);
}
static void no_kernel(uint8_t*, uint8_t*) {}

static Bytes counting(size_t n, uint8_t first = 0) { Bytes b(n); for (size_t i = 0; i < n; ++i) b[i] = uint8_t(first + i * 7); return b; }

// run_staged / run_host_twin: one flat run up, one down
static void flat(size_t inBytes, size_t outBytes)
{
    Built b; Bytes src = counting(inBytes), dst(outBytes, 0);
    b.plan.upload(src.data(), b.in(inBytes), inBytes);
    b.plan.download(dst.data(), b.out(outBytes), outBytes);
    verify("flat", b, inBytes, outBytes);
    run(b.plan, [&](uint8_t* in, uint8_t* out) { CHECK(!inBytes || !std::memcmp(in, src.data(), inBytes), "flat: upload"); std::memset(out, 0x5A, outBytes); });
    for (uint8_t v : dst) CHECK(v == 0x5A, "flat: download");
}

// run_staged_rows: the file side flat, tight rows rounded to 16 down through the caller's pitch; the padding keeps its bytes
static void staged_rows(size_t need, size_t rowBytes, size_t rows, size_t hostPitch)
{
    Built b; Bytes src = counting(need), dst(hostPitch * rows, 0xA5);
    const size_t pitch = align16(rowBytes);
    b.plan.upload(src.data(), b.in(need), need);
    b.plan.download(dst.data(), hostPitch, b.out(pitch * rows), 0, pitch, rowBytes, rows);
    verify("staged rows", b, need, rowBytes * rows);
    run(b.plan, [&](uint8_t*, uint8_t* out) { std::memset(out, 0x11, pitch * rows); });
    for (size_t i = 0; i < dst.size(); ++i) CHECK(dst[i] == (i % hostPitch < rowBytes ? 0x11 : 0xA5), "staged rows: byte %zu", i);
}

// dxtex_generate_mips / _mips3d: every level a part of the input staging, level 0 up, the others down from where the kernels filled them
static void chain(size_t width, size_t height, size_t depth, size_t pad, size_t nlevels)
{
    Built b; std::vector<Bytes> level(nlevels); std::vector<StagePart> part(nlevels);
    size_t up = 0, down = 0, w = width, h = height, d = depth;
    for (size_t i = 0; i < nlevels; ++i)
    {
        const size_t bytes = (w * 4 + pad) * h * d;       // rowPitch * height, or slicePitch * depth
        level[i] = counting(bytes, uint8_t(i));
        part[i] = b.in(bytes);
        (i ? down : up) += bytes;
        w = w > 1 ? w / 2 : 1; h = h > 1 ? h / 2 : 1; d = d > 1 ? d / 2 : 1;
    }
    b.plan.upload(level[0].data(), part[0], part[0].bytes);
    for (size_t i = 1; i < nlevels; ++i) b.plan.download(level[i].data(), part[i], part[i].bytes);
    verify("mip chain", b, up, down);
    CHECK(b.plan.need(STAGE_OUT) == 0, "mip chain: output staging");
    run(b.plan, [&](uint8_t* in, uint8_t*) { for (size_t i = 1; i < nlevels; ++i) std::memset(in + part[i].at, int(0x40 + i), part[i].bytes); });
    for (size_t i = 1; i < nlevels; ++i) for (uint8_t v : level[i]) CHECK(v == 0x40 + i, "mip chain: level %zu", i);
}

// dxtex_scale_mips_alpha_for_coverage: two arenas, whole levels both ways
static void coverage(size_t width, size_t height, size_t nlevels)
{
    Built b; std::vector<Bytes> src(nlevels), dst(nlevels);
    size_t up = 0, down = 0, w = width, h = height;
    for (size_t i = 0; i < nlevels; ++i, w = w > 1 ? w / 2 : 1, h = h > 1 ? h / 2 : 1)
    {
        src[i] = counting((w * 4 + 4) * h); dst[i].assign(w * 4 * h, 0);
        const StagePart ps = b.in(src[i].size()), pd = b.out(dst[i].size());
        b.plan.upload(src[i].data(), ps, ps.bytes);
        b.plan.download(dst[i].data(), pd, pd.bytes);
        up += ps.bytes; down += pd.bytes;
    }
    verify("coverage", b, up, down);
    run(b.plan, no_kernel);
}

// the DDS pairs: unpack = payload flat up, each image's rows a part at the image's pitch, texels down; pack24 = the reverse, the file
// side's rows coming down from inside one part
struct DdsJob { size_t width, rows, pitch, fileOffset, filePitch; };
static void dds(const std::vector<DdsJob>& jobs, size_t fileBytes, size_t imageTexel, size_t fileTexel, bool unpack)
{
    Built b; Bytes file = counting(fileBytes); std::vector<Bytes> image(jobs.size());
    size_t imageSide = 0, fileSide = 0;
    StagePart fp = unpack ? b.in(fileBytes) : b.out(fileBytes);
    if (unpack) b.plan.upload(file.data(), fp, fileBytes);
    for (size_t i = 0; i < jobs.size(); ++i)
    {
        const DdsJob& j = jobs[i];
        const size_t rowBytes = j.width * imageTexel;
        image[i].assign(span(j.pitch, rowBytes, j.rows), 0xA5);
        const StagePart p = unpack ? b.out(image[i].size()) : b.in(image[i].size());
        if (unpack) b.plan.download(image[i].data(), j.pitch, p, 0, j.pitch, rowBytes, j.rows);
        else
        {
            b.plan.upload(image[i].data(), j.pitch, p, 0, j.pitch, rowBytes, j.rows);
            b.plan.download(file.data() + j.fileOffset, j.filePitch, fp, j.fileOffset, j.filePitch, j.width * fileTexel, j.rows);
        }
        imageSide += rowBytes * j.rows; fileSide += j.width * fileTexel * j.rows;
    }
    verify(unpack ? "dds unpack" : "dds pack24", b, unpack ? fileBytes : imageSide, unpack ? imageSide : fileSide);
    run(b.plan, no_kernel);
}

// dxtex_exr_unpack: the stream flat up, the items behind one another in ONE part (rows rounded to 16, no alignment between items)
static void exr(size_t width, size_t height, size_t count, size_t hostPad)
{
    Built b; Bytes stream = counting(width * height * 8 * count); std::vector<Bytes> item(count);
    const size_t rowBytes = width * 8, pitch = align16(rowBytes), itemBytes = pitch * height;
    b.plan.upload(stream.data(), b.in(stream.size()), stream.size());
    const StagePart rows = b.out(itemBytes * count);
    for (size_t i = 0; i < count; ++i)
    {
        item[i].assign((rowBytes + hostPad) * height, 0xA5);
        b.plan.download(item[i].data(), rowBytes + hostPad, rows, i * itemBytes, pitch, rowBytes, height);
    }
    verify("exr unpack", b, stream.size(), rowBytes * height * count);
    run(b.plan, [&](uint8_t*, uint8_t* out) { for (size_t i = 0; i < count; ++i) std::memset(out + i * itemBytes, int(i + 1), itemBytes); });
    for (size_t i = 0; i < count; ++i)
        for (size_t k = 0; k < item[i].size(); ++k) CHECK(item[i][k] == (k % (rowBytes + hostPad) < rowBytes ? i + 1 : 0xA5), "exr unpack: item %zu byte %zu", i, k);
}

// dxtex_analyze (down == false): n images up, nothing down; dxtex_difference / dxtex_merge_image: two up, dst's texel rows down through its pitch
static void inputs(size_t n, size_t width, size_t height, size_t pad, bool down)
{
    Built b; std::vector<Bytes> image(n); Bytes dst((width * 4 + pad) * height, 0xA5);
    size_t up = 0;
    for (size_t i = 0; i < n; ++i)
    {
        image[i] = counting((width * (i ? 16 : 4) + pad) * height);
        b.plan.upload(image[i].data(), b.in(image[i].size()), image[i].size());
        up += image[i].size();
    }
    if (down) b.plan.download(dst.data(), width * 4 + pad, b.out(dst.size()), 0, width * 4 + pad, width * 4, height);
    verify("inputs", b, up, down ? width * 4 * height : 0);
    run(b.plan, [&](uint8_t*, uint8_t* out) { if (down) std::memset(out, 0x22, dst.size()); });
    for (size_t k = 0; down && k < dst.size(); ++k) CHECK(dst[k] == (k % (width * 4 + pad) < width * 4 ? 0x22 : 0xA5), "inputs: byte %zu", k);
}

// dxtex_copy_rectangle: the rectangle's rows into a tight image and back; a host pitch shorter than the row (the packed formats) moves the
// rows one by one and the later row wins
static void rectangle(size_t rowBytes, size_t rows, size_t srcPitch, size_t dstPitch)
{
    Built b; Bytes src = counting(span(srcPitch, rowBytes, rows)), dst(span(dstPitch, rowBytes, rows), 0xA5);
    b.plan.upload(src.data(), srcPitch, b.in(rowBytes * rows), 0, rowBytes, rowBytes, rows);
    b.plan.download(dst.data(), dstPitch, b.out(rowBytes * rows), 0, rowBytes, rowBytes, rows);
    verify("rectangle", b, rowBytes * rows, rowBytes * rows);
    run(b.plan, [&](uint8_t* in, uint8_t* out) { std::memcpy(out, in, rowBytes * rows); });
    // what row-by-row memcpy between the two host images gives
    Bytes want(dst.size(), 0xA5);
    for (size_t y = 0; y < rows; ++y) std::memcpy(want.data() + y * dstPitch, src.data() + y * srcPitch, rowBytes);
    CHECK(dst == want, "rectangle %zu x %zu, pitches %zu -> %zu", rowBytes, rows, srcPitch, dstPitch);
}

// dxtex_convert_to_single_plane: the source flat up; `whole` rows down in one copy, then `cutBytes` of each of the rows after them
static void single_plane(size_t srcBytes, size_t rowBytes, size_t rows, size_t whole, size_t cutBytes, size_t hostPitch)
{
    Built b; Bytes src = counting(srcBytes), dst(hostPitch * rows, 0xA5);
    const size_t pitch = align16(rowBytes);
    b.plan.upload(src.data(), b.in(srcBytes), srcBytes);
    const StagePart staged = b.out(pitch * rows);
    b.plan.download(dst.data(), hostPitch, staged, 0, pitch, rowBytes, whole);
    for (size_t y = whole; y < rows; ++y) b.plan.download(dst.data() + y * hostPitch, hostPitch, staged, y * pitch, pitch, cutBytes, 1);
    verify("single plane", b, srcBytes, rowBytes * whole + cutBytes * (rows - whole));
    run(b.plan, [&](uint8_t*, uint8_t* out) { std::memset(out, 0x33, pitch * rows); });
    for (size_t k = 0; k < dst.size(); ++k) CHECK(dst[k] == (k % hostPitch < (k / hostPitch < whole ? rowBytes : cutBytes) ? 0x33 : 0xA5), "single plane: byte %zu", k);
}

static void refusals()
{
    uint8_t byte = 0;
    { StagingPlan p; p.in(SIZE_MAX - 100); CHECK(!p.ok(), "a part whose padding overflows"); }
    { StagingPlan p; p.in(SIZE_MAX / 2); p.in(SIZE_MAX / 2); p.in(4096); CHECK(!p.ok(), "parts whose sum overflows"); }
    { StagingPlan p; p.out(SIZE_MAX / 2 + 1, 2); CHECK(!p.ok(), "rows x pitch that overflows"); }
    { StagingPlan p; const StagePart a = p.in(SIZE_MAX / 4); p.upload(&byte, SIZE_MAX / 2, a, 0, 1, 1, 8); CHECK(!p.ok(), "a host span that overflows"); }
    { StagingPlan p; const StagePart a = p.in(64); p.upload(&byte, 16, a, 0, SIZE_MAX / 2, 16, 4); CHECK(!p.ok(), "a device span that overflows"); }
    { StagingPlan p; const StagePart a = p.in(64); p.upload(&byte, a, 65); CHECK(!p.ok(), "a copy past the end of its part"); }
    { StagingPlan p; const StagePart a = p.out(64); p.download(&byte, 16, a, 49, 16, 16, 1); CHECK(!p.ok(), "a copy from an offset past the end of its part"); }
    { StagingPlan p; const StagePart a = p.out(64); p.upload(&byte, a, 1); CHECK(!p.ok(), "an upload into the output staging"); }
    { StagingPlan p; const StagePart a = p.in(0); p.upload(&byte, a, 0); p.download(&byte, 0, a, 0, 0, 0, 5); CHECK(p.ok() && p.uploads().empty() && p.downloads().empty(), "copies of no bytes"); }
}

int main()
{
    flat(1, 1); flat(5 * 4 * 3, 8); flat(3108, 240);
    for (size_t w : { size_t(1), size_t(5) })
    {
        staged_rows(w * 3 * 4, w * 4, 4, w * 4); staged_rows(w * 3 * 4, w * 4, 4, w * 4 + 12);
        chain(w, 3, 1, 0, 2); chain(w, 5, 1, 12, 3); chain(w, 5, 3, 12, 3);
        coverage(w, 5, 3);
        for (size_t count : { size_t(1), size_t(6) }) { exr(w, 3, count, 0); exr(w, 3, count, 8); }
        inputs(1, w, 3, 0, false); inputs(6, w, 3, 4, false); inputs(2, w, 3, 0, true); inputs(2, w, 3, 8, true);
        rectangle(w * 4, 2, w * 4 + 8, w * 4); rectangle(w * 4, 3, w * 4, w * 4 + 4);
        single_plane(w * 6 + 5, w * 4, 4, 4, 0, w * 4 + 4); single_plane(w * 6 + 5, w * 4, 4, 2, w * 4 - 4, w * 4);
        // one image; six with an image of no rows in the middle; pitches padded on both sides
        dds({ { w, 3, w * 4, 0, w * 3 } }, w * 9, 4, 3, true);
        dds({ { w, 3, w * 4 + 4, 0, w * 3 } }, w * 9, 4, 3, false);
        std::vector<DdsJob> six;
        size_t at = 0;
        for (size_t i = 0; i < 6; ++i) { const size_t rows = i == 3 ? 0 : 6 - i; six.push_back({ rows ? w : 0, rows, rows ? w * 4 + 4 : 0, rows ? at : 0, rows ? w * 3 + 2 : 0 }); at += rows * (w * 3 + 2); }
        dds(six, at, 4, 3, true); dds(six, at, 4, 3, false);
    }
    // a row of 8 bytes over host pitches of 4: the packed formats' overlapping rows
    rectangle(8, 3, 4, 8); rectangle(8, 3, 8, 4); rectangle(8, 1, 4, 4);
    refusals();
    std::printf("staging plans: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
