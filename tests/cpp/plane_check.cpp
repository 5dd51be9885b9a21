// Host build of dxtex_plane.h for tests/test_single_plane_cpu.py: ConvertToSinglePlane's checks, and what single_plane_kernel writes, by
// visiting every (job, lane, unit) its launch geometry visits and calling the per-lane function the kernel calls.
//
//   plane_check CASES IN OUT
//
// CASES is text. "batch N" is followed by N case lines, which run as ONE submission (checked first, all of them; then cut into launches
// of kPlaneBatchMax jobs as launch_single_plane cuts them). A case line is
//   format width height rowPitch slicePitch srcShift  dstFormat dstWidth dstHeight dstRowPitch dstBytes dstShift  flags
// IN holds, per case in order, slicePitch source bytes and then dstBytes bytes the destination starts with. Each image lives in an
// allocation of its own that ENDS with the image's last byte (so that a sanitizer build sees any access past slicePitch or past the
// destination) and starts `shift` bytes (0..15) after a 16-byte boundary. flags: 1 = null source pixels, 2 = null destination pixels,
// 4 = the destination is the source's memory. OUT receives, per case, the int32 HRESULT of its check, the resolved job's groups (0: the element
// route), elems and units as three uint32 (0 where the check failed), and the dstBytes destination bytes.
#include "dxtex_plane.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dxtex;

namespace
{
struct Case
{
    PlaneImage s, d;
    uint64_t dstBytes;
    unsigned srcShift, dstShift, flags;
    uint8_t* srcMem = nullptr;
    uint8_t* dstMem = nullptr;
    int32_t hr = 0;
    PlaneJob job = {};
};

void run_batch(std::vector<Case*>& batch)
{
    for (Case* c : batch) if ((c->hr = plane_check(c->s, c->d, &c->job)) != kPlaneOk) return;
    for (size_t first = 0; first < batch.size(); first += kPlaneBatchMax)
    {
        PlaneBatch b;
        b.count = uint32_t(batch.size() - first < kPlaneBatchMax ? batch.size() - first : kPlaneBatchMax);
        for (uint32_t k = 0; k < kPlaneBatchMax; ++k) b.job[k] = k < b.count ? batch[first + k]->job : PlaneJob{};
        uint32_t gx = 0, gy = 0;
        plane_grid(b, gx, gy);
        for (uint32_t z = 0; z < b.count; ++z)
            for (uint32_t by = 0; by < gy; ++by)
                for (uint32_t bx = 0; bx < gx; ++bx)
                    for (uint32_t t = 0; t < kPlaneThreads; ++t)
                    {
                        const PlaneJob& j = b.job[z];
                        const uint32_t lane = bx * kPlaneThreads + t;
                        if (lane >= plane_lanes(j)) continue;
                        for (uint32_t unit = by; unit < j.units; unit += gy) plane_lane(j, lane, unit);
                    }
    }
}
}

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: plane_check CASES IN OUT\n"); return 2; }
    FILE* cases = fopen(argv[1], "r");
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!cases || !in || !out) { fprintf(stderr, "plane_check: cannot open a file\n"); return 2; }
    unsigned n = 0;
    while (fscanf(cases, " batch %u", &n) == 1)
    {
        std::vector<Case> store(n);
        std::vector<Case*> batch;
        for (Case& c : store)
        {
            unsigned long long v[12];
            if (fscanf(cases, "%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %u", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8],
                       &v[9], &v[10], &v[11], &c.flags) != 13) { fprintf(stderr, "plane_check: bad case line\n"); return 2; }
            c.s = PlaneImage{ v[1], v[2], int(v[0]), v[3], v[4], 0 };
            c.d = PlaneImage{ v[7], v[8], int(v[6]), v[9], 0, 0 };
            c.srcShift = unsigned(v[5]) & 15u; c.dstBytes = v[10]; c.dstShift = unsigned(v[11]) & 15u;
            // malloc returns 16-byte aligned memory; the image starts `shift` bytes in and ends with the allocation
            const size_t srcTotal = size_t(c.srcShift + c.s.slicePitch), dstTotal = size_t(c.dstShift + c.dstBytes);
            c.srcMem = static_cast<uint8_t*>(malloc(srcTotal ? srcTotal : 1u));
            c.dstMem = static_cast<uint8_t*>(malloc(dstTotal ? dstTotal : 1u));
            if (!c.srcMem || !c.dstMem) { fprintf(stderr, "plane_check: out of memory\n"); return 2; }
            if (fread(c.srcMem + c.srcShift, 1, size_t(c.s.slicePitch), in) != c.s.slicePitch ||
                fread(c.dstMem + c.dstShift, 1, size_t(c.dstBytes), in) != c.dstBytes) { fprintf(stderr, "plane_check: short input\n"); return 2; }
            c.s.pixels = (c.flags & 1u) ? 0 : uint64_t(reinterpret_cast<uintptr_t>(c.srcMem + c.srcShift));
            c.d.pixels = (c.flags & 2u) ? 0 : (c.flags & 4u) ? c.s.pixels : uint64_t(reinterpret_cast<uintptr_t>(c.dstMem + c.dstShift));
            batch.push_back(&c);
        }
        run_batch(batch);
        // a failed check fails the submission: the cases before it report 0 and, like it, keep their destinations as they were
        for (Case& c : store)
        {
            fwrite(&c.hr, sizeof c.hr, 1, out);
            const uint32_t route[3] = { c.hr == kPlaneOk ? c.job.groups : 0u, c.hr == kPlaneOk ? c.job.elems : 0u, c.hr == kPlaneOk ? c.job.units : 0u };
            fwrite(route, sizeof route, 1, out);
            fwrite(c.dstMem + c.dstShift, 1, size_t(c.dstBytes), out);
            free(c.srcMem); free(c.dstMem);
        }
    }
    fclose(cases); fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
