// The search pipeline's primitives (search_common.h) at kernel level: wave_prefix_min, selection_pass, the counting sort of tasks by
// subset size (bc7_bin_count_kernel / bc7_bin_scan_kernel / bc7_bin_scatter_kernel) and queue_take. One translation unit that includes
// the header, so the kernels under test are the header's own (anonymous namespace: this unit's copy, compiled from the same text as the
// encoders'). Everything is integer and exact. The serial references below are written from the rules of the contract, not from the
// kernels: the running minimum, "for i < n, for j > i: swap if e[i] > e[j]", a stable counting sort by size, largest first.
//
//   search_prims_gpu_test              every group on device 0; one line per group: group NAME cases N failed M first-bad ...
//   search_prims_gpu_test reference    no device, no HIP call: the serial references against properties that do not depend on them
//
// After every launch the program synchronises and checks the HIP error; on the first error it names the group and exits without
// launching anything more. Exit status 0 only if every M is 0.
#include "search_common.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

using namespace dxtex;

namespace
{
const char* g_group = "start";

#define HIP_OK(call)                                                                                                          \
    do {                                                                                                                      \
        const hipError_t e_ = (call);                                                                                         \
        if (e_ != hipSuccess)                                                                                                 \
        {                                                                                                                     \
            std::printf("group %s hip error %s at %s:%d\n", g_group, hipGetErrorString(e_), __FILE__, __LINE__);             \
            std::fflush(stdout);                                                                                              \
            std::_Exit(2);                                                                                                    \
        }                                                                                                                     \
    } while (0)

void after_launch()
{
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipGetLastError());
}

struct Rng
{
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull) {}
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    uint32_t below(uint32_t n) { return uint32_t(next() % n); }
    int key31() { return int(next() & 0x7FFFFFFFu); }
};

struct Group
{
    std::string name;
    uint64_t cases = 0, failed = 0;
    std::string firstBad = "none";
    explicit Group(const char* n) : name(n) { g_group = n; }
    void result(bool ok, const std::string& what)
    {
        ++cases;
        if (!ok && !failed++) firstBad = what;
    }
    bool report() const
    {
        std::printf("group %s cases %llu failed %llu first-bad %s\n", name.c_str(), (unsigned long long)cases, (unsigned long long)failed, firstBad.c_str());
        std::fflush(stdout);
        return failed == 0;
    }
};

template<class T> struct DeviceBuf
{
    T* p = nullptr;
    size_t n = 0;
    explicit DeviceBuf(size_t count) : n(count) { HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T))); }
    ~DeviceBuf() { (void)hipFree(p); }
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    void up(const std::vector<T>& h) { if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
    void down(std::vector<T>& h) const { h.resize(n); if (n) HIP_OK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost)); }
    void fill(int byte) { HIP_OK(hipMemset(p, byte, std::max<size_t>(n, 1) * sizeof(T))); }
};

// ---- the serial references --------------------------------------------------------------------------------------------------------------
void serial_prefix_min(const int* in, int* out)
{
    int run = in[0];
    for (int l = 0; l < 64; ++l) { run = std::min(run, in[l]); out[l] = run; }
}

// "bubble up the first n items": for i < n, for j in i+1 .. 63, if e[i] > e[j] swap the keys and swap the shapes
void serial_selection(int* e, uint32_t* s, int n)
{
    for (int i = 0; i < n && i < 64; ++i)
        for (int j = i + 1; j < 64; ++j)
            if (e[i] > e[j]) { std::swap(e[i], e[j]); std::swap(s[i], s[j]); }
}

// stable counting sort of the live tasks (size = tinfo >> 24, 0 = dead) by size, largest first; returns the number of live tasks
uint32_t serial_sort(const std::vector<uint32_t>& tinfo, std::vector<uint2>& order, uint32_t hist[17], uint32_t end[17])
{
    for (int b = 0; b < 17; ++b) hist[b] = end[b] = 0;
    for (uint32_t ti : tinfo) if (ti >> 24) ++hist[ti >> 24];
    uint32_t cursor[17] = {}, run = 0;
    for (int b = 16; b >= 1; --b) { cursor[b] = run; run += hist[b]; end[b] = run; }
    order.assign(run, make_uint2(0, 0));
    for (uint32_t t = 0; t < uint32_t(tinfo.size()); ++t)
        if (tinfo[t] >> 24) order[cursor[tinfo[t] >> 24]++] = make_uint2(t, tinfo[t]);
    return run;
}

// ---- case generators --------------------------------------------------------------------------------------------------------------------
constexpr int kSelFamilies = 9;
const int kSelN[4] = { 4, 8, 16, 64 };
const char* const kSelFamilyName[kSelFamilies] = { "distinct", "ties012", "all-equal", "ascending", "descending", "pad16", "pad32", "inf-among-pads", "float-bits" };

void selection_keys(int family, uint32_t rep, Rng& rng, int* e)
{
    switch (family)
    {
    case 0:         // random distinct: the low six bits are a permutation of the lanes
    {
        int perm[64];
        for (int l = 0; l < 64; ++l) perm[l] = l;
        for (int l = 63; l > 0; --l) std::swap(perm[l], perm[rng.below(uint32_t(l) + 1)]);
        for (int l = 0; l < 64; ++l) e[l] = (rng.key31() & ~63) | perm[l];
        break;
    }
    case 1: for (int l = 0; l < 64; ++l) e[l] = int(rng.below(3)); break;
    case 2:
    {
        const int c = rep == 0 ? 0 : rep == 1 ? 0x7FFFFFFF : rng.key31();
        for (int l = 0; l < 64; ++l) e[l] = c;
        break;
    }
    case 3: case 4:
    {
        int v = int(rng.below(1000));
        const int step = (rep & 1) ? 1 : 1 + int(rng.below(1 << 24));          // rep odd: consecutive keys
        for (int l = 0; l < 64; ++l) { e[family == 3 ? l : 63 - l] = v; v += step; }
        break;
    }
    case 5: case 6:         // real keys in the first lanes, +inf pads behind them: BC7 mode 0 (16 shapes) and BC6H (32 shapes)
    {
        const int real = family == 5 ? 16 : 32;
        for (int l = 0; l < 64; ++l) e[l] = l < real ? ((rep & 1) ? int(rng.below(4)) : rng.key31()) : 0x7FFFFFFF;
        break;
    }
    case 7:                 // real keys that are themselves 0x7FFFFFFF, next to the pads
    {
        const int real = (rep & 1) ? 16 : 32;
        for (int l = 0; l < 64; ++l) e[l] = (l < real && rng.below(3) != 0) ? ((rep & 2) ? int(rng.below(3)) : rng.key31()) : 0x7FFFFFFF;
        break;
    }
    default:                // bit patterns of non-negative floats, +infinity (0x7F800000) among them, pads behind 32 lanes on odd reps
        for (int l = 0; l < 64; ++l)
        {
            const uint32_t r = rng.below(8);
            int v;
            if (r == 0) v = 0x7F800000;
            else if (r == 1) v = 0;
            else if (r == 2) v = int(rng.below(1 << 23));                                  // denormals
            else v = int((rng.below(255) << 23) | rng.below(1 << 23));                      // finite
            e[l] = ((rep & 1) && l >= 32) ? 0x7FFFFFFF : v;
        }
        break;
    }
}

constexpr int kSortFamilies = 9;
const char* const kSortFamilyName[kSortFamilies] = { "uniform", "all-dead", "one-bin-1", "one-bin-8", "one-bin-16", "bins-1-and-16", "one-live-first", "one-live-last", "runs-of-300" };
const uint32_t kSortSizes[7] = { 1u, 255u, 256u, 257u, 524288u, 524289u, 1572869u };

void sort_tinfo(int family, uint32_t ntasks, Rng& rng, std::vector<uint32_t>& tinfo)
{
    tinfo.resize(ntasks);
    uint32_t runSize = 0;
    for (uint32_t t = 0; t < ntasks; ++t)
    {
        uint32_t np;
        switch (family)
        {
        case 0: np = rng.below(17); break;
        case 1: np = 0; break;
        case 2: np = 1; break;
        case 3: np = 8; break;
        case 4: np = 16; break;
        case 5: np = rng.below(2) ? 16 : 1; break;
        case 6: np = t == 0 ? 1 + rng.below(16) : 0; break;
        case 7: np = t == ntasks - 1 ? 1 + rng.below(16) : 0; break;
        default: if (t % 300 == 0) runSize = rng.below(17); np = runSize; break;
        }
        tinfo[t] = (np << 24) | uint32_t(rng.next() & 0xFFFFFFu);
    }
}

// ---- wrapper kernels --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) prefix_min_wrap(const int* in, int* out)
{
    const uint32_t at = blockIdx.x * 64u + threadIdx.x;
    out[at] = wave_prefix_min(in[at]);
}

// four cases per workgroup, a wavefront each, as the encoders' rough passes run it
__global__ void __launch_bounds__(256) selection_wrap(const int* eIn, const int* nOf, uint32_t ncases, int* eOut, uint32_t* sOut)
{
    const int lane = int(threadIdx.x & 63u);
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (c >= ncases) return;            // wave-uniform
    int e = eIn[c * 64u + lane];
    uint32_t s = uint32_t(lane);
    const int n = nOf[c];
    for (int i = 0; i < n; ++i) selection_pass(e, s, lane, i);
    eOut[c * 64u + lane] = e;
    sOut[c * 64u + lane] = s;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}

// Persistent wavefronts pulling from one head, as the search kernels do. The idle mask changes every turn (a hash of wave and turn) and
// always has one bit set. errs[0]: indices >= live handed out, errs[1]: waves that reached the cap on turns, errs[2]: indices handed to
// lanes that were not idle.
__global__ void __launch_bounds__(64) queue_wrap(uint32_t* head, uint32_t live, uint32_t* seen, uint32_t* errs, uint32_t cap, uint32_t salt)
{
    const int lane = int(threadIdx.x);
    WaveQueue q; q.lo = q.hi = 0; q.drained = false;
    for (uint32_t turn = 0;; ++turn)
    {
        if (q.drained && q.lo >= q.hi) break;
        if (turn >= cap) { if (lane == 0) atomicAdd(&errs[1], 1u); break; }
        unsigned long long idle = mix64((static_cast<unsigned long long>(blockIdx.x) << 32) ^ turn ^ (static_cast<unsigned long long>(salt) << 20));
        if (turn % 5u == 0u) idle = ~0ull;                          // all lanes idle: the kernels' first turn
        if (turn % 7u == 3u) idle &= idle >> 17;                    // few lanes idle
        idle |= 1ull << ((turn + blockIdx.x) & 63u);
        const uint32_t idx = queue_take(q, head, live, idle, lane);
        if (idx != 0xFFFFFFFFu)
        {
            if (!((idle >> lane) & 1ull)) atomicAdd(&errs[2], 1u);
            if (idx < live) atomicAdd(&seen[idx], 1u); else atomicAdd(&errs[0], 1u);
        }
    }
}

// ---- groups -----------------------------------------------------------------------------------------------------------------------------
std::string lanes_text(const char* what, uint32_t c, int lane, long long got, long long want)
{
    char b[160];
    std::snprintf(b, sizeof(b), "%s,case=%u,lane=%d,got=%lld,want=%lld", what, c, lane, got, want);
    return b;
}

void prefix_min_cases(std::vector<int>& in, std::vector<std::string>& names)
{
    Rng rng(11);
    auto add = [&](const char* name, const int* k) { in.insert(in.end(), k, k + 64); names.push_back(name); };
    int k[64];
    for (int r = 0; r < 256; ++r) { for (int l = 0; l < 64; ++l) k[l] = rng.key31(); add("random31", k); }
    for (int r = 0; r < 256; ++r) { for (int l = 0; l < 64; ++l) k[l] = int(uint32_t(rng.next())); add("random-signed", k); }
    for (int r = 0; r < 64; ++r) { for (int l = 0; l < 64; ++l) k[l] = int(rng.below(4)); add("random-ties", k); }
    for (int l = 0; l < 64; ++l) k[l] = 100 + 3 * l; add("ascending", k);
    for (int l = 0; l < 64; ++l) k[l] = 1000 - 3 * l; add("descending", k);
    for (int l = 0; l < 64; ++l) k[l] = 77; add("all-equal", k);
    for (int l = 0; l < 64; ++l) k[l] = 0x7FFFFFFF; add("all-equal-max", k);
    static const int edges[8] = { 0, 15, 16, 31, 32, 47, 48, 63 };
    for (int at : edges)
    {
        for (int l = 0; l < 64; ++l) k[l] = 1000 + int(rng.below(1000));          // nothing before `at` is a smaller key ...
        k[at] = 5;
        add("minimum-at-edge", k);
        for (int l = 0; l < 64; ++l) k[l] = 2000 - l;                             // ... and once with a falling ramp before and after it
        k[at] = 5;
        add("minimum-at-edge-on-ramp", k);
    }
}

bool group_prefix_min()
{
    Group g("prefix_min");
    std::vector<int> in; std::vector<std::string> names;
    prefix_min_cases(in, names);
    const uint32_t ncases = uint32_t(names.size());
    DeviceBuf<int> dIn(in.size()), dOut(in.size());
    dIn.up(in); dOut.fill(0xEE);
    hipLaunchKernelGGL(prefix_min_wrap, dim3(ncases), dim3(64), 0, 0, dIn.p, dOut.p);
    after_launch();
    std::vector<int> out; dOut.down(out);
    for (uint32_t c = 0; c < ncases; ++c)
    {
        int want[64];
        serial_prefix_min(&in[c * 64], want);
        int bad = -1;
        for (int l = 0; l < 64 && bad < 0; ++l) if (out[c * 64 + l] != want[l]) bad = l;
        g.result(bad < 0, bad < 0 ? "" : lanes_text(names[c].c_str(), c, bad, out[c * 64 + bad], want[bad]));
    }
    return g.report();
}

constexpr uint32_t kSelReps = 128;

bool group_selection()
{
    Group g("selection");
    const uint32_t ncases = kSelFamilies * 4 * kSelReps;          // 4 608
    std::vector<int> e(size_t(ncases) * 64), nOf(ncases);
    Rng rng(23);
    for (uint32_t c = 0; c < ncases; ++c)
    {
        const int family = int(c / (4 * kSelReps)), ni = int((c / kSelReps) % 4);
        nOf[c] = kSelN[ni];
        selection_keys(family, c % kSelReps, rng, &e[size_t(c) * 64]);
    }
    DeviceBuf<int> dE(e.size()), dN(ncases), dEo(e.size());
    DeviceBuf<uint32_t> dSo(e.size());
    dE.up(e); dN.up(nOf); dEo.fill(0xEE); dSo.fill(0xEE);
    hipLaunchKernelGGL(selection_wrap, dim3((ncases + 3) / 4), dim3(256), 0, 0, dE.p, dN.p, ncases, dEo.p, dSo.p);
    after_launch();
    std::vector<int> eo; std::vector<uint32_t> so;
    dEo.down(eo); dSo.down(so);
    for (uint32_t c = 0; c < ncases; ++c)
    {
        int we[64]; uint32_t ws[64];
        for (int l = 0; l < 64; ++l) { we[l] = e[size_t(c) * 64 + l]; ws[l] = uint32_t(l); }
        serial_selection(we, ws, nOf[c]);
        int bad = -1; bool keyBad = false;
        for (int l = 0; l < 64 && bad < 0; ++l)
        {
            if (eo[size_t(c) * 64 + l] != we[l]) { bad = l; keyBad = true; }
            else if (so[size_t(c) * 64 + l] != ws[l]) bad = l;
        }
        if (bad < 0) { g.result(true, ""); continue; }
        char what[64];
        std::snprintf(what, sizeof(what), "%s,n=%d,%s", kSelFamilyName[c / (4 * kSelReps)], nOf[c], keyBad ? "key" : "shape");
        g.result(false, keyBad ? lanes_text(what, c, bad, eo[size_t(c) * 64 + bad], we[bad]) : lanes_text(what, c, bad, so[size_t(c) * 64 + bad], ws[bad]));
    }
    return g.report();
}

constexpr uint32_t kGuard = 256;

// One sort launched as both encoders launch it; returns "" when the result meets the contract. gateMode 0: no gate pointer, 1: gate closed
// (*gate < gateMin), 2: *gate == gateMin, 3: *gate > gateMin.
std::string sort_once(const std::vector<uint32_t>& tinfo, int gateMode, DeviceBuf<uint32_t>& dTinfo, DeviceBuf<uint2>& dOrder, DeviceBuf<uint32_t>& dCounters,
                      DeviceBuf<uint32_t>& dGate, std::vector<uint2>& order, std::vector<uint8_t>& seenBits)
{
    const uint32_t ntasks = uint32_t(tinfo.size());
    HIP_OK(hipMemcpy(dTinfo.p, tinfo.data(), size_t(ntasks) * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dOrder.p, 0xFF, (size_t(ntasks) + kGuard) * sizeof(uint2)));
    HIP_OK(hipMemset(dCounters.p, 0, 64 * sizeof(uint32_t)));
    const uint32_t gateMin = gateMode == 0 ? 0u : 5u;
    const uint32_t gateVal = gateMode == 1 ? 4u : gateMode == 2 ? 5u : 9u;
    HIP_OK(hipMemcpy(dGate.p, &gateVal, 4, hipMemcpyHostToDevice));
    const uint32_t* gate = gateMode == 0 ? nullptr : dGate.p;
    const uint32_t binGroups = std::min<uint32_t>(kBinGroups, (ntasks + 255) / 256);
    hipLaunchKernelGGL(bc7_bin_count_kernel, dim3(binGroups), dim3(256), 0, 0, dTinfo.p, ntasks, dCounters.p, gate, gateMin);
    after_launch();
    hipLaunchKernelGGL(bc7_bin_scan_kernel, dim3(1), dim3(1), 0, 0, dCounters.p);
    after_launch();
    uint32_t afterScan[64];
    HIP_OK(hipMemcpy(afterScan, dCounters.p, sizeof(afterScan), hipMemcpyDeviceToHost));
    hipLaunchKernelGGL(bc7_bin_scatter_kernel, dim3(binGroups), dim3(256), 0, 0, dTinfo.p, ntasks, dCounters.p, dOrder.p, gate, gateMin);
    after_launch();
    uint32_t counters[64];
    HIP_OK(hipMemcpy(counters, dCounters.p, sizeof(counters), hipMemcpyDeviceToHost));
    order.resize(size_t(ntasks) + kGuard);
    HIP_OK(hipMemcpy(order.data(), dOrder.p, order.size() * sizeof(uint2), hipMemcpyDeviceToHost));

    char b[200];
    std::vector<uint2> want; uint32_t hist[17], end[17];
    uint32_t live = serial_sort(tinfo, want, hist, end);
    if (gateMode == 1)
    {
        for (int i = 0; i < 64; ++i) if (counters[i]) { std::snprintf(b, sizeof(b), "closed gate: counters[%d]=%u", i, counters[i]); return b; }
        live = 0;
    }
    else
    {
        for (int i = 0; i < 64; ++i)
        {
            // after the scatter every cursor has advanced over its bin: [17 + b] is the end of bin b. Every other word stays zero: the
            // queue heads (kQueueBase ..) are zeroed by the same memset and the search kernels start from them.
            const uint32_t w = (i >= 1 && i <= 16) ? hist[i] : (i >= 18 && i <= 33) ? end[i - 17] : i == 34 ? live : 0u;
            if (counters[i] != w) { std::snprintf(b, sizeof(b), "counters[%d]=%u want %u", i, counters[i], w); return b; }
            // between scan and scatter the cursors are the starts of the bins
            const uint32_t ws = (i >= 18 && i <= 33) ? end[i - 17] - hist[i - 17] : w;
            if (afterScan[i] != ws) { std::snprintf(b, sizeof(b), "after scan: counters[%d]=%u want %u", i, afterScan[i], ws); return b; }
        }
    }
    seenBits.assign((size_t(ntasks) + 7) / 8, 0);
    for (uint32_t k = 0; k < live; ++k)
    {
        const uint2 o = order[k];
        if (o.x >= ntasks) { std::snprintf(b, sizeof(b), "order[%u].x=%u beyond %u tasks", k, o.x, ntasks); return b; }
        if (o.y != tinfo[o.x]) { std::snprintf(b, sizeof(b), "order[%u]=(%u,%#x) but tinfo is %#x", k, o.x, o.y, tinfo[o.x]); return b; }
        if ((o.y >> 24) != (want[k].y >> 24)) { std::snprintf(b, sizeof(b), "order[%u] has size %u, the serial sort %u", k, o.y >> 24, want[k].y >> 24); return b; }
        if (k && (o.y >> 24) > (order[k - 1].y >> 24)) { std::snprintf(b, sizeof(b), "order[%u]: size rises from %u to %u", k, order[k - 1].y >> 24, o.y >> 24); return b; }
        if (seenBits[o.x >> 3] & (1u << (o.x & 7))) { std::snprintf(b, sizeof(b), "order[%u]: task %u twice", k, o.x); return b; }
        seenBits[o.x >> 3] |= uint8_t(1u << (o.x & 7));
    }
    // `live` distinct live tasks out of `live`: each exactly once
    for (size_t k = live; k < order.size(); ++k)
        if (order[k].x != 0xFFFFFFFFu || order[k].y != 0xFFFFFFFFu)
        {
            std::snprintf(b, sizeof(b), "order[%zu]=(%#x,%#x) written, %u live of %u tasks", k, order[k].x, order[k].y, live, ntasks);
            return b;
        }
    return "";
}

bool group_bin_sort()
{
    Group g("bin_sort");
    const uint32_t maxTasks = kSortSizes[6];
    DeviceBuf<uint32_t> dTinfo(maxTasks), dCounters(64), dGate(1);
    DeviceBuf<uint2> dOrder(size_t(maxTasks) + kGuard);
    std::vector<uint32_t> tinfo; std::vector<uint2> order; std::vector<uint8_t> bits;
    Rng rng(37);
    for (uint32_t ntasks : kSortSizes)
        for (int family = 0; family < kSortFamilies; ++family)
        {
            sort_tinfo(family, ntasks, rng, tinfo);
            // every case ungated; the gate's three states on the uniform family and, so that a closed gate also meets one-bin lists, on bin 16
            const int gateModes = (family == 0 || family == 4) ? 4 : 1;
            for (int gm = 0; gm < gateModes; ++gm)
            {
                const std::string bad = sort_once(tinfo, gm, dTinfo, dOrder, dCounters, dGate, order, bits);
                char what[64];
                std::snprintf(what, sizeof(what), "%s,ntasks=%u,gate=%d:", kSortFamilyName[family], ntasks, gm);
                g.result(bad.empty(), std::string(what) + bad);
                if (!bad.empty() && g.failed >= 8) return g.report();          // a broken sort fails everywhere: enough said
            }
        }
    return g.report();
}

bool group_queue()
{
    Group g("queue");
    static const uint32_t lives[9] = { 0u, 1u, 63u, 64u, 65u, 4097u, 524288u, 524289u, 536633u };
    static const uint32_t waves[3] = { 1u, 7u, 256u };
    constexpr uint32_t kSeenGuard = 64;
    DeviceBuf<uint32_t> dSeen(size_t(lives[8]) + kSeenGuard), dHead(1), dErrs(4);
    std::vector<uint32_t> seen(dSeen.n);
    uint32_t salt = 1;
    for (uint32_t live : lives)
        for (uint32_t nw : waves)
        {
            dSeen.fill(0); dHead.fill(0); dErrs.fill(0);
            // a turn with an idle lane and an index in reserve hands out at least one index, the turn that finds the list drained none:
            // a wave needs at most live + 1 turns whatever the other waves do
            const uint32_t cap = live + 8u;
            hipLaunchKernelGGL(queue_wrap, dim3(nw), dim3(64), 0, 0, dHead.p, live, dSeen.p, dErrs.p, cap, salt++);
            after_launch();
            uint32_t errs[4], head = 0;
            HIP_OK(hipMemcpy(errs, dErrs.p, sizeof(errs), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(&head, dHead.p, 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(seen.data(), dSeen.p, seen.size() * 4, hipMemcpyDeviceToHost));
            char b[200]; b[0] = 0;
            if (errs[0] || errs[1] || errs[2])
                std::snprintf(b, sizeof(b), "live=%u,waves=%u: %u indices beyond the list, %u waves at the cap of %u turns, %u indices to busy lanes", live, nw, errs[0], errs[1], cap, errs[2]);
            else if (head < live)
                std::snprintf(b, sizeof(b), "live=%u,waves=%u: head stops at %u", live, nw, head);
            else
                for (size_t k = 0; k < seen.size(); ++k)
                    if (seen[k] != (k < live ? 1u : 0u)) { std::snprintf(b, sizeof(b), "live=%u,waves=%u: seen[%zu]=%u", live, nw, k, seen[k]); break; }
            g.result(b[0] == 0, b);
        }
    return g.report();
}

// ---- reference mode: the serial references against properties that do not depend on them ---------------------------------------------
bool reference_mode()
{
    bool ok = true;
    {
        Group g("reference_prefix_min");
        std::vector<int> in; std::vector<std::string> names;
        prefix_min_cases(in, names);
        for (size_t c = 0; c < names.size(); ++c)
        {
            int out[64]; serial_prefix_min(&in[c * 64], out);
            bool good = out[0] == in[c * 64];
            for (int l = 0; l < 64 && good; ++l)
            {
                bool attained = false;          // a lower bound of lanes 0..l that one of them attains
                for (int k = 0; k <= l; ++k) { good &= out[l] <= in[c * 64 + k]; attained |= out[l] == in[c * 64 + k]; }
                good &= attained;
            }
            g.result(good, names[c]);
        }
        ok &= g.report();
    }
    {
        Group g("reference_selection");
        Rng rng(23);
        for (uint32_t c = 0; c < kSelFamilies * 4 * kSelReps; ++c)
        {
            const int family = int(c / (4 * kSelReps)), n = kSelN[(c / kSelReps) % 4];
            int e0[64], e[64]; uint32_t s[64];
            selection_keys(family, c % kSelReps, rng, e0);
            for (int l = 0; l < 64; ++l) { e[l] = e0[l]; s[l] = uint32_t(l); }
            serial_selection(e, s, n);
            std::string bad;
            // the multiset of (e, s) pairs is preserved: s is a permutation of the lanes and every key is still with its lane
            bool used[64] = {};
            for (int l = 0; l < 64 && bad.empty(); ++l)
            {
                if (s[l] >= 64 || used[s[l]]) bad = "shapes are no permutation";
                else if (e[l] != e0[s[l]]) bad = "a key left its shape";
                else used[s[l]] = true;
            }
            // e[0 .. n) are the n smallest keys in non-decreasing order, and nothing behind them is smaller
            std::vector<int> sorted(e0, e0 + 64);
            std::sort(sorted.begin(), sorted.end());
            for (int i = 0; i < n && bad.empty(); ++i) if (e[i] != sorted[i]) bad = "the first n are not the n smallest in order";
            for (int i = 0; i < n && bad.empty(); ++i) for (int j = n; j < 64; ++j) if (e[i] > e[j]) bad = "a key behind the first n is smaller";
            char what[96];
            std::snprintf(what, sizeof(what), "%s,n=%d,case=%u:", kSelFamilyName[family], n, c);
            g.result(bad.empty(), std::string(what) + bad);
        }
        ok &= g.report();
    }
    {
        Group g("reference_sort");
        Rng rng(37);
        std::vector<uint32_t> tinfo; std::vector<uint2> order;
        for (uint32_t ntasks : { 1u, 255u, 256u, 257u, 4099u, 70001u })
            for (int family = 0; family < kSortFamilies; ++family)
            {
                sort_tinfo(family, ntasks, rng, tinfo);
                uint32_t hist[17], end[17];
                const uint32_t live = serial_sort(tinfo, order, hist, end);
                std::string bad;
                uint32_t liveWant = 0;
                for (uint32_t ti : tinfo) liveWant += (ti >> 24) ? 1 : 0;
                if (live != liveWant || order.size() != live) bad = "live count";
                std::vector<uint8_t> used(ntasks, 0);
                for (uint32_t k = 0; k < live && bad.empty(); ++k)
                {
                    const uint2 o = order[k];
                    if (o.x >= ntasks || used[o.x]) bad = "no permutation of the live tasks";
                    else if (o.y != tinfo[o.x] || !(o.y >> 24)) bad = "an entry is not (t, tinfo[t]) of a live task";
                    else if (k && (o.y >> 24) > (order[k - 1].y >> 24)) bad = "sizes rise";
                    else used[o.x] = 1;
                }
                for (int b = 1; b <= 16 && bad.empty(); ++b)
                    if (end[b] > live || (end[b] && (order[end[b] - 1].y >> 24) < uint32_t(b)) || (end[b] < live && (order[end[b]].y >> 24) >= uint32_t(b))) bad = "a bin's end";
                char what[96];
                std::snprintf(what, sizeof(what), "%s,ntasks=%u:", kSortFamilyName[family], ntasks);
                g.result(bad.empty(), std::string(what) + bad);
            }
        ok &= g.report();
    }
    return ok;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "reference") return reference_mode() ? 0 : 1;
    if (argc > 1) { std::fprintf(stderr, "usage: %s [reference]\n", argv[0]); return 2; }
    HIP_OK(hipSetDevice(0));
    bool ok = group_prefix_min();
    ok &= group_selection();
    ok &= group_bin_sort();
    ok &= group_queue();
    return ok ? 0 : 1;
}
