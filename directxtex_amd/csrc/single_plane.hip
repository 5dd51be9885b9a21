// ConvertToSinglePlane (DirectXTexConvert.cpp:4944-5077) on gfx950: NV12 / NV11 -> YUY2, P010 -> Y210, P016 -> Y216.
//
// Pure streaming, no LDS: blockIdx.z picks the job from the argument block, blockIdx.x the 256 lanes of a row (dxtex_plane.h: the wide
// groups of 16 destination bytes, then one lane per remaining element), blockIdx.y the first unit (a row pair of 4:2:0, a row of NV11);
// the grid is sized for the largest job of the batch and a lane outside its own job's extent leaves at once. What a lane reads and writes is
// plane_lane(), which the host check runs over the same geometry: every read stays below pixels + slicePitch, every write inside the
// destination's written elements, row padding is never written.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_plane.h"
#include <algorithm>

namespace dxtex
{
__global__ void __launch_bounds__(kPlaneThreads) single_plane_kernel(PlaneBatch batch)
{
    const PlaneJob& j = batch.job[blockIdx.z];
    const uint32_t gx = blockIdx.x * kPlaneThreads + threadIdx.x;
    if (gx >= plane_lanes(j)) return;
    for (uint32_t unit = blockIdx.y; unit < j.units; unit += gridDim.y) plane_lane(j, gx, unit);
}

hipError_t launch_single_plane(const PlaneJob* jobs, size_t count, hipStream_t stream, KernelMarks* marks)
{
    for (size_t first = 0; first < count; first += kPlaneBatchMax)
    {
        PlaneBatch batch;
        batch.count = uint32_t(std::min<size_t>(kPlaneBatchMax, count - first));
        for (uint32_t k = 0; k < kPlaneBatchMax; ++k) batch.job[k] = k < batch.count ? jobs[first + k] : PlaneJob{};
        uint32_t gx = 0, gy = 0;
        plane_grid(batch, gx, gy);
        if (!gx || !gy) continue;
        if (marks) marks->mark("single_plane_kernel");
        hipLaunchKernelGGL(single_plane_kernel, dim3(gx, gy, batch.count), dim3(kPlaneThreads), 0, stream, batch);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (marks) marks->mark(nullptr);
    return hipSuccess;
}
} // namespace dxtex
