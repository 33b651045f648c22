// Device shim of full_wave_scan_add (grid_ndt_amd/csrc/gndt_blocked.hpp) for tests/test_gpu_blocked_instr.py: one wave per 64 inputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gndt_blocked.hpp"

namespace {

__global__ void __launch_bounds__(64) k_wave_scan(const uint32_t* __restrict__ in, uint32_t* __restrict__ incl, uint32_t* __restrict__ totals) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    uint32_t total;
    const uint32_t x = gndt::full_wave_scan_add(in[i], total);
    incl[i] = x;
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

}  // namespace

// in, incl: 64 * waves values; totals: one per wave
extern "C" int wshim_scan(const uint32_t* in, uint32_t* incl, uint32_t* totals, uint32_t waves, hipStream_t stream) {
    if (waves == 0) return 0;
    hipLaunchKernelGGL(k_wave_scan, dim3(waves), dim3(64), 0, stream, in, incl, totals);
    return (int)hipGetLastError();
}
