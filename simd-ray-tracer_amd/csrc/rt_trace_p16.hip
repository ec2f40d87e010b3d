// rt_trace_p16.hip — the P = 16 trace launches (the 8-GPU band shares),
// a translation unit of their own because the Makefile builds it, and only it, under
// the scheduler's register-pressure trackers (-amdgpu-use-amdgpu-trackers): about
// -1.4 % on the 8-rank share over two same-box A/Bs (0.770 against 0.781 ms, near
// the noise), while the same flag costs the P = 4 kernel of one GPU 1.7 %
// (profiles/r02_sched_trackers_ab.txt).
#include "rtk_trace.h"

extern "C" void rtk_launch_p16(const TraceArgs *a, int simd, int src, int cull, uint32_t n_blocks,
                               hipStream_t stream) {
    launch_p<16>(a, simd, src, cull, n_blocks, stream);
}

// the same shape with per-tile counts (rt_trace_tc.hip dispatches here)
extern "C" void rtk_launch_p16_tile_counts(const TraceArgs *a, int simd, int src, int cull, uint32_t n_blocks,
                                           hipStream_t stream) {
    launch_p<16, kWalkTileCounts>(a, simd, src, cull, n_blocks, stream);
}
