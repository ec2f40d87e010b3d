// rt_trace_tc.hip — the trace launches with per-tile counts (rt_trace_tile_work, TraceArgs.tile_counts_at)
// of every shape but P = 16: trace_kernel compiled with kWalkTileCounts (rtk_trace.h).  A translation
// unit of their own, so that they build beside the uniform kernels of rt_trace.hip, not after them.
#include "rtk_trace.h"

extern "C" void rtk_launch_p16_tile_counts(const TraceArgs *a, int simd, int src, int cull, uint32_t n_blocks,
                                           hipStream_t stream);  // (rt_trace_p16.hip)

extern "C" void rtk_launch_tile_counts(const TraceArgs *a, int simd, int src, int cull, int lanes_per_pixel,
                                       uint32_t n_blocks, hipStream_t stream) {
    switch (lanes_per_pixel) {
        case 32: launch_p<32, kWalkTileCounts>(a, simd, src, cull, n_blocks, stream); break;
        case 16: rtk_launch_p16_tile_counts(a, simd, src, cull, n_blocks, stream); break;
        case 8: launch_p<8, kWalkTileCounts>(a, simd, src, cull, n_blocks, stream); break;
        case 4: launch_p<4, kWalkTileCounts>(a, simd, src, cull, n_blocks, stream); break;
        case 2: launch_p<2, kWalkTileCounts>(a, simd, src, cull, n_blocks, stream); break;
        case 0: launch_p<0, kWalkTileCounts>(a, simd, src, cull, n_blocks, stream); break;
        default: launch_p<1, kWalkTileCounts>(a, simd, src, cull, n_blocks, stream); break;
    }
}
