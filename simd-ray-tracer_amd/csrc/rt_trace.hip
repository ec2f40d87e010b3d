// rt_trace.hip — the trace launches of every shape but P = 16 (rtk_trace.h).
#include "rtk_trace.h"

extern "C" int rtk_launch_trace_grid(const TraceArgs *a, int simd, int src, int cull, int lanes_per_pixel,
                                     uint32_t n_blocks, hipStream_t stream) {
    if (n_blocks == 0) return 0;
    if (a->tile_counts_at) {  // per-tile counts: the kernels compiled with kWalkTileCounts (rt_trace_tc.hip)
        if (!a->sel) return -1;  // (the table is indexed by the selection's reference tiles)
        rtk_launch_tile_counts(a, simd, src, cull, lanes_per_pixel, n_blocks, stream);
        return hipGetLastError() == hipSuccess ? 0 : -5;
    }
    switch (lanes_per_pixel) {
        case 32: launch_p<32>(a, simd, src, cull, n_blocks, stream); break;
        case 16: rtk_launch_p16(a, simd, src, cull, n_blocks, stream); break;  // (rt_trace_p16.hip)
        case 8: launch_p<8>(a, simd, src, cull, n_blocks, stream); break;
        case 4: launch_p<4>(a, simd, src, cull, n_blocks, stream); break;
        case 2: launch_p<2>(a, simd, src, cull, n_blocks, stream); break;
        case 0: launch_p<0>(a, simd, src, cull, n_blocks, stream); break;
        default: launch_p<1>(a, simd, src, cull, n_blocks, stream); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int rtk_launch_trace(const TraceArgs *a, int simd, int src, int cull, int lanes_per_pixel,
                                hipStream_t stream) {
    return rtk_launch_trace_grid(a, simd, src, cull, lanes_per_pixel,
                                 rtk_tile_count(a->width, a->local_rows, lanes_per_pixel), stream);
}
