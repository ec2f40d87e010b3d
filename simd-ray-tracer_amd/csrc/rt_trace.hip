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

// rt_direction_union (inspection hook): one wave runs the direction walk's union (rtk_walk.h wave_or) under
// exec = lanes.  in: 64 low words, 64 high words, 64 canary words; out: the union's two words, then each
// lane's canary -- a register every lane, active or not, writes before the union and reads back after it.
__global__ void __launch_bounds__(64) direction_union_kernel(const uint32_t *in, uint64_t lanes, uint32_t wide, uint32_t *out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t lo = in[lane], hi = in[64u + lane];
    uint32_t canary = in[128u + lane];
    asm volatile("" : "+v"(canary));  // (a VGPR of its own from here on)
    if ((lanes >> lane) & 1ull) {
        const uint64_t u = wide ? rtk::wave_or<true>(lo, hi) : rtk::wave_or<false>(lo, 0u);
        if (lane == (uint32_t)__builtin_ctzll(lanes)) out[0] = (uint32_t)u, out[1] = (uint32_t)(u >> 32);
    }
    asm volatile("" : "+v"(canary));
    out[2u + lane] = canary;
}

extern "C" int rtk_launch_direction_union(const uint32_t *in, uint64_t lanes, uint32_t wide, uint32_t *out,
                                          hipStream_t stream) {
    hipLaunchKernelGGL(direction_union_kernel, dim3(1), dim3(64), 0, stream, in, lanes, wide, out);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int rtk_launch_trace(const TraceArgs *a, int simd, int src, int cull, int lanes_per_pixel,
                                hipStream_t stream) {
    return rtk_launch_trace_grid(a, simd, src, cull, lanes_per_pixel,
                                 rtk_tile_count(a->width, a->local_rows, lanes_per_pixel), stream);
}
