// rt_first_hit.hip — rt_trace_first_hit: the first segment of every pixel's path as a pass of its own.
// Per pixel: the primary ray (start_sample), the exact pair tests of the pairs its wave tile's cone may
// reach (the cull pass's cone test, run here per wave and kept in registers), one hit select, and
// the winner's sphere, depth, normal and albedo stored to the caller's planes.  No trip loop, no ring,
// no LDS, no atomics; the functions are the trace kernel's own (rtk_math.h, rtk_walk.h, rtk_cull.h),
// so the bits are those of trace_kernel's first segment.
#include "rtk_cull.h"
#include "rtk_walk.h"

namespace rtk {

constexpr uint32_t kHitMiss = 0xFFFFFFFFu;  // RT_HIT_MISS (rt_trace.h; bit 31 of a key is kKeyInside = RT_HIT_INSIDE)

// One wave per 8x8 wave tile of Shape<1>, one lane per pixel; four waves per block over the 16x16 block
// tile, which lies in one reference tile (rtk_shape.h), so the bitmap decides per block (tile_selected<1>).
// CULL off (a device created with Cull off): every pair of every group is tested.
// CENTRE: RT_HIT_PIXEL_CENTRE (start_sample<true>).
template <bool SIMD, bool CULL, bool CENTRE>
__global__ __launch_bounds__(256) void first_hit_kernel(TraceArgs a, uint2 *hit, float4 *normal, float4 *albedo) {
    constexpr uint32_t TW = Shape<1>::TW, TH = Shape<1>::TH;
    const uint32_t tile = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tile_x = tile % a.tiles_x, tile_y = tile / a.tiles_x;
    if (!tile_selected<1>(a, tile_x, tile_y)) return;  // (block-uniform; no byte of the tile is written)
    const uint32_t x0 = tile_x * (2u * TW) + (wave & 1u) * TW, y0 = tile_y * (2u * TH) + (wave >> 1) * TH;
    if (x0 >= a.width || y0 >= a.height) return;  // a wave tile outside the image (wave-uniform; the kernel has no barrier)
    const uint32_t x = x0 + lane % TW, y = y0 + lane / TW;
    const bool valid = x < a.width && y < a.height;
    const bool fast = a.fast_sqrt != 0u;
    const uint32_t n_pairs = 2u * a.n_groups, n_words = rtk_mask_words(a.n_groups);
    Cone cone;
    if (CULL)
        cone = tile_cone(a, (double)x0 - 0.501, (double)(x0 + TW - 1u) + 0.501, (double)y0 - 0.501,
                         (double)(y0 + TH - 1u) + 0.501);
    Sample p;
    RayPk ray;
    Hit h;
    hit_reset(h);
    bool started = false;  // (wave-uniform: a wave whose every word is zero forms no ray)
    for (uint32_t w = 0; w < n_words; ++w) {
        // the word's pairs: the tile's cone test (a ballot), or every pair of the scene; nothing is stored
        uint64_t m;
        if (CULL) {
            m = wave_tile_mask<1>(a, cone, w, lane);
        } else {
            const uint32_t left = n_pairs - 64u * w;
            m = left >= 64u ? ~0ull : (1ull << left) - 1ull;
        }
        // (readfirstlane returns int: widen each half as u32, as the trace kernel's primary rounds do)
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)m);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(m >> 32));
        m = (uint64_t)lo | ((uint64_t)hi << 32);
        if (m != 0 && !started) {
            start_sample<CENTRE>(a, x, y, a.prev_count, p);
            ray = {p.rx, p.ry, p.rz};
            started = true;
        }
        while (m) {  // the tile's sphere pairs, in the reference's order
            const uint32_t pr = w * 64u + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t g = pr >> 1;
            const Group G = load_group_at((cv4f_t *)a.groups + kGroupF4 * g);
            recheck_pairs<SIMD>(a, G, g, ray, h, fast, (pr & 1u) == 0u, (pr & 1u) != 0u);
        }
    }
    // ---- hit select, as trace_kernel spells it (x64_math.h:579-585 HorizontalMin + first equal lane;
    // the scalar rules' one slot and its own flag)
    float tmin;
    uint32_t key, sidx;
    if (SIMD) {
        asm("v_min3_f32 %0, %1, %2, %3\n\t"
            "v_min_f32 %0, %0, %4"
            : "=&v"(tmin)
            : "v"(h.t0), "v"(h.t1), "v"(h.t2), "v"(h.t3));
        key = h.t0 == tmin ? h.k0 : h.t1 == tmin ? h.k1 : h.t2 == tmin ? h.k2 : h.k3;
        sidx = key & ~kKeyInside;
    } else {
        tmin = h.t0;
        sidx = h.k0;
        key = sidx | (h.ins != 0 ? kKeyInside : 0u);
    }
    if (!valid) return;  // pixels of the wave tile outside the image write nothing
    const size_t pix = (size_t)y * a.width + x;
    if (!started || tmin == kFMax) {
        if (hit) hit[pix] = make_uint2(kHitMiss, __float_as_uint(kFMax));
        if (normal) normal[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (albedo) albedo[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    if (hit) hit[pix] = make_uint2(key, __float_as_uint(tmin));
    if (normal || albedo) {
        // the winner's record, gathered per lane, and HitNormal as shade_hit and shade form it
        const float4 *rec = a.materials + kSphereF4 * sidx;
        if (normal) {
            const float4 sc = rec[0];
            const float cx = sc.x - p.rx.x, cy = sc.y - p.ry.x, cz = sc.z - p.rz.x;
            const float ipx = p.rx.y * tmin, ipy = p.ry.y * tmin, ipz = p.rz.y * tmin;
            float nx = ipx - cx, ny = ipy - cy, nz = ipz - cz;
            normalize(nx, ny, nz);
            if ((key & kKeyInside) != 0u) {
                nx = -nx;
                ny = -ny;
                nz = -nz;
            }
            normal[pix] = make_float4(nx, ny, nz, 0.0f);
        }
        if (albedo) {
            const float4 cs = rec[1];
            albedo[pix] = make_float4(cs.x, cs.y, cs.z, 1.0f);
        }
    }
}

}  // namespace rtk

extern "C" int rtk_launch_first_hit(const TraceArgs *a, int simd, int cull, int centre, void *hit, float *normal,
                                    float *albedo, hipStream_t stream) {
    const uint32_t tiles_y = (a->height + 2u * rtk::Shape<1>::TH - 1u) / (2u * rtk::Shape<1>::TH);
    const dim3 grid(a->tiles_x * tiles_y), block(256);
#define RTK_FIRST_HIT(S, C, J) \
    hipLaunchKernelGGL((rtk::first_hit_kernel<S, C, J>), grid, block, 0, stream, *a, (uint2 *)hit, (float4 *)normal, (float4 *)albedo)
    switch ((simd ? 4 : 0) | (cull ? 2 : 0) | (centre ? 1 : 0)) {
        case 0: RTK_FIRST_HIT(false, false, false); break;
        case 1: RTK_FIRST_HIT(false, false, true); break;
        case 2: RTK_FIRST_HIT(false, true, false); break;
        case 3: RTK_FIRST_HIT(false, true, true); break;
        case 4: RTK_FIRST_HIT(true, false, false); break;
        case 5: RTK_FIRST_HIT(true, false, true); break;
        case 6: RTK_FIRST_HIT(true, true, false); break;
        default: RTK_FIRST_HIT(true, true, true); break;
    }
#undef RTK_FIRST_HIT
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
