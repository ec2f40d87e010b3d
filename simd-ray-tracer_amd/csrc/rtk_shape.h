// rtk_shape.h — the launch geometry shared by the trace kernels (rtk_trace.h)
// and the scheduling kernels (rt_sched.hip): wave tile shapes, ring and mask
// sizes, the secondary-walk variants and the occupancy targets.
#pragma once
#include <stdint.h>

#include "rt_kernel.h"

namespace rtk {

constexpr int kWavesPerBlock = 4;
// primary pair mask words per wave tile (rtk_mask_words): the LDS-image kernels keep this
// small (it is static LDS, and C2's blocks fill the CU's 160 KB 7 times)
template <bool GS>
struct MaskWords {
    static constexpr int N = GS ? (int)((2u * kMaxGroups + 63u) / 64u) : (int)((2u * kMaxLdsGroups + 63u) / 64u);
};
constexpr uint32_t kFoldTable = 256;
// Per-pixel out-of-order sample slots (LDS ring): at least P (every sample
// lane holds one sample in flight) plus slack: 16 per pixel at P <= 4 (12 and
// 32 measured slower), 2 per sample lane above.  A multiple of 4, so a
// whole-batch fold never wraps.
template <int P>
struct Ring {
    static constexpr uint32_t N = P <= 4 ? 16u : 2u * (uint32_t)P;
};

#ifndef RTK_SOLO_WAVES_PER_SIMD  // the same target for the one-wave kernels (A/B: make variant KFLAGS=-DRTK_SOLO_WAVES_PER_SIMD=8)
#define RTK_SOLO_WAVES_PER_SIMD 7
#endif
#ifndef RTK_MIN_WAVES_PER_SIMD  // occupancy target (VGPR budget) of the production (SMEM) kernels;
#define RTK_MIN_WAVES_PER_SIMD 7   // 7 waves = 72 VGPRs, no VGPR spills: measured best on C2 with the
#endif                             // cluster walk (w6 116.5k, w7 120.0-121.1k, w8 118.2k Mrays/s, w8 spills)

// Work shape.  A wave owns a small pixel tile and P lanes per pixel: the
// lanes of a pixel take its samples in order as they free up (kDynamic in
// trace_kernel), park each finished sample's radiance in a per-pixel LDS
// ring, and the pixel's owner lane (j == 0) folds the ring into the running
// mean strictly in sample order (main.cpp:484-487), so results are
// bit-identical to one lane tracing the samples one after another.  P > 1
// splits the long per-pixel sample chains of pixels that see geometry over
// several lanes: the heaviest waves get P times shorter, which removes most
// of the kernel's tail.  Tiles: P=1 8x8, P=2 8x4, P=4 4x4 pixels per wave.
// P = 0 is the other direction, for launches of one frame (the reference's
// OnRender unit): one lane per pixel and kPixelsPerLane pixels per lane over a
// 16x16 wave tile (slot q of lane l: the 8x8 quadrant q, pixel l of it).  A
// lane whose path ends starts its next pixel's sample in the next primary
// round, so a wave stays full instead of draining after one pass, and a
// launch has a quarter of the waves (each of which pays the wave's setup once).
constexpr uint32_t kPixelsPerLane = 4;
template <int P>
struct Shape {
    static constexpr uint32_t LP = P == 0 ? 1u : (uint32_t)P;         // lanes per pixel
    static constexpr uint32_t Q = P == 0 ? kPixelsPerLane : 1u;       // pixels per lane
    static constexpr uint32_t TW = P == 0 ? 16u : P <= 2 ? 8u : P <= 8 ? 4u : 2u;
    static constexpr uint32_t TH = P == 0 ? 16u : P == 1 ? 8u : P <= 4 ? 4u : P <= 16 ? 2u : 1u;
    static_assert(TW * TH * LP == 64u * Q, "a wave is 64 lanes");
    // a block tile (2TW x 2TH) lies in exactly one reference tile, so a tile selection
    // (TraceArgs.sel) is a set of whole block tiles
    static_assert(kRefTile % (2u * TW) == 0 && kRefTile % (2u * TH) == 0, "block tiles divide the reference tile");
};

// Occupancy target of the one-wave kernels per secondary walk: the two-word
// scene-wide cluster walk (C5: 256 spheres) takes 8 waves/SIMD (63 VGPRs, the
// cull mask in dynamic LDS leaves room for 32 workgroups per CU): C5 +2.7 %
// same-box, while C2 (one word) and RTWeekend (four per-lane words) lose
// 1.5 % and 0.5 % at 8 and keep 7.
#ifndef RTK_SOLO_WAVES_CL2
#define RTK_SOLO_WAVES_CL2 8
#endif
constexpr int solo_waves(int walk) { return walk == kWalkCl2 ? RTK_SOLO_WAVES_CL2 : RTK_SOLO_WAVES_PER_SIMD; }

// What a kWalk* value (rt_kernel.h) compiles into a trace kernel
template <int WALK> struct Walk {
    // the per-group walk (small scenes) may merge primary and secondary rounds
    static constexpr bool MERGEABLE = WALK == kWalkAny || WALK == kWalkGroups;
    static constexpr int W = WALK == kWalkCl2 || WALK == kWalkCl2Rel ? 2 : WALK == kWalkCl4 || WALK == kWalkCl4Rel ? 4 : 1;
    static constexpr bool REL = WALK == kWalkCl1Rel || WALK == kWalkCl2Rel || WALK == kWalkCl4Rel;
    static constexpr bool CLUSTERS = WALK >= kWalkCl1;
    // member entries by the direction table (rtk_walk.h direction_groups); DIR64: its masks are 64 bits wide
    static constexpr bool DIR = WALK == kWalkCl1Dir || WALK == kWalkCl1Dir64;
    static constexpr bool DIR64 = WALK == kWalkCl1Dir64;
};

}  // namespace rtk

// F<P>(...) for the launch shape code lanes_per_pixel (0: kPixelsPerLane pixels per lane)
#define RTK_BY_P(F, ...)                                     \
    switch (lanes_per_pixel) {                               \
        case 32: F<32>(__VA_ARGS__); break;                  \
        case 16: F<16>(__VA_ARGS__); break;                  \
        case 8: F<8>(__VA_ARGS__); break;                    \
        case 4: F<4>(__VA_ARGS__); break;                    \
        case 2: F<2>(__VA_ARGS__); break;                    \
        case 0: F<0>(__VA_ARGS__); break;                    \
        default: F<1>(__VA_ARGS__); break;                   \
    }
