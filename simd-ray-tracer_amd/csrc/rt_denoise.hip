// rt_denoise.hip — rt_denoise: one pass of the edge-avoiding a-trous filter over a running mean and
// rt_trace_first_hit's planes (the filter is defined, operation by operation, in rt_trace.h).  A 5 x 5 tap
// pattern at step s; a tap enters with the product of the kernel weight and up to three tent falloffs
// (normal, depth, luminance), and only where it saw the sphere the centre saw.  Every operation is one f32
// operation in the stated order (-ffp-contract=off, the compiler's IEEE division), so both shapes below and
// the numpy restatement (tests/denoise_ref.py) give the same bits.
//
// Two shapes of one pass, over the same per-pixel function (filter_pixel):
//   direct  one thread per pixel, 64 x 4 pixels per block, every tap read from global memory: the lanes of a
//           wave are neighbours in x at every step, so each tap is one coalesced load.
//   lds     a block takes 32 x 8 pixels of ONE residue class modulo s -- x = rx + s u, y = ry + s v -- so the
//           taps of its pixels are the dense (32 + 4) x (8 + 4) tile of that class; it is loaded once into
//           LDS (colour, hit, and where the stop needs them luminance and normal) and every tap reads LDS.
// launch_lds() routes a pass to one of them by its step: lds up to step 8, direct from 16 on (measured:
// DESIGN.md, profiles/denoise_ab.txt).
// -DRTK_DENOISE_SHAPE=0 / =1 (make variant KFLAGS=...) forces direct / lds for every step: the A/B builds of
// scripts/denoise_ab.py.
#include "rtk_math.h"

namespace rtk {

constexpr uint32_t kDenoiseMiss = 0xFFFFFFFFu;  // RT_HIT_MISS
constexpr int kDnTX = 32, kDnTY = 8, kDnHalo = 2;
constexpr int kDnLW = kDnTX + 2 * kDnHalo, kDnLH = kDnTY + 2 * kDnHalo, kDnLN = kDnLW * kDnLH;  // 36 x 12 = 432 entries

__device__ __forceinline__ float dn_lum(const float4 &c) {
    const float a = 0.2126f * c.x, b = 0.7152f * c.y, d = 0.0722f * c.z;
    return (a + b) + d;
}
__device__ __forceinline__ float dn_pos(float v) { return v > 0.0f ? v : 0.0f; }  // (a NaN gives 0)
__device__ __forceinline__ float dn_albedo(float c) { return c > 0.01f ? c : 0.01f; }

// I_i[q]: src[q]; in pass 0 of the demodulated variant Mean[q] / a[q] (a = 1 on a miss: the value itself)
__device__ __forceinline__ float4 dn_load_colour(const DenoiseArgs &a, size_t q) {
    float4 c = ((const float4 *)a.src)[q];
    if (a.demod_in) {
        const float4 al = ((const float4 *)a.albedo)[q];
        if (al.w == 1.0f) {
            c.x = c.x / dn_albedo(al.x);
            c.y = c.y / dn_albedo(al.y);
            c.z = c.z / dn_albedo(al.z);
        }
    }
    return c;
}

// Where the taps of pixel (x, y) come from: global memory ...
struct DirectTaps {
    const DenoiseArgs &a;
    using Handle = size_t;
    __device__ __forceinline__ Handle at(int, int, int qx, int qy) const { return (size_t)qy * a.width + (size_t)qx; }
    __device__ __forceinline__ uint2 hit(Handle q) const { return ((const uint2 *)a.hit)[q]; }
    __device__ __forceinline__ float4 normal(Handle q) const { return ((const float4 *)a.normal)[q]; }
    __device__ __forceinline__ float4 colour(Handle q) const { return dn_load_colour(a, q); }
    __device__ __forceinline__ float lum(Handle, const float4 &c) const { return dn_lum(c); }
};
// ... or the block's LDS tile, where (lu, lv) is the pixel's place in it
struct LdsTaps {
    const float4 *col, *nrm;
    const uint2 *hits;
    const float *lums;
    int lu, lv;
    using Handle = int;
    __device__ __forceinline__ Handle at(int dx, int dy, int, int) const {
        return (lv + kDnHalo + dy) * kDnLW + lu + kDnHalo + dx;
    }
    __device__ __forceinline__ uint2 hit(Handle e) const { return hits[e]; }
    __device__ __forceinline__ float4 normal(Handle e) const { return nrm[e]; }
    __device__ __forceinline__ float4 colour(Handle e) const { return col[e]; }
    __device__ __forceinline__ float lum(Handle e, const float4 &) const { return lums[e]; }
};

// One pixel of one pass.  NRM, DEP, COL: which stops are on (NormalPower != 0, SigmaDepth > 0, SigmaColor > 0).
template <bool NRM, bool DEP, bool COL, class Taps>
__device__ __forceinline__ void filter_pixel(const DenoiseArgs &a, const Taps &t, uint32_t x, uint32_t y) {
    constexpr float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const int s = (int)a.step, w_img = (int)a.width, h_img = (int)a.height;
    const auto hc = t.at(0, 0, (int)x, (int)y);
    const uint2 hp = t.hit(hc);
    const uint32_t kp = hp.x;
    const float tp = __uint_as_float(hp.y);
    const bool surface = kp != kDenoiseMiss;
    const float4 cp = t.colour(hc);
    float lp = 0.0f, rz = 0.0f;
    if (COL) lp = t.lum(hc, cp);
    if (DEP && surface) rz = 1.0f / (a.sigma_depth * tp);
    float4 np = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (NRM && surface) np = t.normal(hc);
    float ax = 0.0f, ay = 0.0f, az = 0.0f, ws = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = (int)y + dy * s;
        if (qy < 0 || qy >= h_img) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = (int)x + dx * s;
            if (qx < 0 || qx >= w_img) continue;
            float w = K[dy + 2] * K[dx + 2];
            float4 cq = cp;
            if (dx != 0 || dy != 0) {
                const auto h = t.at(dx, dy, qx, qy);
                const uint2 hq = t.hit(h);
                if (hq.x != kp) continue;
                if (surface) {
                    if (NRM) {
                        const float4 nq = t.normal(h);
                        float d = dn_pos(dot3(np.x, np.y, np.z, nq.x, nq.y, nq.z));
                        for (uint32_t i = 0; i < a.normal_power; ++i) d = d * d;
                        w = w * d;
                    }
                    if (DEP) w = w * dn_pos(1.0f - fabsf(tp - __uint_as_float(hq.y)) * rz);
                }
                // (a weight that is not > 0 here stays so under the colour stop: 0 or NaN times a value in [0, 1])
                if (!(w > 0.0f)) continue;
                cq = t.colour(h);
                if (COL) {
                    w = w * dn_pos(1.0f - fabsf(lp - t.lum(h, cq)) * a.ic);
                    if (!(w > 0.0f)) continue;
                }
            }
            ax = ax + w * cq.x;
            ay = ay + w * cq.y;
            az = az + w * cq.z;
            ws = ws + w;
        }
    }
    float ox = ax / ws, oy = ay / ws, oz = az / ws;
    const size_t p = (size_t)y * a.width + x;
    if (a.remod_out) {
        const float4 al = ((const float4 *)a.albedo)[p];
        if (al.w == 1.0f) {
            ox = ox * dn_albedo(al.x);
            oy = oy * dn_albedo(al.y);
            oz = oz * dn_albedo(al.z);
        }
    }
    ((float4 *)a.dst)[p] = make_float4(ox, oy, oz, cp.w);
    if (a.rgba8) a.rgba8[p] = rgba8(ox, oy, oz, a.srgb_pow != 0u);
}

template <bool NRM, bool DEP, bool COL>
__global__ __launch_bounds__(256) void denoise_direct_kernel(DenoiseArgs a) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    filter_pixel<NRM, DEP, COL>(a, DirectTaps{a}, x, y);
}

// blockIdx.x = rx * TUP + tile_u with TUP = gridDim.x / step, a multiple of 8, and blockIdx.y = tile_v * step + ry:
// a block's XCD is its linear index modulo 8 = tile_u modulo 8, so the step^2 classes of one tile's neighbourhood,
// which share every line they read, run on one XCD and meet in its L2 (blocks with tile_u past the image leave).
template <bool NRM, bool DEP, bool COL>
__global__ __launch_bounds__(256) void denoise_lds_kernel(DenoiseArgs a) {
    __shared__ float4 s_col[kDnLN];
    __shared__ uint2 s_hit[kDnLN];
    __shared__ float4 s_nrm[NRM ? kDnLN : 1];
    __shared__ float s_lum[COL ? kDnLN : 1];
    const int s = (int)a.step, w_img = (int)a.width, h_img = (int)a.height;
    const uint32_t tup = gridDim.x / a.step;
    const int rx = (int)(blockIdx.x / tup), ry = (int)(blockIdx.y % a.step);
    const int u0 = (int)(blockIdx.x % tup) * kDnTX, v0 = (int)(blockIdx.y / a.step) * kDnTY;
    if (rx + u0 * s >= w_img) return;  // (block-uniform, before the barrier: the padding of TUP)
    for (int e = (int)threadIdx.x; e < kDnLN; e += 256) {
        const int qx = rx + (u0 - kDnHalo + e % kDnLW) * s, qy = ry + (v0 - kDnHalo + e / kDnLW) * s;
        if (qx < 0 || qx >= w_img || qy < 0 || qy >= h_img) continue;  // (an entry outside the image is never read)
        const size_t q = (size_t)qy * a.width + (size_t)qx;
        const uint2 hq = ((const uint2 *)a.hit)[q];
        const float4 c = dn_load_colour(a, q);
        s_hit[e] = hq;
        s_col[e] = c;
        if (COL) s_lum[e] = dn_lum(c);
        if (NRM && hq.x != kDenoiseMiss) s_nrm[e] = ((const float4 *)a.normal)[q];  // (a miss's normal is never read)
    }
    __syncthreads();
    const int lu = (int)(threadIdx.x & 31u), lv = (int)(threadIdx.x >> 5);
    const int x = rx + (u0 + lu) * s, y = ry + (v0 + lv) * s;
    if (x >= w_img || y >= h_img) return;
    filter_pixel<NRM, DEP, COL>(a, LdsTaps{s_col, s_nrm, s_hit, s_lum, lu, lv}, (uint32_t)x, (uint32_t)y);
}

// Which shape runs a pass of this step.
static bool launch_lds(uint32_t step) {
#ifdef RTK_DENOISE_SHAPE
    (void)step;
    return RTK_DENOISE_SHAPE != 0;
#else
    return step <= 8u;
#endif
}

template <bool NRM, bool DEP, bool COL>
static void launch_pass(const DenoiseArgs &a, hipStream_t stream) {
    if (launch_lds(a.step)) {
        // pixels of one residue class along x and y (the largest class), in tiles, times the classes
        const uint32_t nu = (a.width + a.step - 1u) / a.step, nv = (a.height + a.step - 1u) / a.step;
        const uint32_t tup = ((nu + kDnTX - 1u) / kDnTX + 7u) & ~7u;
        const dim3 grid(tup * a.step, (nv + kDnTY - 1u) / kDnTY * a.step);
        hipLaunchKernelGGL((denoise_lds_kernel<NRM, DEP, COL>), grid, dim3(256), 0, stream, a);
    } else {
        const dim3 grid((a.width + 63u) / 64u, (a.height + 3u) / 4u);
        hipLaunchKernelGGL((denoise_direct_kernel<NRM, DEP, COL>), grid, dim3(256), 0, stream, a);
    }
}

}  // namespace rtk

extern "C" int rtk_launch_denoise_pass(const DenoiseArgs *a, hipStream_t stream) {
    if (a->width == 0u || a->height == 0u || a->step == 0u) return -1;
    switch ((a->normal_power != 0u ? 4 : 0) | (a->sigma_depth > 0.0f ? 2 : 0) | (a->ic > 0.0f ? 1 : 0)) {
        case 0: rtk::launch_pass<false, false, false>(*a, stream); break;
        case 1: rtk::launch_pass<false, false, true>(*a, stream); break;
        case 2: rtk::launch_pass<false, true, false>(*a, stream); break;
        case 3: rtk::launch_pass<false, true, true>(*a, stream); break;
        case 4: rtk::launch_pass<true, false, false>(*a, stream); break;
        case 5: rtk::launch_pass<true, false, true>(*a, stream); break;
        case 6: rtk::launch_pass<true, true, false>(*a, stream); break;
        default: rtk::launch_pass<true, true, true>(*a, stream); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
