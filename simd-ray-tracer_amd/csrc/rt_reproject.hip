// rt_reproject.hip — rt_reproject: the running mean carried across a camera move (the pass is defined, operation
// by operation, in rt_trace.h).  One thread per pixel of the new frame, 64 x 4 pixels per block as
// denoise_direct_kernel has them: the pixel's surface point is projected into the previous frame, up to four
// history pixels around it that saw the same sphere at a consistent distance are gathered, and the fresh mean is
// folded into their weighted mean.  A reprojection is locally close to a translation, so the lanes of a wave,
// neighbours in x, read neighbouring history pixels: each tap is a few cache lines per wave, and nothing is staged
// in LDS.  Every operation is one f32 operation in the stated order (-ffp-contract=off, the compiler's IEEE
// division and square root; the direction is rtk_math.h's normalize, start_sample's own), so the kernel and the
// numpy restatement (tests/reproject_ref.py) give the same bits.
//
// rt_reproject_clip is the same pass with one step more: before the fold the gathered history colour is clamped,
// per channel, to mean +- Gamma * sigma of the fresh frame's pixels of the same sphere in a (2R + 1)^2 window
// (variance clipping; rt_trace.h states it operation by operation, tests/reproject_clip_ref.py restates it).  Both
// calls run reproject_pixel, so steps 1 to 8 are one piece of code; the clamp is a functor the fold calls, empty in
// reproject_kernel.  reproject_clip_kernel takes 32 x 8 pixels per block and loads the (32 + 2R) x (8 + 2R) tile of
// Mean.xyz and Hit.Key once into LDS, 16 B per entry (8.3 KB at R = 3); every tap of the window reads LDS.  Every
// thread reaches the barrier, whatever its own pixel is; an entry outside the image holds a NaN colour and
// RT_HIT_MISS, and is not read either (the tap loop tests the image's bounds).  A shape with one thread per pixel and
// every tap a global load was built beside it and lost at every radius (profiles/reproject_clip_ab.txt).
#include "rtk_math.h"

namespace rtk {

constexpr uint32_t kReprojectMiss = 0xFFFFFFFFu;  // RT_HIT_MISS

__device__ __forceinline__ bool rp_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e+38f; }  // (a NaN fails)

// The clamp of rt_reproject: none.
struct NoClip {
    __device__ __forceinline__ void operator()(uint32_t, float &, float &, float &) const {}
};

// Steps 1 to 8 for the pixel (x, y) inside the image, p its index, m = Mean[p] and hp = Hit[p] (the caller loads
// them: reproject_clip_kernel does so before its barrier).  `clip(kp, hx, hy, hz)` runs on the gathered history
// colour of a pixel that kept at least one tap, between H = acc / ws and the fold.
template <class Clip>
__device__ __forceinline__ void reproject_pixel(const ReprojectArgs &a, uint32_t x, uint32_t y, size_t p, const float4 &m,
                                                const uint2 &hp, const Clip &clip) {
    const uint32_t kp = hp.x;
    float ox = m.x, oy = m.y, oz = m.z;  // fresh: the mean itself
    uint32_t count = a.frames;
    if (a.history != nullptr && kp != kReprojectMiss) {
        const float tp = __uint_as_float(hp.y);
        // the pixel-centre primary direction, as start_sample<true> forms it
        const float fx = -1.0f + ((float)x * 2.0f) / a.wf;
        const float fy = -1.0f + ((float)y * 2.0f) / a.hf;
        const float kx = (fx * a.film_w) * 0.5f;
        const float ky = (fy * a.film_h) * 0.5f;
        float dx = ((a.film_center[0] + kx * a.cam_x[0]) + ky * a.cam_y[0]) - a.cam_pos[0];
        float dy = ((a.film_center[1] + kx * a.cam_x[1]) + ky * a.cam_y[1]) - a.cam_pos[1];
        float dz = ((a.film_center[2] + kx * a.cam_x[2]) + ky * a.cam_y[2]) - a.cam_pos[2];
        normalize(dx, dy, dz);
        // the surface point, seen from the previous camera
        const float vx = (a.cam_pos[0] + dx * tp) - a.prev_pos[0];
        const float vy = (a.cam_pos[1] + dy * tp) - a.prev_pos[1];
        const float vz = (a.cam_pos[2] + dz * tp) - a.prev_pos[2];
        const float u = dot3(vx, vy, vz, a.prev_x[0], a.prev_x[1], a.prev_x[2]);
        const float v = dot3(vx, vy, vz, a.prev_y[0], a.prev_y[1], a.prev_y[2]);
        const float d = dot3(vx, vy, vz, a.fv[0], a.fv[1], a.fv[2]);
        const float qx = (u / d) * a.ff, qy = (v / d) * a.ff;
        const float sx = (((qx * 2.0f) / a.prev_film_w) + 1.0f) * a.hw;
        const float sy = (((qy * 2.0f) / a.prev_film_h) + 1.0f) * a.hh;
        // (written so that a NaN fails; inside, floorf(sx) is in [-1, Width - 1]: the conversion below is safe)
        if (d > 0.0f && sx >= -1.0f && sx < a.wf && sy >= -1.0f && sy < a.hf) {
            const float te = __builtin_sqrtf(dot3(vx, vy, vz, vx, vy, vz));
            const float lim = a.depth_tolerance * te;
            const float fx0 = __builtin_floorf(sx), fy0 = __builtin_floorf(sy);
            const float ax = sx - fx0, ay = sy - fy0;
            const int x0 = (int)fx0, y0 = (int)fy0;
            const int w_img = (int)a.width, h_img = (int)a.height;
            float accx = 0.0f, accy = 0.0f, accz = 0.0f, ws = 0.0f;
            uint32_t n = 0xFFFFFFFFu;
            bool kept = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qxi = x0 + (i & 1), qyi = y0 + (i >> 1);
                if (qxi < 0 || qxi >= w_img || qyi < 0 || qyi >= h_img) continue;
                const float w = ((i & 1) ? ax : 1.0f - ax) * ((i >> 1) ? ay : 1.0f - ay);
                if (!(w > 0.0f)) continue;
                const size_t q = (size_t)qyi * a.width + (size_t)qxi;
                const uint32_t nq = a.history_count[q];
                if (nq == 0u) continue;
                const uint2 hq = ((const uint2 *)a.history_hit)[q];
                if (hq.x != kp) continue;
                if (a.depth_tolerance > 0.0f && !(__builtin_fabsf(te - __uint_as_float(hq.y)) <= lim)) continue;
                const float4 c = ((const float4 *)a.history)[q];
                if (!(rp_finite(c.x) && rp_finite(c.y) && rp_finite(c.z))) continue;
                accx = accx + w * c.x;
                accy = accy + w * c.y;
                accz = accz + w * c.z;
                ws = ws + w;
                n = nq < n ? nq : n;
                kept = true;
            }
            if (kept) {
                n = n < a.max_history ? n : a.max_history;
                float hx = accx / ws, hy = accy / ws, hz = accz / ws;
                clip(kp, hx, hy, hz);
                const float fr = (float)a.frames;
                const float al = fr / ((float)n + fr);
                ox = hx + (m.x - hx) * al;
                oy = hy + (m.y - hy) * al;
                oz = hz + (m.z - hz) * al;
                const uint32_t room = a.max_history - n;  // (n + Frames without wrapping)
                count = a.frames < room ? n + a.frames : a.max_history;
            }
        }
    }
    ((float4 *)a.out)[p] = make_float4(ox, oy, oz, m.w);
    a.out_count[p] = count;
    if (a.rgba8) a.rgba8[p] = rgba8(ox, oy, oz, a.srgb_pow != 0u);
}

__global__ __launch_bounds__(256) void reproject_kernel(ReprojectArgs a) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    reproject_pixel(a, x, y, p, ((const float4 *)a.mean)[p], ((const uint2 *)a.hit)[p], NoClip{});
}

// ------------------------------------------------- rt_reproject_clip
constexpr int kClipTX = 32, kClipTY = 8;  // pixels per block

__device__ __forceinline__ float rp_pos(float v) { return v > 0.0f ? v : 0.0f; }  // rt_denoise's pos (a NaN gives 0)

// The new step for the pixel (x, y) at (lu, lv) of the block's LDS tile of (Mean.xyz, Hit.Key): the sums over the
// window in the stated order, the band, the clamp by comparisons (a NaN bound clamps nothing).
template <int R>
struct ClipHistory {
    const float4 *tile;
    float gamma;
    int x, y, lu, lv, w_img, h_img;
    __device__ __forceinline__ void operator()(uint32_t kp, float &hx, float &hy, float &hz) const {
        float s1x = 0.0f, s1y = 0.0f, s1z = 0.0f, s2x = 0.0f, s2y = 0.0f, s2z = 0.0f, nf = 0.0f;
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= h_img) continue;
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= w_img) continue;
                const float4 c = tile[(lv + R + dy) * (kClipTX + 2 * R) + lu + R + dx];
                if (__float_as_uint(c.w) != kp) continue;
                if (!(rp_finite(c.x) && rp_finite(c.y) && rp_finite(c.z))) continue;
                s1x = s1x + c.x;
                s1y = s1y + c.y;
                s1z = s1z + c.z;
                s2x = s2x + c.x * c.x;
                s2y = s2y + c.y * c.y;
                s2z = s2z + c.z * c.z;
                nf = nf + 1.0f;
            }
        }
        if (nf > 0.0f) {
            clamp(s1x, s2x, nf, hx);
            clamp(s1y, s2y, nf, hy);
            clamp(s1z, s2z, nf, hz);
        }
    }
    __device__ __forceinline__ void clamp(float s1, float s2, float nf, float &hc) const {
        const float m = s1 / nf;
        const float sd = __builtin_sqrtf(rp_pos(s2 / nf - m * m));
        const float lo = m - gamma * sd, hi = m + gamma * sd;
        if (hc < lo) hc = lo;
        if (hc > hi) hc = hi;
    }
};

template <int R>
__global__ __launch_bounds__(256) void reproject_clip_kernel(ReprojectClipArgs c) {
    constexpr int LW = kClipTX + 2 * R, LH = kClipTY + 2 * R, LN = LW * LH;
    __shared__ float4 s_tile[LN];
    const int w_img = (int)c.rp.width, h_img = (int)c.rp.height;
    const int x0 = (int)blockIdx.x * kClipTX, y0 = (int)blockIdx.y * kClipTY;
    const int lu = (int)(threadIdx.x & 31u), lv = (int)(threadIdx.x >> 5);
    const int x = x0 + lu, y = y0 + lv;
    const bool inside = x < w_img && y < h_img;
    // the thread's own pixel first, so that its loads are under way while the tile is filled
    const size_t p = inside ? (size_t)y * c.rp.width + (size_t)x : 0u;
    float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint2 hp = make_uint2(kReprojectMiss, 0u);
    if (inside) {
        m = ((const float4 *)c.rp.mean)[p];
        hp = ((const uint2 *)c.rp.hit)[p];
    }
    // Every thread of the block comes here and to the barrier: misses, fresh pixels and threads outside the image
    // too.  (Without a history no pixel reaches the clamp and the tile is not filled: the condition is the block's.)
    if (c.rp.history != nullptr) {
        for (int e = (int)threadIdx.x; e < LN; e += 256) {
            const int qx = x0 - R + e % LW, qy = y0 - R + e / LW;
            // outside the image: a key no pixel that reaches the clamp has, and a colour the finiteness rule drops
            float4 v = make_float4(__uint_as_float(0x7FC00000u), 0.0f, 0.0f, __uint_as_float(kReprojectMiss));
            if (qx >= 0 && qx < w_img && qy >= 0 && qy < h_img) {
                const size_t q = (size_t)qy * c.rp.width + (size_t)qx;
                v = ((const float4 *)c.rp.mean)[q];
                v.w = __uint_as_float(((const uint32_t *)c.rp.hit)[2u * q]);
            }
            s_tile[e] = v;
        }
    }
    __syncthreads();
    if (!inside) return;
    reproject_pixel(c.rp, (uint32_t)x, (uint32_t)y, p, m, hp, ClipHistory<R>{s_tile, c.gamma, x, y, lu, lv, w_img, h_img});
}

template <int R>
static void launch_clip(const ReprojectClipArgs &c, hipStream_t stream) {
    const dim3 grid((c.rp.width + kClipTX - 1u) / kClipTX, (c.rp.height + kClipTY - 1u) / kClipTY);
    hipLaunchKernelGGL(reproject_clip_kernel<R>, grid, dim3(256), 0, stream, c);
}

}  // namespace rtk

extern "C" int rtk_launch_reproject(const ReprojectArgs *a, hipStream_t stream) {
    if (a->width == 0u || a->height == 0u) return -1;
    const dim3 grid((a->width + 63u) / 64u, (a->height + 3u) / 4u);
    hipLaunchKernelGGL(rtk::reproject_kernel, grid, dim3(256), 0, stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int rtk_launch_reproject_clip(const ReprojectClipArgs *c, hipStream_t stream) {
    if (c->rp.width == 0u || c->rp.height == 0u) return -1;
    switch (c->radius) {
        case 1: rtk::launch_clip<1>(*c, stream); break;
        case 2: rtk::launch_clip<2>(*c, stream); break;
        case 3: rtk::launch_clip<3>(*c, stream); break;
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
