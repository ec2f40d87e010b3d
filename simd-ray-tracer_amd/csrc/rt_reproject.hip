// rt_reproject.hip — rt_reproject: the running mean carried across a camera move (the pass is defined, operation
// by operation, in rt_trace.h).  One thread per pixel of the new frame, 64 x 4 pixels per block as
// denoise_direct_kernel has them: the pixel's surface point is projected into the previous frame, up to four
// history pixels around it that saw the same sphere at a consistent distance are gathered, and the fresh mean is
// folded into their weighted mean.  A reprojection is locally close to a translation, so the lanes of a wave,
// neighbours in x, read neighbouring history pixels: each tap is a few cache lines per wave, and nothing is staged
// in LDS.  Every operation is one f32 operation in the stated order (-ffp-contract=off, the compiler's IEEE
// division and square root; the direction is rtk_math.h's normalize, start_sample's own), so the kernel and the
// numpy restatement (tests/reproject_ref.py) give the same bits.
#include "rtk_math.h"

namespace rtk {

constexpr uint32_t kReprojectMiss = 0xFFFFFFFFu;  // RT_HIT_MISS

__device__ __forceinline__ bool rp_finite(float v) { return __builtin_fabsf(v) <= 3.402823466e+38f; }  // (a NaN fails)

__global__ __launch_bounds__(256) void reproject_kernel(ReprojectArgs a) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const float4 m = ((const float4 *)a.mean)[p];
    const uint2 hp = ((const uint2 *)a.hit)[p];
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
                const float hx = accx / ws, hy = accy / ws, hz = accz / ws;
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

}  // namespace rtk

extern "C" int rtk_launch_reproject(const ReprojectArgs *a, hipStream_t stream) {
    if (a->width == 0u || a->height == 0u) return -1;
    const dim3 grid((a->width + 63u) / 64u, (a->height + 3u) / 4u);
    hipLaunchKernelGGL(rtk::reproject_kernel, grid, dim3(256), 0, stream, *a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
