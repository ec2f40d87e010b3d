// rtk_cull.h — the primary-ray cone test and the tile selection, shared by the cull pass
// (rt_sched.hip cull_kernel) and the first-hit pass (rt_first_hit.hip), which culls inside its kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernel.h"
#include "rtk_shape.h"

namespace rtk {

// Conservative per-wave culling for primary rays.  All primary rays of a
// tile start at CameraPosition and point into the tile's film rectangle
// (+-0.5 px jitter), i.e. inside a cone (axis A, half-angle theta).  A sphere
// can pass the exact test d < r^2 only if the LINE through the camera along
// some cone direction comes within r of its centre, i.e. if the angle between
// +-C and A is below theta + asin(r/|C|).  The cone and the test are computed
// in f64, so their own rounding is negligible; the margins cover the f32 path
// the kernel actually traces: each traced direction lies within ~1e-6 rad of
// the ideal cone (film point and Normalize rounding; |jitter| <= 0.5 + 1e-7 px,
// covered by the 0.501 px bound), and the reference-rounded distance is within
// 13.3u|C|^2 of the exact one -- the test uses a 1e-5 rad
// angular margin and r'^2 = r^2 (1 + 1e-5) + 1e-5 |C|^2, ten times both.  A
// group it rejects is one every lane's exact test misses: skipping it changes
// nothing.
struct Cone {
    double ax, ay, az;     // axis
    double cos_t, sin_t;   // inflated half-angle
};

__device__ __forceinline__ Cone tile_cone(const TraceArgs &a, double u0, double u1, double v0, double v1) {
    const double fcx = (double)a.film_center[0] - a.cam_pos[0];
    const double fcy = (double)a.film_center[1] - a.cam_pos[1];
    const double fcz = (double)a.film_center[2] - a.cam_pos[2];
    const double aa[2] = {(-1.0 + (u0 * 2.0) / a.width) * a.film_w * 0.5, (-1.0 + (u1 * 2.0) / a.width) * a.film_w * 0.5};
    const double bb[2] = {(-1.0 + (v0 * 2.0) / a.height) * a.film_h * 0.5,
                          (-1.0 + (v1 * 2.0) / a.height) * a.film_h * 0.5};
    double cx[4], cy[4], cz[4];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double ka = aa[i & 1], kb = bb[i >> 1];
        const double x = fcx + ka * a.cam_x[0] + kb * a.cam_y[0];
        const double y = fcy + ka * a.cam_x[1] + kb * a.cam_y[1];
        const double z = fcz + ka * a.cam_x[2] + kb * a.cam_y[2];
        const double inv = 1.0 / __builtin_sqrt(x * x + y * y + z * z);
        cx[i] = x * inv;
        cy[i] = y * inv;
        cz[i] = z * inv;
        sx += cx[i];
        sy += cy[i];
        sz += cz[i];
    }
    Cone c;
    const double inv = 1.0 / __builtin_sqrt(sx * sx + sy * sy + sz * sz);
    c.ax = sx * inv;
    c.ay = sy * inv;
    c.az = sz * inv;
    double ct = 1.0;
    for (int i = 0; i < 4; ++i) ct = fmin(ct, c.ax * cx[i] + c.ay * cy[i] + c.az * cz[i]);
    const double st = __builtin_sqrt(fmax(0.0, 1.0 - ct * ct));
    const double cd = 0.99999999995, sd = 1e-5;  // cos/sin of the 1e-5 rad margin
    c.cos_t = ct * cd - st * sd;
    c.sin_t = st * cd + ct * sd;
    return c;
}

__device__ __forceinline__ bool cone_may_hit(const TraceArgs &a, const Cone &c, float px, float py, float pz, float r2) {
    if (!(r2 >= 0.0f)) return false;  // padding lanes of the scalar packing (-inf)
    const double qx = (double)px - a.cam_pos[0], qy = (double)py - a.cam_pos[1], qz = (double)pz - a.cam_pos[2];
    const double c2 = qx * qx + qy * qy + qz * qz;
    const double rr = (double)r2 * (1.0 + 1e-5) + 1e-5 * c2;
    if (rr >= c2) return true;  // the camera is (nearly) inside: never cull
    const double sb = __builtin_sqrt(rr / c2), cb = __builtin_sqrt(1.0 - rr / c2);
    if (c.cos_t <= 0.0) return true;  // cone wider than 90 degrees: no culling
    const double cos_lim = c.cos_t * cb - c.sin_t * sb;  // cos(theta + beta)
    const double cos_phi = fabs(c.ax * qx + c.ay * qy + c.az * qz) / __builtin_sqrt(c2);
    return cos_phi >= cos_lim - 1e-12;
}

// Primary-ray culling of one wave tile (TW x TH pixels at x0, ly0): bit p of
// the mask is set when some sphere of pair p (sphere slots 2p, 2p + 1: half
// p & 1 of group p >> 1) may pass some primary ray's exact test
// (cone_may_hit).  One sphere per lane, 64 per ballot, folded into one bit
// per pair; word w covers pairs 64w .. 64w+63 (spheres 128w .. 128w+127).
template <int P>
__device__ __forceinline__ uint64_t wave_tile_mask(const TraceArgs &a, const Cone &c, uint32_t w, uint32_t lane) {
    const float *gf = reinterpret_cast<const float *>(a.groups);
    uint64_t gm = 0;
    for (uint32_t q = 0; q < 2u && w * 128u + q * 64u < 4u * a.n_groups; ++q) {
        const uint32_t sph = w * 128u + q * 64u + lane;  // sphere slot 4*g + l
        bool cand = false;
        if (sph < 4u * a.n_groups) {
            const float *row = gf + (size_t)(sph >> 2) * (4u * kGroupF4) + (sph & 3u);
            cand = cone_may_hit(a, c, row[4u * kRowX], row[4u * kRowY], row[4u * kRowZ], row[4u * kRowR2]);
        }
        uint64_t m = __ballot(cand);
        m = (m | (m >> 1)) & 0x5555555555555555ull;  // bit 2i: some sphere of pair 32q + i
        m = (m | (m >> 1)) & 0x3333333333333333ull;  // compress the even bits into bits 0..31
        m = (m | (m >> 2)) & 0x0F0F0F0F0F0F0F0Full;
        m = (m | (m >> 4)) & 0x00FF00FF00FF00FFull;
        m = (m | (m >> 8)) & 0x0000FFFF0000FFFFull;
        m = (m | (m >> 16)) & 0x00000000FFFFFFFFull;
        gm |= m << (32u * q);
    }
    return gm;
}

// Tile selection (TraceArgs.sel, rt_trace_tiles): whether block tile (tile_x, tile_y) of launch
// shape P lies in a listed reference tile.  Block tiles divide the reference tile (rtk_shape.h),
// so its first pixel decides; that pixel is inside the image, so the bit exists.
template <int P>
__device__ __forceinline__ bool tile_selected(const TraceArgs &a, uint32_t tile_x, uint32_t tile_y) {
    if (!a.sel) return true;
    const uint32_t t = ((tile_y * 2u * Shape<P>::TH) / kRefTile) * a.sel_tiles_x + (tile_x * 2u * Shape<P>::TW) / kRefTile;
    return ((a.sel[t >> 5] >> (t & 31u)) & 1u) != 0u;
}

}  // namespace rtk
