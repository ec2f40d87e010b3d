// TEST-ONLY: the walk layer of csrc/rtk_walk.h, one function or one small family per entry point.
// This file includes the header itself and holds no copy of anything under test; it is built with
// the kernel translation units' own flags (simd-ray-tracer_amd/Makefile, target walk_probe) into
// tests/walk_probe/libwalk_probe.so, which is never linked into librt_trace.so.
// tests/walk_probe.py loads it; tests/walk_ref.py holds the references, tests/test_gpu_walk_layer.py the cases.
//
// Every entry point takes DEVICE pointers, counts and a stream, launches one kernel and returns 0, or
// -1 for a NULL pointer and -4 for a failed launch (hipGetLastError).  The caller allocates every buffer
// (with guard words behind the outputs), synchronises and reads back.
//
// Kernels: a 1-D grid of 256-thread blocks, one ray per lane: rays[6 i ..] = {Ox, Oy, Oz, Dx, Dy, Dz}.
// The sphere operands of the packed tests are SGPR operands of their asm, so every kernel reads them from
// a table through an index that is the same in every lane, in a uniform loop over pairs, groups or entries
// (the table through the constant address space, as the walks read theirs).  The lanes past the count n
// come in two forms (`early`):
//   0  they compute on the clamped index n - 1 and store nothing: full exec everywhere;
//   1  they return first: every ballot, compare mask and packed op of the last wave runs under partial exec.
// Outputs are entry-major: word w of lane i for table entry p is out[(p n + i) W + w].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtk_walk.h"

namespace {

using namespace rtk;

constexpr uint32_t kBlock = 256;
typedef const __attribute__((address_space(4))) uint32_t cu32_t;

// (EARLY lanes have returned already; the others clamp)
#define WALK_PROBE_LANE()                                       \
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;       \
    if (EARLY && i >= n) return;                                \
    const bool store = i < n;                                   \
    const uint32_t j = store ? i : n - 1u

__device__ __forceinline__ RayPk load_ray(const float *rays, uint32_t j) {
    const float *r = rays + 6ull * j;
    return {f2{r[0], r[3]}, f2{r[1], r[4]}, f2{r[2], r[5]}};
}

__device__ __forceinline__ Sample as_sample(const RayPk &r) {
    Sample p = {};
    p.rx = r.x, p.ry = r.y, p.rz = r.z;
    return p;
}

__device__ __forceinline__ void store_hit(uint32_t *out, uint32_t i, const Hit &h) {
    uint32_t *o = out + 9ull * i;
    o[0] = __float_as_uint(h.t0), o[1] = __float_as_uint(h.t1), o[2] = __float_as_uint(h.t2), o[3] = __float_as_uint(h.t3);
    o[4] = h.k0, o[5] = h.k1, o[6] = h.k2, o[7] = h.k3;
    o[8] = h.ins;
}

// pairs: two rows per sphere pair, {x0, x1, y0, y1} and {z0, z1, -, -}; for which == 2 the rows hold
// C = RN(S - O) of the launch's common origin.  out: {T0, T1, dist0, dist1} per (pair, lane).
template <bool EARLY>
__global__ void __launch_bounds__(kBlock) k_exact(const float *rays, uint32_t n, const float4 *pairs, uint32_t n_pairs,
                                                  uint32_t which, float *out) {
    WALK_PROBE_LANE();
    const RayPk r = load_ray(rays, j);
    cv4f_t *tab = (cv4f_t *)pairs;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        const v4f_t a = tab[2u * p], b = tab[2u * p + 1u];
        f2 T, d;
        if (which == 0u) {
            const Sample s = as_sample(r);
            float T0, T1, d0, d1;
            sphere_core(s, a.x, a.z, b.x, T0, d0);
            sphere_core(s, a.y, a.w, b.y, T1, d1);
            T = f2{T0, T1}, d = f2{d0, d1};
        } else if (which == 1u) {
            d = pair_dist(r, f2{a.x, a.y}, f2{a.z, a.w}, f2{b.x, b.y}, T);
        } else {
            d = pair_dist_c(r, f2{a.x, a.y}, f2{a.z, a.w}, f2{b.x, b.y}, T);
        }
        if (store) {
            float *o = out + 4ull * ((uint64_t)p * n + i);
            o[0] = T.x, o[1] = T.y, o[2] = d.x, o[3] = d.y;
        }
    }
}

// steps: {T, dist, r2} of lane i's step s at steps[3 (s n + i)]; step s goes to class s & 3 of group
// gids[s >> 2] where the rule set's hit test passes.  out: the lane's Hit, nine words.
template <bool SIMD, bool EARLY>
__global__ void __launch_bounds__(kBlock) k_candidate(const float *steps, const uint32_t *gids, uint32_t n,
                                                      uint32_t n_gsteps, uint32_t fast, uint32_t *out) {
    WALK_PROBE_LANE();
    Hit h;
    hit_reset(h);
    cu32_t *gt = (cu32_t *)gids;
    const bool fs = fast != 0u;
    for (uint32_t gs = 0; gs < n_gsteps; ++gs) {
        const uint32_t g = gt[gs];
        const float *s0 = steps + 3ull * ((uint64_t)(4u * gs) * n + j);
        const uint64_t stride = 3ull * n;
        const float *s1 = s0 + stride, *s2 = s1 + stride, *s3 = s2 + stride;
        const bool h0 = SIMD ? s0[1] < s0[2] : !(s0[1] > s0[2]);
        const bool h1 = SIMD ? s1[1] < s1[2] : !(s1[1] > s1[2]);
        const bool h2 = SIMD ? s2[1] < s2[2] : !(s2[1] > s2[2]);
        const bool h3 = SIMD ? s3[1] < s3[2] : !(s3[1] > s3[2]);
        if (h0) candidate<SIMD, 0>(h, g, s0[0], s0[1], s0[2], fs);
        if (h1) candidate<SIMD, 1>(h, g, s1[0], s1[1], s1[2], fs);
        if (h2) candidate<SIMD, 2>(h, g, s2[0], s2[1], s2[2], fs);
        if (h3) candidate<SIMD, 3>(h, g, s3[0], s3[1], s3[2], fs);
    }
    if (store) store_hit(out, i, h);
}

// groups: n_groups records of kGroupF4 rows as the host packs them; prim: kPrimF4 rows per group of the
// launch's common origin (variant 6 only).  variant: 0 test_group; 1-4 recheck_pairs with
// (f01, f23) = (variant - 1) & 1, (variant - 1) & 2; 5 test_group_pf<., false, rel>; 6 test_pair_prim
// over every pair in ascending order.  out: the lane's Hit.
template <bool SIMD, bool EARLY>
__global__ void __launch_bounds__(kBlock) k_group(const float *rays, uint32_t n, const float4 *groups, uint32_t n_groups,
                                                  uint32_t n_spheres, const float4 *prim, uint32_t variant, uint32_t fast,
                                                  uint32_t rel, uint32_t *out) {
    WALK_PROBE_LANE();
    const RayPk r = load_ray(rays, j);
    TraceArgs a = {};
    a.groups = groups;
    a.n_groups = n_groups;
    a.n_spheres = n_spheres;
    Hit h;
    hit_reset(h);
    const bool fs = fast != 0u;
    cv4f_t *gp = (cv4f_t *)groups;
    if (variant == 6u) {
        for (uint32_t pr = 0; pr < 2u * n_groups; ++pr) test_pair_prim<SIMD>(a, (cv4f_t *)prim, pr, r, h, fs);
    } else {
        for (uint32_t g = 0; g < n_groups; ++g) {
            const Group G = load_group_at(gp + kGroupF4 * g);
            if (variant == 0u) {
                test_group<SIMD>(a, G, g, r, h, fs, nullptr);
            } else if (variant <= 4u) {
                const uint32_t f = variant - 1u;
                recheck_pairs<SIMD>(a, G, g, r, h, fs, (f & 1u) != 0u, (f & 2u) != 0u);
            } else if (rel) {
                test_group_pf<SIMD, false, true>(a, nullptr, G, g, r, h, fs);
            } else {
                test_group_pf<SIMD, false, false>(a, nullptr, G, g, r, h, fs);
            }
        }
    }
    if (store) store_hit(out, i, h);
}

// pairs as k_exact's.  out: {e0, e1, T0, T1, cc0, cc1} per (pair, lane).
template <bool EARLY>
__global__ void __launch_bounds__(kBlock) k_prefilter(const float *rays, uint32_t n, const float4 *pairs, uint32_t n_pairs,
                                                      float *out) {
    WALK_PROBE_LANE();
    const RayPk r = load_ray(rays, j);
    cv4f_t *tab = (cv4f_t *)pairs;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        const v4f_t a = tab[2u * p], b = tab[2u * p + 1u];
        f2 T, cc;
        const f2 e = pair_prefilter(r, f2{a.x, a.y}, f2{a.z, a.w}, f2{b.x, b.y}, T, cc);
        if (store) {
            float *o = out + 6ull * ((uint64_t)p * n + i);
            o[0] = e.x, o[1] = e.y, o[2] = T.x, o[3] = T.y, o[4] = cc.x, o[5] = cc.y;
        }
    }
}

// out: f01 | f23 << 1 per (group, lane)
template <bool REL, bool EARLY>
__global__ void __launch_bounds__(kBlock) k_prefilter_group(const float *rays, uint32_t n, const float4 *groups,
                                                            uint32_t n_groups, uint32_t *out) {
    WALK_PROBE_LANE();
    const RayPk r = load_ray(rays, j);
    cv4f_t *gp = (cv4f_t *)groups;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const Group G = load_group_at(gp + kGroupF4 * g);
        bool f01, f23;
        prefilter_group<REL>(G, r, f01, f23);
        if (store) out[(uint64_t)g * n + i] = (f01 ? 1u : 0u) | (f23 ? 2u : 0u);
    }
}

// c0: one row {c0x, c0y, c0z, -}.  out: RayX, eight floats {x.x, x.y, y.x, y.y, z.x, z.y, w.x, w.y} per lane.
template <bool EARLY>
__global__ void __launch_bounds__(kBlock) k_expand(const float *rays, uint32_t n, const float4 *c0, float *out) {
    WALK_PROBE_LANE();
    const RayPk r = load_ray(rays, j);
    const RayX x = ray_expand(r, *(cv4f_t *)c0);
    if (store) {
        float *o = out + 8ull * i;
        o[0] = x.x.x, o[1] = x.x.y, o[2] = x.y.x, o[3] = x.y.y, o[4] = x.z.x, o[5] = x.z.y, o[6] = x.w.x, o[7] = x.w.y;
    }
}

// pairs as k_exact's, of the recentred table.  out: {e'0, e'1, T0, T1} per (pair, lane).
template <bool EARLY>
__global__ void __launch_bounds__(kBlock) k_prefilter_x(const float *rays, uint32_t n, const float4 *c0, const float4 *pairs,
                                                        uint32_t n_pairs, float *out) {
    WALK_PROBE_LANE();
    const RayPk r = load_ray(rays, j);
    const RayX x = ray_expand(r, *(cv4f_t *)c0);
    cv4f_t *tab = (cv4f_t *)pairs;
    for (uint32_t p = 0; p < n_pairs; ++p) {
        const v4f_t a = tab[2u * p], b = tab[2u * p + 1u];
        f2 T;
        const f2 e = pair_prefilter_x(x, f2{a.x, a.y}, f2{a.z, a.w}, f2{b.x, b.y}, T);
        if (store) {
            float *o = out + 4ull * ((uint64_t)p * n + i);
            o[0] = e.x, o[1] = e.y, o[2] = T.x, o[3] = T.y;
        }
    }
}

// cct: {cc0, cc1, T0, T1} per lane.  entries: three rows each, {r0, r1, beta0, beta1},
// {srho0, srho1, ymid0, ymid1}, {yhalf0, yhalf1, -, -}.  ClConst as clustered_groups builds it.
// out per (entry, lane): member_thr t (2), cluster_thr t (2) and b (2), cluster_slab d (2) and thr (2).
template <bool EARLY>
__global__ void __launch_bounds__(kBlock) k_thresholds(const float *rays, const float *cct, uint32_t n, const float4 *entries,
                                                       uint32_t n_entries, float *out) {
    WALK_PROBE_LANE();
    const RayPk r = load_ray(rays, j);
    const float *c = cct + 4ull * j;
    const f2 cc = {c[0], c[1]}, T = {c[2], c[3]};
    const float oy = r.y.x, dy = r.y.y;
    const float slab_e0 = __builtin_fmaf(__builtin_fabsf(oy), 0x1p-21f, kSlabRel);
    ClConst k;
    k.kc = f2{walk_const(kClRel), walk_const(kBehindRel)};
    k.kp = f2{walk_const(kPfRel), walk_const(kSlabRel)};
    k.aux = f2{slab_e0, __builtin_fabsf(dy)};
    cv4f_t *tab = (cv4f_t *)entries;
    for (uint32_t e = 0; e < n_entries; ++e) {
        const v4f_t r0 = tab[3u * e], r1 = tab[3u * e + 1u], r2 = tab[3u * e + 2u];
        const f2 tm = member_thr(cc, k, f2{r0.x, r0.y});
        f2 tc, b, d, thr;
        cluster_thr(cc, k, f2{r0.x, r0.y}, f2{r0.z, r0.w}, tc, b);
        cluster_slab(cc, T, r, k, f2{r1.x, r1.y}, f2{r1.z, r1.w}, f2{r2.x, r2.y}, d, thr);
        if (store) {
            float *o = out + 10ull * ((uint64_t)e * n + i);
            o[0] = tm.x, o[1] = tm.y, o[2] = tc.x, o[3] = tc.y, o[4] = b.x, o[5] = b.y;
            o[6] = d.x, o[7] = d.y, o[8] = thr.x, o[9] = thr.y;
        }
    }
}

// sc: {Sx, Sy, Sz, rho} per lane; slot per lane.  out: {own_sphere(p, sc, slot), origin_near(p, sc)} per lane.
template <bool EARLY>
__global__ void __launch_bounds__(kBlock) k_own(const float *rays, const float4 *sc, const uint32_t *slot, uint32_t n,
                                                uint32_t *out) {
    WALK_PROBE_LANE();
    const Sample p = as_sample(load_ray(rays, j));
    const float4 s = sc[j];
    const uint32_t own = own_sphere(p, s, slot[j]);
    const bool near = origin_near(p, s);
    if (store) out[2ull * i] = own, out[2ull * i + 1u] = near ? 1u : 0u;
}

inline dim3 grid_of(uint32_t n) { return dim3((n + kBlock - 1u) / kBlock); }
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -4; }

}  // namespace

#define WALK_PROBE_LAUNCH(kernel_early, kernel_clamp, ...)                                            \
    do {                                                                                              \
        if (n == 0u) return 0;                                                                        \
        if (early) hipLaunchKernelGGL(kernel_early, grid_of(n), dim3(kBlock), 0, stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(kernel_clamp, grid_of(n), dim3(kBlock), 0, stream, __VA_ARGS__);      \
        return launched();                                                                            \
    } while (0)

extern "C" int walk_probe_exact(const float *rays, uint32_t n, const float4 *pairs, uint32_t n_pairs, uint32_t which,
                                int early, float *out, hipStream_t stream) {
    if (!rays || !pairs || !out || which > 2u) return -1;
    WALK_PROBE_LAUNCH(k_exact<true>, k_exact<false>, rays, n, pairs, n_pairs, which, out);
}

extern "C" int walk_probe_candidate(const float *steps, const uint32_t *gids, uint32_t n, uint32_t n_gsteps, int simd, int fast,
                                    int early, uint32_t *out, hipStream_t stream) {
    if (!steps || !gids || !out) return -1;
    const uint32_t fs = fast ? 1u : 0u;
    if (simd) WALK_PROBE_LAUNCH((k_candidate<true, true>), (k_candidate<true, false>), steps, gids, n, n_gsteps, fs, out);
    WALK_PROBE_LAUNCH((k_candidate<false, true>), (k_candidate<false, false>), steps, gids, n, n_gsteps, fs, out);
}

extern "C" int walk_probe_group(const float *rays, uint32_t n, const float4 *groups, uint32_t n_groups, uint32_t n_spheres,
                                const float4 *prim, uint32_t variant, int simd, int fast, int rel, int early, uint32_t *out,
                                hipStream_t stream) {
    if (!rays || !groups || !out || variant > 6u || (variant == 6u && !prim)) return -1;
    const uint32_t fs = fast ? 1u : 0u, rl = rel ? 1u : 0u;
    if (simd)
        WALK_PROBE_LAUNCH((k_group<true, true>), (k_group<true, false>), rays, n, groups, n_groups, n_spheres, prim, variant,
                          fs, rl, out);
    WALK_PROBE_LAUNCH((k_group<false, true>), (k_group<false, false>), rays, n, groups, n_groups, n_spheres, prim, variant, fs,
                      rl, out);
}

extern "C" int walk_probe_prefilter(const float *rays, uint32_t n, const float4 *pairs, uint32_t n_pairs, int early, float *out,
                                    hipStream_t stream) {
    if (!rays || !pairs || !out) return -1;
    WALK_PROBE_LAUNCH(k_prefilter<true>, k_prefilter<false>, rays, n, pairs, n_pairs, out);
}

extern "C" int walk_probe_prefilter_group(const float *rays, uint32_t n, const float4 *groups, uint32_t n_groups, int rel,
                                          int early, uint32_t *out, hipStream_t stream) {
    if (!rays || !groups || !out) return -1;
    if (rel) WALK_PROBE_LAUNCH((k_prefilter_group<true, true>), (k_prefilter_group<true, false>), rays, n, groups, n_groups, out);
    WALK_PROBE_LAUNCH((k_prefilter_group<false, true>), (k_prefilter_group<false, false>), rays, n, groups, n_groups, out);
}

extern "C" int walk_probe_expand(const float *rays, uint32_t n, const float4 *c0, int early, float *out, hipStream_t stream) {
    if (!rays || !c0 || !out) return -1;
    WALK_PROBE_LAUNCH(k_expand<true>, k_expand<false>, rays, n, c0, out);
}

extern "C" int walk_probe_prefilter_x(const float *rays, uint32_t n, const float4 *c0, const float4 *pairs, uint32_t n_pairs,
                                      int early, float *out, hipStream_t stream) {
    if (!rays || !c0 || !pairs || !out) return -1;
    WALK_PROBE_LAUNCH(k_prefilter_x<true>, k_prefilter_x<false>, rays, n, c0, pairs, n_pairs, out);
}

extern "C" int walk_probe_thresholds(const float *rays, const float *cct, uint32_t n, const float4 *entries, uint32_t n_entries,
                                     int early, float *out, hipStream_t stream) {
    if (!rays || !cct || !entries || !out) return -1;
    WALK_PROBE_LAUNCH(k_thresholds<true>, k_thresholds<false>, rays, cct, n, entries, n_entries, out);
}

extern "C" int walk_probe_own(const float *rays, const float4 *sc, const uint32_t *slot, uint32_t n, int early, uint32_t *out,
                              hipStream_t stream) {
    if (!rays || !sc || !slot || !out) return -1;
    WALK_PROBE_LAUNCH(k_own<true>, k_own<false>, rays, sc, slot, n, out);
}
