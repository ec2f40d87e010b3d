// rtk_math.h — the reference's lane math layer (x64_math.h, base.h:474-887) and
// the per-sample path state, restated for gfx950 device code: every function
// cites the reference lines it reproduces.
//
// Exactness: built with -ffp-contract=off (every op rounds separately, as the
// reference's SSE lane ops do), IEEE f32 denormals, correctly rounded sqrt and
// division (short verified sequences where their range is guaranteed); the
// one FMA the reference's -mfma build emits (Reflectance, main.cpp:299) is an
// explicit fmaf; rsqrtss is reproduced by table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernel.h"

namespace rtk {

constexpr float kEps = 1e-4f;   // base.h:889 F32Epsilon
constexpr float kFMax = 1e30f;  // base.h:891 F32Max
constexpr float kPfDirTol = 1.0f / 65536.0f;  // |1 - |D|^2| bound of the secondary prefilter (host: rt_pack.cpp)
// RandomFloat's (Max-Min)/(f64)(u32)-1 rounded to f32 (base.h:985), for the
// three ranges the path uses: (-0.5,0.5) and (0,1) -> 1, (-1,1) -> 2.
constexpr float kInvRange1 = (float)(1.0 / 4294967295.0);
constexpr float kInvRange2 = (float)(2.0 / 4294967295.0);

__device__ __forceinline__ uint32_t pcg(uint64_t &s) {  // base.h:954-963
    const uint64_t old = s;
    s = old * 6364136223846793005ULL + 1442695040888963407ULL;
    const uint32_t v = (uint32_t)(old >> 32) ^ (uint32_t)old;
    return __builtin_amdgcn_alignbit(v, v, (uint32_t)(old >> 59));  // RotateRight32
}

__device__ __forceinline__ float rand_float(uint64_t &s, float lo, float inv) {  // base.h:983-989
    const float r = (float)pcg(s) * inv;
    return r + lo;
}

__device__ __forceinline__ uint64_t seed_mix(uint64_t i) {  // main.cpp:668-675
    uint64_t s = 0x420247153476526ULL * i;
    s += 0x8442885C91A5C8DULL;
    s ^= s >> ((7u + i) % 64u);
    s ^= s << 23;
    s ^= s >> ((0x29u ^ i) % 64u);
    s = (s * 0x11C19226CEB4769AULL) + 0x1105404122082911ULL;
    s ^= s << 19;
    s ^= s >> 13;
    return s;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    const float px = ax * bx, py = ay * by, pz = az * bz;  // x64_math.h:224-227
    return (px + py) + pz;
}

// Short correctly rounded sequences.  tests/test_gpu_math_layer.py runs each of
// them, from this header, alone on the GPU (tests/math_probe) and holds it to the
// f64 result rounded once: rcp_rn and sqrt_rn on every mantissa of a binade or
// two and on 4,096 mantissas of every binade of their ranges, div_rn on 3.6e6
// edge-case and random pairs.  (When they were written, copies of them were
// compared with the compiler's IEEE sequence over every f32 of [2^-40, 2^40] /
// [2^-60, 2^60] and on 8.6e9 pairs: DESIGN.md, "Short exact sequences".)
// RN(1/b) for b in [2^-40, 2^40]: v_rcp_f32 (< 1 ulp) + one Newton step.
__device__ __forceinline__ float rcp_rn(float b) {
    const float y0 = __builtin_amdgcn_rcpf(b);
    return __builtin_fmaf(__builtin_fmaf(-b, y0, 1.0f), y0, y0);
}

// RN(sqrt(x)) for x = 0 or x in [2^-60, 2^60] (Markstein): y = v_rsq_f32(x),
// g = RN(x y), h = y / 2, r = x - g^2 (one fma, exact), result RN(g + r h).
// Held to the f64 sqrt rounded once by tests/test_gpu_math_layer.py, also from
// 2^-102 to the top of f32 (beyond what any caller needs: normalize takes len
// from the IEEE sqrt above 2^40).  x = +0: v_rsq gives +inf, clamped to 2^64 so
// g = 0 and the result is +0 (the range's y is below 2^30).
// Outside the domain it is NOT the IEEE sqrt: x < 0 gives -inf or a large
// negative value (v_rsq is NaN, the clamp's fminf turns it into 2^64; measured
// -inf on all of [-2^-10, -2^-25]), -inf gives -inf, and -0, +inf and NaN give
// NaN (-0: -inf * -0; +inf: v_rsq is +0, inf * 0).  The callers: normalize's x is
// a sum of squares, never negative or -0, and it sends a NaN len (x = +inf) to
// its IEEE path; linear_to_srgb's is in [0.0031308, 1] or NaN, and NaN stays NaN;
// shade's two uses are commented there; the candidate root (rtk_walk.h) is
// guarded by the host's proof (fast_sqrt).
// Five full-rate ops besides the transcendental, against eight for v_sqrt_f32
// and its two +-1 ulp residual tests (round 5's form): C2 +2.5 %, RTWeekend
// +2.3 % (profiles/r06q_sqrt_ab.txt).
__device__ __forceinline__ float sqrt_rn(float x) {
    const float y = __builtin_fminf(__builtin_amdgcn_rsqf(x), 0x1p64f);
    const float g = x * y, h = 0.5f * y;
    return __builtin_fmaf(__builtin_fmaf(-g, g, x), h, g);
}

// RN(a/b) from y = RN(1/b) (Markstein: q0 = a*y, exact residual, one fma
// correction) for b > 0 and a == +0 or |a/b| >= 2^-100 (no underflow in the
// residual).  a == -0 would come out +0: neither caller divides one (the film
// numerator is never -0; normalize sends any zero quotient to its IEEE path).
__device__ __forceinline__ float div_rn(float a, float b, float y) {
    const float q0 = a * y;
    return __builtin_fmaf(__builtin_fmaf(-q0, b, a), y, q0);
}

// The running-mean weights of the frame after pc folded ones (main.cpp:484-487):
// {RN(1 / (f32)(pc + 1)), RN((f32)pc / (f32)(pc + 1))}, the reference's f32
// divisions, by the short sequences: n = (f32)(pc + 1) is in [1, 2^32], inside
// rcp_rn's verified range, so RN(1/n) is rcp_rn(n) itself, and pc / n is +0 or
// >= 1/2 (div_rn's condition).  (The host keeps pc + 1 below 2^32: rt_trace.)
__device__ __forceinline__ float2 fold_weights(uint32_t pc) {
    const float n = (float)(pc + 1u);
    const float y = rcp_rn(n);
    return make_float2(y, div_rn((float)pc, n, y));
}

// v3::Normalize (x64_math.h:234-245): IEEE divide by the correctly rounded
// sqrt, zero when len^2 <= 1e-4.  Fast path: one reciprocal shared by the
// three quotients; lanes outside its proven range (a quotient below 2^-99,
// or len not a finite value up to 2^40: the test is !(len <= 2^40), so that the
// NaN sqrt_rn returns for len^2 = +inf, finite components from about 2^63.5,
// goes there too) take the compiler's IEEE sequence, square root included: the
// reference's len = +inf then gives quotients of +-0.  (The reciprocal from
// sqrt_rn's own v_rsq by a Newton step measured equal and was not kept:
// profiles/r06u_norm_rcp_and_c2_options_ab.txt.)
__device__ __forceinline__ void normalize(float &x, float &y, float &z) {
    const float l2 = dot3(x, y, z, x, y, z);
    const bool keep = l2 > kEps;
    const float len = sqrt_rn(l2);
    const float inv = rcp_rn(len);
    float qx = div_rn(x, len, inv), qy = div_rn(y, len, inv), qz = div_rn(z, len, inv);
    // (a zero component also takes the IEEE path: rare, and exact either way)
    const float m = __builtin_fminf(__builtin_fminf(__builtin_fabsf(qx), __builtin_fabsf(qy)), __builtin_fabsf(qz));
    if (__builtin_expect(keep && (m < 0x1p-99f || !(len <= 0x1p40f)), 0)) {
        const float ieee_len = __builtin_sqrtf(l2);
        qx = x / ieee_len;
        qy = y / ieee_len;
        qz = z / ieee_len;
    }
    x = keep ? qx : 0.0f;
    y = keep ? qy : 0.0f;
    z = keep ? qz : 0.0f;
}

// rsqrtss (x64_math.h:71-74) from the 2x1024 table: exponent parity + top
// 10 mantissa bits pick the entry, the remaining even exponent scales it.
// The table sits in the block's LDS image, or (large scenes, in_lds false:
// the LDS budget goes to occupancy) is read from HBM through the caches.
struct Lut {
    const float *lds, *glob;
    bool in_lds;  // wave-uniform
};

// For a positive normal v with unbiased exponent e: the entry is
// (e & 1) * 1024 + mantissa[22:13], i.e. bits [23:13] of v with bit 23 (the
// biased exponent's parity, the opposite of e's) flipped; the scale is
// floor(e / 2), which is (int)(bits(v) - bits(1.0f)) >> 24 (the mantissa adds
// less than half a unit of that shift).  Checked against the direct form on
// every positive normal f32 (index and result bits): two bit-field ops instead
// of five, most of them the half-rate shift class.
__device__ __forceinline__ float rsqrt_x86(const Lut &lut, float v) {
    const uint32_t u = __float_as_uint(v);
    const uint32_t idx = ((u >> 13) & 2047u) ^ 1024u;
    const float base = lut.in_lds ? lut.lds[idx] : lut.glob[idx];
    const int32_t sh = (int32_t)(u - 0x3F800000u) >> 24;
    return __uint_as_float(__float_as_uint(base) - ((uint32_t)sh << 23));
}

__device__ __forceinline__ float saturate(float v) {  // x64_math.h:97-101
    if (v < 0.0f) return 0.0f;
    if (v > 1.0f) return 1.0f;
    return v;
}

__device__ __forceinline__ uint32_t to_u8(float v) {  // main.cpp:341-343
    const float s = saturate(v) * 255.0f;
    if (s != s) return 0u;
    return (uint32_t)(int32_t)s & 0xFFu;
}

__device__ __forceinline__ float linear_to_srgb(float l) {  // main.cpp:312-329
    l = saturate(l);
    return l < 0.0031308f ? l * 12.92f : sqrt_rn(l);  // l in [0.0031308, 1]
}

// The exact-pow branch of LinearToSRGB (main.cpp:320-321, '#if 0' in the
// reference; RT_FLAG_SRGB_POW).  powf there is libm's (musl in the WASM build,
// glibc on Linux: the same algorithm, not correctly rounded); here the f64
// pow rounded once to f32.  The two differ in the last f32 bit on ~46k of the
// 70.4M inputs in [0.0031308, 1], and the RGBA8 byte on none of them
// (exhaustive: tests/test_srgb_pow.py on the CPU, and the GPU's own bytes
// against the oracle's over the same range in tests/test_gpu_parity.py).
// Unfused, as wasm32 has no FMA.
__device__ __forceinline__ float linear_to_srgb_pow(float l) {
    l = saturate(l);
    if (l < 0.0031308f) return l * 12.92f;
    const float p = (float)pow((double)l, (double)(1.0f / 2.4f));
    return 1.055f * p - 0.055f;
}

// ColorFromV4(LinearToSRGB(v)) (main.cpp:340-346, 490).
__device__ __forceinline__ uint32_t rgba8(float x, float y, float z, bool pw) {
    if (pw)
        return to_u8(linear_to_srgb_pow(x)) | (to_u8(linear_to_srgb_pow(y)) << 8) |
               (to_u8(linear_to_srgb_pow(z)) << 16) | (255u << 24);
    return to_u8(linear_to_srgb(x)) | (to_u8(linear_to_srgb(y)) << 8) | (to_u8(linear_to_srgb(z)) << 16) |
           (255u << 24);
}

// r0 = ((1 - eta)/(1 + eta))^2 comes from the sphere record: the host's IEEE
// division and product per material and side (rt_pack.cpp put_material), the
// same bits as the kernel's own (RTWeekend +0.4 %, its 8-rank share +1.3 %,
// profiles/r06s_diel_tab_ab.txt)
__device__ __forceinline__ float reflectance(float cos_t, float r0) {  // main.cpp:292-300
    float r1 = 1.0f - cos_t;
    r1 = r1 * r1 * r1 * r1 * r1;
    return __builtin_fmaf(1.0f - r0, r1, r0);  // contracted by the reference's -mfma build
}

typedef float f2 __attribute__((ext_vector_type(2)));

struct Sample {
    f2 rx, ry, rz;     // {origin, direction} per axis (the packed pair test reads them in place)
    float ax, ay, az;  // attenuation
    float cx, cy, cz;  // output colour
    uint64_t rng;
    uint32_t bounce;
};

// Jittered primary ray (main.cpp:375-385).
// The kernel's by-value TraceArgs re-read from the kernarg segment (scalar
// loads, K$ hits) at each use: the camera fields start_sample needs are then
// not held in SGPRs across the trace loop, where they were spilled to VGPR
// lanes and restored with ~30 v_readlane per primary round.
typedef const __attribute__((address_space(4))) TraceArgs cargs_t;
__device__ __forceinline__ cargs_t &kernel_args() {
    cargs_t *p = (cargs_t *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));  // opaque per use: the loads stay at the use site
    return *p;
}

// A launch-invariant value tested where it is used: opaque to the optimiser at that use, so the
// test stays there as one scalar compare.  Left to the compiler the compare is hoisted out of
// the trip loop and its result held across the loop as a 64-bit lane mask.
__device__ __forceinline__ uint32_t at_use(uint32_t v) {
    asm volatile("" : "+s"(v));
    return v;
}

// CENTRE (the first-hit pass's RT_HIT_PIXEL_CENTRE): both jitters are exactly 0 and no RNG is touched
// (p.rng is left 0); every operation from the film point on is the same sequence.
template <bool CENTRE = false, typename Args>
__device__ __forceinline__ void start_sample(const Args &a, uint32_t x, uint32_t y, uint32_t frame, Sample &p) {
    p.rng = CENTRE ? 0ull : seed_mix(((uint64_t)frame * a.height + y) * a.width + x);
    const float jx = CENTRE ? 0.0f : rand_float(p.rng, -0.5f, kInvRange1);
    const float jy = CENTRE ? 0.0f : rand_float(p.rng, -0.5f, kInvRange1);
    // ((x + Jx) * 2) / W with (f32)W and its reciprocal RN(1/W) from the host: the
    // numerator is +0 or >= 2^-24 (Jx = -0.5 + r is never -0), so div_rn's
    // range condition holds
    const float fx = -1.0f + div_rn(((float)x + jx) * 2.0f, a.width_f, a.inv_width);
    const float fy = -1.0f + div_rn(((float)y + jy) * 2.0f, a.height_f, a.inv_height);
    const float kx = (fx * a.film_w) * 0.5f;
    const float ky = (fy * a.film_h) * 0.5f;
    const float px = (a.film_center[0] + kx * a.cam_x[0]) + ky * a.cam_y[0];
    const float py = (a.film_center[1] + kx * a.cam_x[1]) + ky * a.cam_y[1];
    const float pz = (a.film_center[2] + kx * a.cam_x[2]) + ky * a.cam_y[2];
    p.rx.x = a.cam_pos[0];
    p.ry.x = a.cam_pos[1];
    p.rz.x = a.cam_pos[2];
    float dx = px - p.rx.x, dy = py - p.ry.x, dz = pz - p.rz.x;
    normalize(dx, dy, dz);
    p.rx.y = dx;
    p.ry.y = dy;
    p.rz.y = dz;
    p.ax = p.ay = p.az = 1.0f;
    p.cx = p.cy = p.cz = 0.0f;
    p.bounce = 0;
}

// Emission, attenuation and the next direction (main.cpp:446-481).  A hit at the bounce limit
// takes the emission term alone: trace_kernel restates the first three statements for it, and
// they must stay the same operations on the same operands there and here.
__device__ __forceinline__ void shade(const Lut &lut, float4 col_spec, float4 emis_ior, const float4 *diel, float hx,
                                      float hy, float hz, bool inside, Sample &p) {
    p.cx = p.cx + emis_ior.x * p.ax;
    p.cy = p.cy + emis_ior.y * p.ay;
    p.cz = p.cz + emis_ior.z * p.az;
    p.ax = p.ax * col_spec.x;
    p.ay = p.ay * col_spec.y;
    p.az = p.az * col_spec.z;
    float nx = hx, ny = hy, nz = hz;
    normalize(nx, ny, nz);
    const float k2 = 2.0f * dot3(p.rx.y, p.ry.y, p.rz.y, nx, ny, nz);
    const float bx = p.rx.y - k2 * nx, by = p.ry.y - k2 * ny, bz = p.rz.y - k2 * nz;  // PureBounce
    if (inside) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    const float ior = emis_ior.w;
    if (ior == 0.0f) {
        float rx = rand_float(p.rng, -1.0f, kInvRange2);
        float ry = rand_float(p.rng, -1.0f, kInvRange2);
        float rz = rand_float(p.rng, -1.0f, kInvRange2);
        const float l2 = dot3(rx, ry, rz, rx, ry, rz);  // v3::NormalizeFast
        const bool keep = l2 > kEps;
        const float inv = rsqrt_x86(lut, l2);
        rx = keep ? rx * inv : 0.0f;
        ry = keep ? ry * inv : 0.0f;
        rz = keep ? rz * inv : 0.0f;
        const float s = col_spec.w;
        const float om = 1.0f - s;
        float dx = om * (nx + rx) + s * bx;
        float dy = om * (ny + ry) + s * by;
        float dz = om * (nz + rz) + s * bz;
        normalize(dx, dy, dz);
        p.rx.y = dx;
        p.ry.y = dy;
        p.rz.y = dz;
    } else {
        // {1/IOR, r0 outside, r0 inside} of the record's row 3 (dielectric lanes only)
        const float4 dq = *diel;
        const float eta = inside ? ior : dq.x;
        const float dd = dot3(-p.rx.y, -p.ry.y, -p.rz.y, nx, ny, nz);
        const float cos_t = dd < 1.0f ? dd : 1.0f;  // _mm_min_ss
        // |1 - q.q| is +0, >= 2^-25 or NaN: inside sqrt_rn's range (NaN stays NaN).  1 - c*c is +0 or
        // >= 2^-25 for |c| <= 1; cos_t a few ulps below -1 makes it negative, where the reference's sqrtss
        // gives NaN and sqrt_rn -inf (or a large negative value): `eta * sin_t > 1` is false for both, and
        // sin_t has no other use (tests/test_gpu_math_layer.py, test_sqrt_rn_below_zero...)
        const float sin_t = sqrt_rn(1.0f - cos_t * cos_t);
        const bool cant = eta * sin_t > 1.0f;
        const float qx = eta * (p.rx.y + cos_t * nx);
        const float qy = eta * (p.ry.y + cos_t * ny);
        const float qz = eta * (p.rz.y + cos_t * nz);
        const float q = -sqrt_rn(__builtin_fabsf(1.0f - dot3(qx, qy, qz, qx, qy, qz)));
        float rx = qx + q * nx, ry = qy + q * ny, rz = qz + q * nz;
        normalize(rx, ry, rz);
        bool refl = cant;
        if (!refl) refl = reflectance(cos_t, inside ? dq.z : dq.y) > rand_float(p.rng, 0.0f, kInvRange1);
        if (refl && !inside) {
            p.rx.y = bx;
            p.ry.y = by;
            p.rz.y = bz;
        } else {
            p.rx.y = rx;
            p.ry.y = ry;
            p.rz.y = rz;
        }
    }
}

}  // namespace rtk
