// rtk_walk.h — the sphere walks of the trace kernel: group loaders, the exact
// packed pair test and candidate logic, the FMA prefilter and its exact
// recheck, the clustered prefilter walk, and the primary rounds' pair test.
#pragma once
#include "rtk_math.h"

namespace rtk {

struct Group {
    float x[4], y[4], z[4], r2[4];
    float r2p[4];  // prefilter threshold r^2 + E (see pair_prefilter)
};

__device__ __forceinline__ void group_rows(Group &G, float4 x, float4 y, float4 z, float4 r2p, float4 r2) {
    G.x[0] = x.x; G.x[1] = x.y; G.x[2] = x.z; G.x[3] = x.w;
    G.y[0] = y.x; G.y[1] = y.y; G.y[2] = y.z; G.y[3] = y.w;
    G.z[0] = z.x; G.z[1] = z.y; G.z[2] = z.z; G.z[3] = z.w;
    G.r2p[0] = r2p.x; G.r2p[1] = r2p.y; G.r2p[2] = r2p.z; G.r2p[3] = r2p.w;
    G.r2[0] = r2.x; G.r2[1] = r2.y; G.r2[2] = r2.z; G.r2[3] = r2.w;
}

// Group rows from the constant address space: read-only for the kernel's
// lifetime, so a wave-uniform address always becomes s_loads into SGPRs
// (immediate offsets from one base: rows 0-3 one dwordx16, row 4 a dwordx4).
// Rows 0-3 hold the centres and r*r, all an exact test reads; row 4 the prefilter thresholds.
typedef float v4f_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) v4f_t cv4f_t;
__device__ __forceinline__ float4 f4(v4f_t v) { return make_float4(v.x, v.y, v.z, v.w); }
// Rows 0-3 of a group record or of a cluster-table entry: one contiguous 64 B
// block at a 16 B aligned address, read as ONE s_load_dwordx16 (row by row the
// backend issued a dwordx8 and two dwordx4 for it: three scalar-memory
// instructions and their address setup per entry of the walk).
typedef float v16f_t __attribute__((ext_vector_type(16)));
typedef v16f_t v16f_a16_t __attribute__((aligned(16)));
typedef const __attribute__((address_space(4))) v16f_a16_t cv16f_t;
struct Rows4 {
    v4f_t r0, r1, r2, r3;
};
__device__ __forceinline__ Rows4 load_rows4(cv4f_t *e) {
    const v16f_t v = *(cv16f_t *)e;
    return {__builtin_shufflevector(v, v, 0, 1, 2, 3), __builtin_shufflevector(v, v, 4, 5, 6, 7),
            __builtin_shufflevector(v, v, 8, 9, 10, 11), __builtin_shufflevector(v, v, 12, 13, 14, 15)};
}
static_assert(kRowX == 0 && kRowY == 1 && kRowZ == 2 && kRowR2 == 3 && kRowR2P == 4, "group rows 0-3: centres and r*r");
__device__ __forceinline__ Group load_group_at(cv4f_t *cg) {
    Group G;
    const Rows4 r = load_rows4(cg);
    group_rows(G, f4(r.r0), f4(r.r1), f4(r.r2), f4(cg[kRowR2P]), f4(r.r3));
    return G;
}

template <int SRC>
__device__ __forceinline__ Group load_group(const TraceArgs &a, const float4 *lds_groups, uint32_t g) {
    if (SRC == kSrcSmem) return load_group_at((cv4f_t *)a.groups + kGroupF4 * g);
    Group G;
    const float4 *r = lds_groups + kGroupF4 * g;
    group_rows(G, r[kRowX], r[kRowY], r[kRowZ], r[kRowR2P], r[kRowR2]);
    return G;
}

// The shared part of one sphere test: T, |C - D*T|^2 (main.cpp:401-407).
__device__ __forceinline__ void sphere_core(const Sample &p, float sx, float sy, float sz, float &T, float &dist) {
    const float cx = sx - p.rx.x, cy = sy - p.ry.x, cz = sz - p.rz.x;
    T = dot3(cx, cy, cz, p.rx.y, p.ry.y, p.rz.y);
    const float qx = cx - p.rx.y * T, qy = cy - p.ry.y * T, qz = cz - p.rz.y * T;
    dist = dot3(qx, qy, qz, qx, qy, qz);
}

// Per-lane hit state.  SIMD rules: the reference's four lane minima
// (MinT / MaterialIndex / InsideSphere, main.cpp:394-396), one per residue
// class s & 3.  Scalar rules use slot 0 only (main.cpp:541-545).
// A class keeps its sphere and its inside flag as one key, (4 g + L) | inside << 31: the word a
// pending hit carries (trace_kernel pend_s), so the hit select picks one register per class and
// rebuilds nothing.
// The scalar rules keep what they kept: the sphere index in k0 and the flag, which is not sticky there,
// in `ins` (the reference's two variables, main.cpp:574-575).  Their select is no more than an OR of
// the two, so a packed key saves them nothing, and with it the 8-wave kernels of the scalar rules spilled
// registers the parent form does not (profiles/r15a_resources.txt).  `ins` is dead under the SIMD rules.
constexpr uint32_t kKeyInside = 0x80000000u;
struct Hit {
    float t0, t1, t2, t3;
    uint32_t k0, k1, k2, k3;
    uint32_t ins;
};

__device__ __forceinline__ void hit_reset(Hit &h) {
    h.t0 = h.t1 = h.t2 = h.t3 = kFMax;
    h.k0 = h.k1 = h.k2 = h.k3 = 0;
    h.ins = 0;
}

// The key of an accepted candidate: s | in << 31 for the wave-uniform sphere index s (below 2^31).
// gfx950 reads one scalar register or literal per VALU instruction, the select's lane mask included,
// so selecting between the two scalars s and s | 2^31 costs two copies into VGPRs first.  The select's
// own source modifier sets the bit instead: a negated source of v_cndmask_b32 is the source with bit 31
// flipped, bit for bit (no arithmetic, nothing canonicalised), so one copy of s and one select do it.
// Small sphere indices are f32 denormals as bit patterns: that the modifier flips bit 31 and flushes
// nothing was confirmed on gfx950 by the bit-exact GPU suite (tests/test_gpu_hit_key.py among it, sphere
// indices from 0 up); a port to another target has to check it again.
// in_mask: the lane mask of `in`, taken where `in` is compared (candidate), so that it is the compare's
// own SGPR pair.  A ballot taken inside the accept region is rebuilt there with v_cndmask + v_cmp_ne,
// two VALU per accepted candidate and a VGPR live into the region.  Only the bits of lanes active at
// the select are read, and for those the mask taken outside holds the lane's own `in`.
__device__ __forceinline__ uint32_t hit_key(uint32_t s, uint64_t in_mask) {
    uint32_t key;
    asm("v_cndmask_b32_e64 %0, %1, -%1, %2" : "=v"(key) : "v"(s), "s"(in_mask));
    return key;
}

// Exact intersection of one candidate sphere (main.cpp:413-429 / 561-578),
// given its T and |C - D*T|^2 from the packed distance test.
// fast: the host proved every hittable r^2 is 0 or in [2^-36, 2^60], so
// r^2 - dist (positive, hence >= ulp(r^2)/2, or exactly 0) is inside sqrt_rn's
// verified range.
template <bool SIMD, int L>
__device__ __forceinline__ void candidate(Hit &h, uint32_t g, float T, float dist, float r2, bool fast) {
    const float X = fast ? sqrt_rn(r2 - dist) : __builtin_sqrtf(r2 - dist);
    float it = T - X;
    const bool in = it < kEps;
    const uint64_t in_mask = __builtin_amdgcn_ballot_w64(in);  // (see hit_key)
    if (in) it = T + X;
    const uint32_t s = 4u * g + (uint32_t)L;  // (wave-uniform)
    if (SIMD) {
        float &tl = L == 0 ? h.t0 : L == 1 ? h.t1 : L == 2 ? h.t2 : h.t3;
        uint32_t &kl = L == 0 ? h.k0 : L == 1 ? h.k1 : L == 2 ? h.k2 : h.k3;
        if (it < tl && it > kEps) {  // strict: the earliest group keeps a tie
            tl = it;
            // the class's flag is a sticky OR (main.cpp:425): bit 31 of the old key stays
            kl = (kl & kKeyInside) | hit_key(s, in_mask);
        }
    } else {
        if (!(it > h.t0) && !(it < kEps)) {  // the later sphere wins a tie
            h.t0 = it;
            h.k0 = s;
            h.ins = in ? 1u : 0u;  // (not sticky: main.cpp:574)
        }
    }
}


// T and |C - D*T|^2 for two spheres of a group at once: every f32 op of
// main.cpp:401-407 becomes one packed v_pk_{add,mul}_f32 over the pair (same
// IEEE rounding per element; a packed op issues at the cost of a scalar one
// on gfx950, so this halves the sphere loop's VALU instructions).
// The ray as three {origin, direction} register pairs: a packed op can then
// broadcast either half to both lanes with op_sel / op_sel_hi, so the pair
// test needs no duplicated (splat) copies of the ray.
struct RayPk {
    f2 x, y, z;  // {o, d} per axis
};

__device__ __forceinline__ f2 pair_dist(const RayPk &r, f2 sx, f2 sy, f2 sz, f2 &T) {
    f2 cx, cy, cz, t, d;
    // c = s - o ; T = (cx*dx + cy*dy) + cz*dz ; q = c - d*T (in c) ;
    // dist = (qx*qx + qy*qy) + qz*qz  -- op for op the reference's f32 sequence
    asm("v_pk_add_f32 %[cx], %[sx], %[rx] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %[cy], %[sy], %[ry] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %[cz], %[sz], %[rz] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t], %[cx], %[rx] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %[d], %[cy], %[ry] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[T], %[t], %[d]\n\t"
        "v_pk_mul_f32 %[t], %[cz], %[rz] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[T], %[T], %[t]\n\t"
        "v_pk_mul_f32 %[t], %[rx], %[T] op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[cx], %[cx], %[t] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t], %[ry], %[T] op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[cy], %[cy], %[t] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t], %[rz], %[T] op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[cz], %[cz], %[t] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[d], %[cx], %[cx]\n\t"
        "v_pk_mul_f32 %[t], %[cy], %[cy]\n\t"
        "v_pk_add_f32 %[d], %[d], %[t]\n\t"
        "v_pk_mul_f32 %[t], %[cz], %[cz]\n\t"
        "v_pk_add_f32 %[d], %[d], %[t]"
        : [cx] "=&v"(cx), [cy] "=&v"(cy), [cz] "=&v"(cz), [t] "=&v"(t), [T] "=&v"(T), [d] "=&v"(d)
        : [sx] "s"(sx), [sy] "s"(sy), [sz] "s"(sz), [rx] "v"(r.x), [ry] "v"(r.y), [rz] "v"(r.z));
    return d;
}

// Secondary-ray prefilter: an FMA estimate of |C - D*T|^2 for two spheres
// in 10 packed ops instead of the exact test's 19:
//   C = S - O ;  cc = |C|^2 ;  T = C.D ;  e = cc - T*T      (fused)
// For |D|^2 within K = 2^-16 of 1 and every origin on a sphere of the scene
// (true for all secondary rays: NextRayOrigin is a hit point), |e - dist|
// where dist is the reference's exactly-rounded value (main.cpp:401-407) is
// below E_j = M_j (32u + 1.01K), u = 2^-24, M_j a bound on |C|^2 for
// sphere j over every such origin (derivation: DESIGN.md).  The host stores
// r2p_j >= r^2_j + E_j (rounded up), so e >= r2p proves dist > r^2 -- the
// sphere is missed under both rule sets -- and only groups where some lane
// fails that proof run the exact test.  A wave with any lane outside the
// |D|^2 bound runs the exact loop instead.
__device__ __forceinline__ f2 pair_prefilter(const RayPk &r, f2 sx, f2 sy, f2 sz, f2 &T, f2 &cc) {
    f2 cx, cy, cz, e;
    asm("v_pk_add_f32 %[cx], %[sx], %[rx] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %[cy], %[sy], %[ry] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %[cz], %[sz], %[rz] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[cc], %[cz], %[cz]\n\t"
        "v_pk_fma_f32 %[cc], %[cy], %[cy], %[cc]\n\t"
        "v_pk_fma_f32 %[cc], %[cx], %[cx], %[cc]\n\t"
        "v_pk_mul_f32 %[T], %[cx], %[rx] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_fma_f32 %[T], %[cy], %[ry], %[T] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %[T], %[cz], %[rz], %[T] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %[e], %[T], %[T], %[cc] neg_lo:[1,0,0] neg_hi:[1,0,0]"
        : [cx] "=&v"(cx), [cy] "=&v"(cy), [cz] "=&v"(cz), [cc] "=&v"(cc), [T] "=&v"(T), [e] "=&v"(e)
        : [sx] "s"(sx), [sy] "s"(sy), [sz] "s"(sz), [rx] "v"(r.x), [ry] "v"(r.y), [rz] "v"(r.z));
    return e;
}

// The expanded prefilter of the scene-wide cluster walks (kWalkCl1 / Cl2 / Cl4; rt_pack.cpp
// expand_table proves it): the same estimate written as dot products of the centre
// itself, so the three packed subtractions C = S - O per pair go and nothing is left per sphere but
// FMAs -- 7 packed ops instead of 10, the centre rows still in SGPRs.  With S' = RN(S - c0) from the
// host's second table and O' = RN(O - c0) (c0: the table's centre, so that the values that cancel
// stay of the scene's own size):
//   T  = fma(S'x, Dx, fma(S'y, Dy, fma(S'z, Dz, -O'.D)))           ~ (S - O).D
//   A  = fma(S'x, -2O'x, fma(S'y, -2O'y, fma(S'z, -2O'z, |O'|^2)))  ~ |S - O|^2 - |S'|^2
//   e' = fma(-T, T, A)                                              ~ e - |S'|^2
// and the table's thresholds are t' = t - |S'|^2 + G (near the line: e' >= t' skips) and behind
// thresholds lowered by T's new error.  The ray's part, formed once per walk in this fixed order:
//   O'    = O - c0 per axis (one rounding each)
//   |O'|^2 = fma(O'x, O'x, fma(O'y, O'y, O'z O'z))
//   -O'.D  = -fma(O'x, Dx, fma(O'y, Dy, O'z Dz))
// held as three pairs {-2O', D} (the doubling and the negation are exact) and {|O'|^2, -O'.D}, so a
// packed op broadcasts either half with op_sel as pair_prefilter does.
struct RayX {
    f2 x, y, z;  // {-2O', D} per axis
    f2 w;        // {|O'|^2, -O'.D}
};

// Written where the walk starts (as walk_const): c0 is read from the table there and the origin passes
// through an empty asm, so the block is neither formed at shading time nor held across the trip loop.
__device__ __forceinline__ RayX ray_expand(const RayPk &r, v4f_t c0) {
    float ox = r.x.x - c0.x, oy = r.y.x - c0.y, oz = r.z.x - c0.z;
    asm volatile("" : "+v"(ox), "+v"(oy), "+v"(oz));
    const float dx = r.x.y, dy = r.y.y, dz = r.z.y;
    const float oo = __builtin_fmaf(ox, ox, __builtin_fmaf(oy, oy, oz * oz));
    const float od = __builtin_fmaf(ox, dx, __builtin_fmaf(oy, dy, oz * dz));
    return {f2{-2.0f * ox, dx}, f2{-2.0f * oy, dy}, f2{-2.0f * oz, dz}, f2{oo, -od}};
}

__device__ __forceinline__ f2 pair_prefilter_x(const RayX &r, f2 sx, f2 sy, f2 sz, f2 &T) {
    f2 A, e;
    asm("v_pk_fma_f32 %[T], %[sz], %[rz], %[rw] op_sel:[0,1,1] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %[T], %[sy], %[ry], %[T] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %[T], %[sx], %[rx], %[T] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %[A], %[sz], %[rz], %[rw] op_sel_hi:[1,0,0]\n\t"
        "v_pk_fma_f32 %[A], %[sy], %[ry], %[A] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %[A], %[sx], %[rx], %[A] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %[e], %[T], %[T], %[A] neg_lo:[1,0,0] neg_hi:[1,0,0]"
        : [T] "=&v"(T), [A] "=&v"(A), [e] "=&v"(e)
        : [sx] "s"(sx), [sy] "s"(sy), [sz] "s"(sz), [rx] "v"(r.x), [ry] "v"(r.y), [rz] "v"(r.z), [rw] "v"(r.w));
    return e;
}

// The exact recheck of one group's flagged sphere pairs (f01, f23): only such
// a pair reruns the exact packed test (same ops as test_group) and the exact
// candidate logic decides, so results are identical.
// The group's r^2 row comes with its centres (rows 0-3 of the record, one
// scalar load: load_group_exact_at / load_group_at).
template <bool SIMD>
__device__ __forceinline__ void recheck_pairs(const TraceArgs &a, const Group &G, uint32_t g, const RayPk &p, Hit &h, bool fast,
                                              bool f01, bool f23) {
    const float4 r2 = make_float4(G.r2[0], G.r2[1], G.r2[2], G.r2[3]);
    if (f01) {
        f2 T01;
        const f2 d01 = pair_dist(p, f2{G.x[0], G.x[1]}, f2{G.y[0], G.y[1]}, f2{G.z[0], G.z[1]}, T01);
        const uint32_t s0 = 4u * g;
        const bool h0 = SIMD ? d01.x < r2.x : s0 + 0u < a.n_spheres && !(d01.x > r2.x);
        const bool h1 = SIMD ? d01.y < r2.y : s0 + 1u < a.n_spheres && !(d01.y > r2.y);
        if (h0) candidate<SIMD, 0>(h, g, T01.x, d01.x, r2.x, fast);
        if (h1) candidate<SIMD, 1>(h, g, T01.y, d01.y, r2.y, fast);
    }
    if (f23) {
        f2 T23;
        const f2 d23 = pair_dist(p, f2{G.x[2], G.x[3]}, f2{G.y[2], G.y[3]}, f2{G.z[2], G.z[3]}, T23);
        const uint32_t s0 = 4u * g;
        const bool h2 = SIMD ? d23.x < r2.z : s0 + 2u < a.n_spheres && !(d23.x > r2.z);
        const bool h3 = SIMD ? d23.y < r2.w : s0 + 3u < a.n_spheres && !(d23.y > r2.w);
        if (h2) candidate<SIMD, 2>(h, g, T23.x, d23.x, r2.z, fast);
        if (h3) candidate<SIMD, 3>(h, g, T23.y, d23.y, r2.w, fast);
    }
}

// Per-lane ("relative") prefilter threshold: t = RN(cc * 2^-15 + r^2) with
// cc = the lane's computed |C|^2, where the threshold row (kRowR2P) holds r^2 (-inf: never hit).
// The error bound of e (and of the reference-rounded dist) scales with the
// lane's own |C|^2 instead of the scene-wide M_j, so the test still proves
// misses in scenes whose M_j bound is useless (RTWeekend's ground sphere
// makes M ~ 1.6e4 against r^2 ~ 1.6e-4).  Proof: with
// |C|^2 <= cc (1 + 5u) and E = 23.5u + K(1+K) the combined error of e and of
// the reference's dist relative to |C|^2, e >= t gives dist > r^2 whenever
// cc >= r^2 / 232 (then cc (2^-15 (1-u) - (1+5u) E) >= u r^2 covers t's own
// rounding); and when cc < r^2 / 232, e <= cc < t, so nothing is skipped.
constexpr float kPfRel = 0x1p-15f;

// Prefilter flags of group G's two sphere pairs for this lane's ray.
template <bool REL>
__device__ __forceinline__ void prefilter_group(const Group &G, const RayPk &p, bool &f01, bool &f23) {
    f2 T01, T23, c01, c23;
    const f2 e01 = pair_prefilter(p, f2{G.x[0], G.x[1]}, f2{G.y[0], G.y[1]}, f2{G.z[0], G.z[1]}, T01, c01);
    const f2 e23 = pair_prefilter(p, f2{G.x[2], G.x[3]}, f2{G.y[2], G.y[3]}, f2{G.z[2], G.z[3]}, T23, c23);
    if (REL) {
        f01 = !(e01.x >= __builtin_fmaf(c01.x, kPfRel, G.r2p[0])) | !(e01.y >= __builtin_fmaf(c01.y, kPfRel, G.r2p[1]));
        f23 = !(e23.x >= __builtin_fmaf(c23.x, kPfRel, G.r2p[2])) | !(e23.y >= __builtin_fmaf(c23.y, kPfRel, G.r2p[3]));
    } else {
        f01 = !(e01.x >= G.r2p[0]) | !(e01.y >= G.r2p[1]);
        f23 = !(e23.x >= G.r2p[2]) | !(e23.y >= G.r2p[3]);
    }
}

// The prefiltered walks' counters of the diagnostic build (rtk_trace.h TraceStats; clustered_groups says
// what each counts there)
struct PfStats {
    uint32_t groups, cl_tested, pairs, cl_top_entered, lane_pairs;
    // entries some lane is near on either half (near-line ballots n0 | n1 != 0): member-pair entries, cluster-pair entries
    uint32_t near_entries, cl_near_entries;
};

// Group g for a secondary ray through the prefilter: one wave branch per
// group, and inside it one per flagged pair.  (Measured: +5.5 % on C2 over
// one exact recheck of both pairs per flagged group.)
template <bool SIMD, bool GS, bool REL>
__device__ __forceinline__ void test_group_pf(const TraceArgs &a, const float4 *lds_groups, const Group &G, uint32_t g,
                                              const RayPk &p, Hit &h, bool fast, PfStats *ps = nullptr) {
    bool f01, f23;
    prefilter_group<REL>(G, p, f01, f23);
    if (ps) {
        ps->groups += __ballot(f01 | f23) != 0;
        ps->pairs += (__ballot(f01) != 0) + (__ballot(f23) != 0);
        ps->lane_pairs += __builtin_popcountll(__ballot(f01)) + __builtin_popcountll(__ballot(f23));
    }
    if (f01 | f23) recheck_pairs<SIMD>(a, G, g, p, h, fast, f01, f23);
}

template <bool SIMD>
__device__ __forceinline__ void test_group(const TraceArgs &a, const Group &G, uint32_t g, const RayPk &p, Hit &h, bool fast,
                                           uint32_t *hit_groups);

// Rows 0-3 only (one s_load_dwordx16): what the exact recheck of the cluster walk reads.
__device__ __forceinline__ Group load_group_exact_at(cv4f_t *cg) {
    Group G;
    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const Rows4 r = load_rows4(cg);
    group_rows(G, f4(r.r0), f4(r.r1), f4(r.r2), z4, f4(r.r3));
    return G;
}

// The full sphere loop over all groups from SGPRs.  PF: secondary rays
// through the prefilter; else the exact test.
template <bool SIMD, bool PF, bool GS, bool REL = false>
__device__ __forceinline__ void all_groups_smem(const TraceArgs &a, const float4 *lds_groups, const RayPk &ray, Hit &h, bool fast,
                                                uint32_t *hit_groups, PfStats *ps = nullptr) {
    cv4f_t *gp = (cv4f_t *)a.groups;
    // one group in SGPRs at a time: its s_load (scalar-cache hit) is covered
    // by the other waves on the SIMD -- measured as fast as a ping-pong
    // prefetch, at half the SGPRs (and two groups per trip under one branch
    // measured 2 % slower)
    for (uint32_t g = 0; g < a.n_groups; ++g, gp += kGroupF4) {
        const Group G = load_group_at(gp);
        if (PF) test_group_pf<SIMD, GS, REL>(a, lds_groups, G, g, ray, h, fast, ps);
        else test_group<SIMD>(a, G, g, ray, h, fast, hit_groups);
    }
}

// The clustered prefilter (secondary rays; rt_pack.cpp cluster_table proves
// it).  A wave tests the ray against about sqrt(n) cluster bounding volumes,
// two per packed prefilter, and only the members of a cluster some lane may
// reach run the per-sphere prefilter; a sphere pair some lane may hit sets
// bit (slot >> 1) of the wave's pair mask (W u64 words, SGPRs only; W = 1
// tables carry the bit itself, W = 2 tables the pair index).  The
// exact recheck then walks the flagged groups in ascending order -- the
// reference's order, so the per-class minima, tie rules and sticky inside flags
// come out as in the full loop.  The recheck runs on every lane: a lane whose
// own estimate cleared the pair has a proven miss there, which its exact test
// reproduces, so no per-lane flags are needed.
constexpr int kClWords = 4;  // pair-mask words (n_groups <= 128)
// Per-lane thresholds (pf_relative, rt_pack.cpp per_lane_bounds):
// cluster: e_c >= RN(cc kClRel + R_c); sphere: e >= RN(cc kPfRel + r^2) (kPfRel
// below); behind: T < RN(b - cc kBehindRel).
constexpr float kClRel = 9.2e-4f;               // >= (a + a^2 + E1)(1 + 6u), a = 8.917e-4
constexpr float kBehindRel = 4.5f * 0x1p-24f;    // >= 4.3u (|Q|, |C_j| <= (1 + cc)/2)

// ballot(a && b) as ballot(a) & ballot(b): the backend folds the ballot of a
// single compare into the v_cmp's own lane mask, but materialises the ballot of
// a conjunction through v_cndmask + v_cmp_ne (two VALU per ballot)
__device__ __forceinline__ uint64_t ballot_and(bool a, bool b) {
    return __builtin_amdgcn_ballot_w64(a) & __builtin_amdgcn_ballot_w64(b);
}

// One trip's round decision (trace_kernel), on the scalar unit in six instructions:
//   pri    = want & ring                   the lanes that can start their pending sample
//   do_sec = popcount(sec) >= (pri ? thr : 1)
//          = sec != 0 && (pri == 0 || popcount(sec) >= thr) for thr >= 1 (rt_host.cpp sets no 0)
//   round  = do_sec ? sec : pri            the lanes this round traces
// The conjunction's own SCC (pri != 0) picks the count to compare against and the compare's SCC
// picks the round's mask (as merge_word1 does); the compiler's lowering turned each compare into
// a 64-bit lane mask (s_cselect_b64 -1/0) and combined and re-tested the masks -- about 20
// scalar instructions for the same three values.  do_sec comes back as an integer so that its
// later tests are scalar compares of it, not further lane masks.
__device__ __forceinline__ void round_select(uint64_t want, uint64_t ring, uint64_t sec, uint32_t thr, uint64_t &pri,
                                             uint32_t &do_sec, uint64_t &round) {
    uint32_t need;
    asm("s_and_b64 %[pri], %[want], %[ring]\n\t"
        "s_cselect_b32 %[need], %[thr], 1\n\t"
        "s_bcnt1_i32_b64 %[ds], %[sec]\n\t"
        "s_cmp_ge_u32 %[ds], %[need]\n\t"
        "s_cselect_b32 %[ds], 1, 0\n\t"
        "s_cselect_b64 %[rnd], %[sec], %[pri]"
        : [pri] "=&s"(pri), [need] "=&s"(need), [ds] "=&s"(do_sec), [rnd] "=&s"(round)
        : [want] "s"(want), [ring] "s"(ring), [sec] "s"(sec), [thr] "s"(thr)
        : "scc");
}

// (a | b) != 0 as an integer from the OR's own SCC: the test of it is then one scalar compare
__device__ __forceinline__ uint32_t any_lane(uint64_t a, uint64_t b) {
    uint64_t t;
    uint32_t r;
    asm("s_or_b64 %[t], %[a], %[b]\n\t"
        "s_cselect_b32 %[r], 1, 0"
        : [t] "=&s"(t), [r] "=&s"(r)
        : [a] "s"(a), [b] "s"(b)
        : "scc");
    return r;
}

// Entry e of the cluster table at byte offset off (a 32-bit offset from the
// table's base keeps the per-entry address arithmetic to one SALU add).
__device__ __forceinline__ cv4f_t *cl_entry(cv4f_t *ct, uint32_t off) {
    return (cv4f_t *)((const __attribute__((address_space(4))) char *)ct + off);
}

// The member pairs [first, first + count) of an entered cluster: a sphere pair
// some lane may hit ORs its word-w bits into every word w of the wave's pair
// mask (rt_kernel.h: the entry's row of word w holds the bit or 0).  The walk is
// SALU-heavy (ballots, mask merges, loop control issue on the CU's one scalar
// unit): C5's member loop at 48 SALU per entry ran 17 % slower than at 34.
// wave[w] |= f ? bits[w] : 0 for every word under one compare of the ballot f:
// s_cselect_b64 per word (the compiler's lowering selects 32-bit halves, two
// per word) -- the merge runs on the CU's one scalar unit for every member.
template <int W>
__device__ __forceinline__ void merge_words(uint64_t (&wave)[kClWords], uint64_t f, const uint64_t (&bits)[W]) {
    uint64_t t0, t1;
    if constexpr (W == 2) {
        asm("s_cmp_lg_u64 %[f], 0\n\t"
            "s_cselect_b64 %[t0], %[b0], 0\n\t"
            "s_cselect_b64 %[t1], %[b1], 0\n\t"
            "s_or_b64 %[w0], %[w0], %[t0]\n\t"
            "s_or_b64 %[w1], %[w1], %[t1]"
            : [w0] "+s"(wave[0]), [w1] "+s"(wave[1]), [t0] "=&s"(t0), [t1] "=&s"(t1)
            : [f] "s"(f), [b0] "s"(bits[0]), [b1] "s"(bits[1])
            : "scc");
    } else {
        static_assert(W == 4, "pair-mask words");
        uint64_t t2, t3;
        asm("s_cmp_lg_u64 %[f], 0\n\t"
            "s_cselect_b64 %[t0], %[b0], 0\n\t"
            "s_cselect_b64 %[t1], %[b1], 0\n\t"
            "s_cselect_b64 %[t2], %[b2], 0\n\t"
            "s_cselect_b64 %[t3], %[b3], 0\n\t"
            "s_or_b64 %[w0], %[w0], %[t0]\n\t"
            "s_or_b64 %[w1], %[w1], %[t1]\n\t"
            "s_or_b64 %[w2], %[w2], %[t2]\n\t"
            "s_or_b64 %[w3], %[w3], %[t3]"
            : [w0] "+s"(wave[0]), [w1] "+s"(wave[1]), [w2] "+s"(wave[2]), [w3] "+s"(wave[3]), [t0] "=&s"(t0),
              [t1] "=&s"(t1), [t2] "=&s"(t2), [t3] "=&s"(t3)
            : [f] "s"(f), [b0] "s"(bits[0]), [b1] "s"(bits[1]), [b2] "s"(bits[2]), [b3] "s"(bits[3])
            : "scc");
    }
}

// One-word tables: wave |= (n0 & k0) ? bits0 : 0, then the same for member 1.  The
// lane-mask conjunction's own SCC (result != 0) feeds the 64-bit select, so a member
// costs and + select + or on the scalar unit (the compiler's lowering: and, compare,
// two 32-bit selects, or; C2 +1.6 % over it, profiles/r07a_scalar_diet_ab.txt).
// (x0, x1: the lanes that do not leave this member -- own_sphere below; one more conjunction each)
__device__ __forceinline__ void merge_word1(uint64_t &wave, uint64_t n0, uint64_t k0, uint64_t x0, uint64_t bits0,
                                            uint64_t n1, uint64_t k1, uint64_t x1, uint64_t bits1) {
    uint64_t t;
    asm("s_and_b64 %[t], %[n0], %[k0]\n\t"
        "s_and_b64 %[t], %[t], %[x0]\n\t"
        "s_cselect_b64 %[t], %[b0], 0\n\t"
        "s_or_b64 %[w], %[w], %[t]\n\t"
        "s_and_b64 %[t], %[n1], %[k1]\n\t"
        "s_and_b64 %[t], %[t], %[x1]\n\t"
        "s_cselect_b64 %[t], %[b1], 0\n\t"
        "s_or_b64 %[w], %[w], %[t]"
        : [w] "+&s"(wave), [t] "=&s"(t)
        : [n0] "s"(n0), [k0] "s"(k0), [x0] "s"(x0), [b0] "s"(bits0), [n1] "s"(n1), [k1] "s"(k1), [x1] "s"(x1),
          [b1] "s"(bits1)
        : "scc");
}
// (single lane masks: per-lane tables test no behind rule at the member level)
__device__ __forceinline__ void merge_word1(uint64_t &wave, uint64_t f0, uint64_t bits0, uint64_t f1, uint64_t bits1) {
    uint64_t t;
    asm("s_cmp_lg_u64 %[f0], 0\n\t"
        "s_cselect_b64 %[t], %[b0], 0\n\t"
        "s_or_b64 %[w], %[w], %[t]\n\t"
        "s_cmp_lg_u64 %[f1], 0\n\t"
        "s_cselect_b64 %[t], %[b1], 0\n\t"
        "s_or_b64 %[w], %[w], %[t]"
        : [w] "+&s"(wave), [t] "=&s"(t)
        : [f0] "s"(f0), [b0] "s"(bits0), [f1] "s"(f1), [b1] "s"(bits1)
        : "scc");
}

// an SGPR pointer the compiler cannot see through: loads through it stay where they are written
__device__ __forceinline__ cv4f_t *opaque(cv4f_t *p) {
    asm volatile("" : "+s"(p));
    return p;
}

// The per-lane thresholds of per-lane (REL) tables, both members of an entry
// per packed FMA.  The constants sit in VGPR pairs (kc = {kClRel, kBehindRel},
// kp = {kPfRel, kSlabRel}, aux = {slab_e0, |D.y|}) and op_sel broadcasts one
// half to both lanes: an f32 FMA with a literal and an SGPR row lowered to
// v_mov + v_fmamk, two VALU per threshold where this is half of one.  Every
// value is the same single-rounded FMA as fmaf, so the bits are unchanged.
struct ClConst {
    f2 kc, kp, aux;
};

// A constant in a VGPR, written where the walk starts: a plain constant is
// hoisted to the kernel's entry and held across every loop, which pushed other
// values into scratch.
__device__ __forceinline__ float walk_const(float c) {
    float r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "s"(c));
    return r;
}

// t = cc * kPfRel + r (a member pair's near-line thresholds)
__device__ __forceinline__ f2 member_thr(f2 cc, const ClConst &k, f2 r) {
    f2 t;
    asm("v_pk_fma_f32 %[t], %[cc], %[kp], %[r] op_sel_hi:[1,0,1]" : [t] "=v"(t) : [cc] "v"(cc), [kp] "v"(k.kp), [r] "s"(r));
    return t;
}

// A cluster pair's near-line thresholds t = cc kClRel + R, behind bounds
// b = beta - cc kBehindRel, and the height-slab distance d = |O.y + D.y T - ymid|
// (before the abs) with its limit thr = |D.y| srho + (yhalf + E),
// E = cc kSlabRel + slab_e0 (cluster_pair below).
__device__ __forceinline__ void cluster_thr(f2 cc, const ClConst &k, f2 r, f2 beta, f2 &t, f2 &b) {
    asm("v_pk_fma_f32 %[t], %[cc], %[kc], %[r] op_sel_hi:[1,0,1]\n\t"
        "v_pk_fma_f32 %[b], %[cc], %[kc], %[beta] op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[0,1,0] neg_hi:[0,1,0]"
        : [t] "=&v"(t), [b] "=&v"(b)
        : [cc] "v"(cc), [kc] "v"(k.kc), [r] "s"(r), [beta] "s"(beta));
}
__device__ __forceinline__ void cluster_slab(f2 cc, f2 T, const RayPk &ray, const ClConst &k, f2 srho, f2 ymid,
                                             f2 yhalf, f2 &d, f2 &thr) {
    asm("v_pk_fma_f32 %[thr], %[cc], %[kp], %[aux] op_sel:[0,1,0] op_sel_hi:[1,1,0]\n\t"
        "v_pk_add_f32 %[thr], %[yhalf], %[thr]\n\t"
        "v_pk_fma_f32 %[thr], %[aux], %[srho], %[thr] op_sel:[1,0,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %[d], %[ry], %[T], %[ry] op_sel:[1,0,0] op_sel_hi:[1,1,0]\n\t"
        "v_pk_add_f32 %[d], %[d], %[ymid] neg_lo:[0,1] neg_hi:[0,1]"
        : [thr] "=&v"(thr), [d] "=&v"(d)
        : [cc] "v"(cc), [kp] "v"(k.kp), [aux] "v"(k.aux), [yhalf] "s"(yhalf), [srho] "s"(srho), [ry] "v"(ray.y),
          [T] "v"(T), [ymid] "s"(ymid));
}

// The sphere a secondary ray leaves (scene-wide tables; rt_pack.cpp own_sphere_rho proves
// it).  The ray's origin lies on sphere j, so the near-line estimate always flags j and the
// behind rule never clears it (T >= -r against b < -r), yet the candidate is rejected: T - X < eps
// turns it into T + X ~ 0.  A lane proves that for itself from the ray it has: with C = RN(S_j - O)
// (the reference's own C_j, bit for bit), cc = |C|^2 and T = C.D as pair_prefilter forms them,
//   |RN(rho_j - cc kOwnCc)| < RN(-T kOwnLam)          rho_j = r_j^2, or +inf where nothing is proven
// shows that the reference's candidate j has T + X < eps: rejected under both rule sets whatever the
// running minima are.  Such a lane leaves slot j out of its own member flag (the value returned
// here; kOwnNone: no slot).  The wave's mask stays the union over lanes, and a lane still runs the
// exact test of j when another lane flags the pair, which reproduces the rejection.
// The test measures how far the origin lies off the sphere (rho - cc) rather than bounding it, so it
// assumes nothing about the segment that led here, only |D|^2 within 2^-16 of 1 (every prefiltered round).
constexpr uint32_t kOwnNone = 0xFFFFFFFFu;
constexpr float kOwnCc = 1.0f - 5.0f * 0x1p-18f;  // 1 - 1.25K: K T^2 and the roundings of dist, cc and X
constexpr float kOwnLam = 1.9e-4f;                // 1.9 eps of the 2 eps the square root's slope allows
__device__ __forceinline__ uint32_t own_sphere(const Sample &p, float4 sc, uint32_t slot) {
    const float cx = sc.x - p.rx.x, cy = sc.y - p.ry.x, cz = sc.z - p.rz.x;
    const float cc = __builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz));
    const float T = __builtin_fmaf(cz, p.rz.y, __builtin_fmaf(cy, p.ry.y, cx * p.rx.y));
    const float d = __builtin_fmaf(cc, -kOwnCc, sc.w);
    return __builtin_fabsf(d) < T * -kOwnLam ? slot : kOwnNone;
}

// own (scene-wide tables): the slot this lane's ray leaves and cannot accept (own_sphere), kOwnNone for none
// X: the expanded prefilter on the recentred table (pair_prefilter_x; scene-wide tables only)
// Lazy flags (scene-wide tables): an entry's load, prefilter and two near-line ballots n0, n1 run on every
// entry; the behind compares, the own-sphere compares and the merge only where some lane is near one of the
// two spheres, under one wave-uniform branch on n0 | n1 (any_lane).  58 % of C2's member-pair entries and
// 52 % of C5's have no near lane (profiles/r16a_near_share.txt) and then issue 2 v_cmp and the branch where
// they issued 6 v_cmp and the merge's 8 scalar instructions.
// Bit for bit the walk that runs all of it on every entry: member m's contribution to the wave mask is
// (n_m & k_m & x_m) != 0 ? bits_m : 0 with n, k, x the near, not-behind and not-own lane masks.  Where n0 == 0 and n1 == 0 both conjunctions
// are 0 whatever k and x are, so the skipped entry ORs nothing into the mask; where the branch is taken the
// code is the unconditional one.  The mask is the same, so the recheck walks the same pairs in the same order.
// Per-lane (REL) tables run the loop without the branch: their members test neither rule, the four-word form's
// f0 | f1 region is this branch already, and no measured workload runs the one- and two-word forms.
template <int W, bool REL, bool X>
__device__ __forceinline__ void member_pairs(cv4f_t *ct, uint32_t first, uint32_t count, const RayPk &ray, const RayX &rx,
                                             uint64_t (&wave)[kClWords], const ClConst &k, uint32_t own, PfStats *ps) {
    static_assert(!(X && REL), "the expanded prefilter is for scene-wide tables");
    constexpr uint32_t kEntryBytes = 16u * cl_entry_f4(W, REL);
    constexpr bool kLazy = !REL;
    if (ps) ps->groups += count;
    // (the end offset opaque to the optimiser: it otherwise derives a trip count and runs a
    // second, down-counting induction variable beside the offset -- one more SALU per entry)
    uint32_t end = (first + count) * kEntryBytes;
    asm volatile("" : "+s"(end));
    for (uint32_t off = first * kEntryBytes; off != end; off += kEntryBytes) {
        cv4f_t *e = cl_entry(ct, off);
        const Rows4 rows = load_rows4(e);  // (one scalar load per entry)
        const v4f_t r0 = rows.r0, r1 = rows.r1, r2 = rows.r2, r3 = rows.r3;
        f2 T, cc = {};
        const f2 v = X ? pair_prefilter_x(rx, f2{r0.x, r0.y}, f2{r0.z, r0.w}, f2{r1.x, r1.y}, T)
                       : pair_prefilter(ray, f2{r0.x, r0.y}, f2{r0.z, r0.w}, f2{r1.x, r1.y}, T, cc);
        // a lane may hit the sphere: near the line, and not wholly behind the origin
        const f2 tr = REL ? member_thr(cc, k, f2{r1.z, r1.w}) : f2{r1.z, r1.w};
        const float t0 = tr.x, t1 = tr.y;
        const float b0 = REL ? __builtin_fmaf(cc.x, -kBehindRel, r3.x) : r3.x;
        const float b1 = REL ? __builtin_fmaf(cc.y, -kBehindRel, r3.y) : r3.y;
        // Members of per-lane (REL) tables take the near-line test only: their behind
        // threshold is a per-lane FMA, and the rule stays at the cluster level
        // (RTWeekend +2.7 % same box; C2's scene-wide table loses 1.7 % without it).
        // Either way a skipped pair is a proven miss.
        constexpr bool kBehind = !REL;
        const uint64_t n0m = __builtin_amdgcn_ballot_w64(!(v.x >= t0)), n1m = __builtin_amdgcn_ballot_w64(!(v.y >= t1));
        if (ps) ps->near_entries += (n0m | n1m) != 0 ? 1u : 0u;
        if constexpr (kLazy) {
            if (!any_lane(n0m, n1m)) continue;
        }
        if constexpr (W == 1) {
            const uint64_t w0 = (uint64_t)__float_as_uint(r2.x) | ((uint64_t)__float_as_uint(r2.y) << 32);
            const uint64_t w1 = (uint64_t)__float_as_uint(r2.z) | ((uint64_t)__float_as_uint(r2.w) << 32);
            // (scene-wide tables: row 3 zw = the members' sphere slots, against the slot each lane leaves)
            if constexpr (kBehind)
                merge_word1(wave[0], n0m, __builtin_amdgcn_ballot_w64(!(T.x < b0)),
                            __builtin_amdgcn_ballot_w64(own != __float_as_uint(r3.z)), w0, n1m,
                            __builtin_amdgcn_ballot_w64(!(T.y < b1)),
                            __builtin_amdgcn_ballot_w64(own != __float_as_uint(r3.w)), w1);
            else
                merge_word1(wave[0], n0m, w0, n1m, w1);
        } else {
            const uint64_t f0m = kBehind ? n0m & __builtin_amdgcn_ballot_w64(!(T.x < b0)) &
                                               __builtin_amdgcn_ballot_w64(own != __float_as_uint(r3.z))
                                         : n0m;
            const uint64_t f1m = kBehind ? n1m & __builtin_amdgcn_ballot_w64(!(T.y < b1)) &
                                               __builtin_amdgcn_ballot_w64(own != __float_as_uint(r3.w))
                                         : n1m;
            if constexpr (W == 2) {
                uint64_t bw0[W], bw1[W];  // member 0 and 1 bits in word w
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const v4f_t rb = w == 0 ? r2 : e[3 + w];
                    bw0[w] = (uint64_t)__float_as_uint(rb.x) | ((uint64_t)__float_as_uint(rb.y) << 32);
                    bw1[w] = (uint64_t)__float_as_uint(rb.z) | ((uint64_t)__float_as_uint(rb.w) << 32);
                }
                merge_words<W>(wave, f0m, bw0);
                merge_words<W>(wave, f1m, bw1);
            } else {
                // four-word tables: a member's bit rows of words 1-3 are read only when some lane flagged it (a
                // uniform branch), so they do not hold 12 SGPRs across every entry's prefilter (RTWeekend
                // +0.7 %; the two-word form keeps its selects: C5 -0.5 % this way, profiles/r05u_lazy_bits_ab.txt);
                // word 0's row came with the entry's one load
                const bool f0 = f0m != 0, f1 = f1m != 0;
                if (f0 | f1) {
                    cv4f_t *eb = opaque(e);
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        const v4f_t rb = w == 0 ? r2 : eb[3 + w];
                        if (f0) wave[w] |= (uint64_t)__float_as_uint(rb.x) | ((uint64_t)__float_as_uint(rb.y) << 32);
                        if (f1) wave[w] |= (uint64_t)__float_as_uint(rb.z) | ((uint64_t)__float_as_uint(rb.w) << 32);
                    }
                }
            }
        }
    }
}

// One cluster-pair entry (both levels of the table share the row layout):
// the wave's lanes that may reach cluster 0 / 1 (near the line, not wholly
// behind the origin, and for per-lane tables inside the height slab).
// Height slab (per-lane tables): the line's height over the t range that can
// reach the cluster is c +- |D.y| srho with c = O.y + D.y T; it cannot meet a
// member when that range clears [ymid - yhalf, ymid + yhalf] by the lane's
// margin E (a ground-plane scene: rays leaving the ground cross the thin layer
// of small spheres only near their origin).
// (The sub-level slab and behind tests stay: without them RTWeekend -0.1 % and -3 %, profiles/r06n_slab_ab.txt.)
template <bool REL, bool X>
__device__ __forceinline__ void cluster_pair(cv4f_t *e, const RayPk &ray, const RayX &rx, const ClConst &k, uint64_t &m0,
                                             uint64_t &m1, v4f_t &ranges, PfStats *ps) {
    const Rows4 rows = load_rows4(e);  // (one scalar load per entry; row 2 = the entry's ranges)
    const v4f_t r0 = rows.r0, r1 = rows.r1, r3 = rows.r3;
    ranges = rows.r2;
    f2 T, cc = {};
    const f2 v = X ? pair_prefilter_x(rx, f2{r0.x, r0.y}, f2{r0.z, r0.w}, f2{r1.x, r1.y}, T)
                   : pair_prefilter(ray, f2{r0.x, r0.y}, f2{r0.z, r0.w}, f2{r1.x, r1.y}, T, cc);
    // (near: the entry's two near-line lane masks, for the diagnostic build's count alone -- the behind compares and the
    // slab block stay on every entry: under a branch on the near masks C2 and RTWeekend both lost, DESIGN_HISTORY)
    if constexpr (REL) {
        f2 t, b;
        cluster_thr(cc, k, f2{r1.z, r1.w}, f2{r3.x, r3.y}, t, b);
        if (ps) ps->cl_near_entries += (__ballot(!(v.x >= t.x)) | __ballot(!(v.y >= t.y))) != 0 ? 1u : 0u;
        m0 = ballot_and(!(v.x >= t.x), !(T.x < b.x));
        m1 = ballot_and(!(v.y >= t.y), !(T.y < b.y));
        const v4f_t r4 = e[4];
        f2 d, thr;
        cluster_slab(cc, T, ray, k, f2{r3.z, r3.w}, f2{r4.x, r4.y}, f2{r4.z, r4.w}, d, thr);
        m0 &= __builtin_amdgcn_ballot_w64(!(__builtin_fabsf(d.x) > thr.x));
        m1 &= __builtin_amdgcn_ballot_w64(!(__builtin_fabsf(d.y) > thr.y));
    } else {
        if (ps) ps->cl_near_entries += (__ballot(!(v.x >= r1.z)) | __ballot(!(v.y >= r1.w))) != 0 ? 1u : 0u;
        m0 = ballot_and(!(v.x >= r1.z), !(T.x < r3.x));
        m1 = ballot_and(!(v.y >= r1.w), !(T.y < r3.y));
    }
}

// ps (RTK_STATS): groups += member-pair entries tested, pairs += sphere pairs
// rechecked exactly, lane_pairs += clusters entered (per wave, both levels),
// cl_tested += cluster-pair entries tested (both levels), cl_top_entered += top
// clusters entered (two-level tables).
// Tables of two or more mask words (more than 32 groups) have two levels: a
// top cluster's entry ranges index sub-cluster entries of a few spheres each,
// whose ranges index the member entries (rt_pack.cpp lay_out); the bound
// of a cluster covers every sphere under it, so a skipped top cluster skips
// its sub-clusters' members too.
// X: the walk-specialised scene-wide kernels' expanded prefilter (pair_prefilter_x): a.clusters is then
// the recentred table, whose first row holds its centre c0, in front of entry 0 (rt_pack.cpp expand_table;
// rt_kernel.h kPrefilterExpanded is the launch fact).
template <bool SIMD, int W, bool GS, bool REL, bool X = false>
__device__ __forceinline__ void clustered_groups(const TraceArgs &a, const float4 *lds_groups, const RayPk &ray,
                                                 Hit &h, bool fast, uint32_t own, PfStats *ps) {
    // (X: a.clusters names the row {c0, 0}, entry 0 the row behind it -- one more immediate offset of
    // every entry's load, where a row in front of the table cost an address pair of its own)
    cv4f_t *ct = (cv4f_t *)a.clusters + (X ? 1 : 0);
    uint64_t wave[kClWords] = {0ull, 0ull, 0ull, 0ull};
    constexpr uint32_t kEntryBytes = 16u * cl_entry_f4(W, REL);
    constexpr bool kTwoLevels = W >= 2;
    // per-lane part of the height-slab margin (REL tables; rt_pack.cpp per_lane_bounds)
    const float oy = ray.y.x, dy = ray.y.y;
    const float slab_e0 = REL ? __builtin_fmaf(__builtin_fabsf(oy), 0x1p-21f, kSlabRel) : 0.0f;
    ClConst k;
    if constexpr (REL) {
        k.kc = f2{walk_const(kClRel), walk_const(kBehindRel)};
        k.kp = f2{walk_const(kPfRel), walk_const(kSlabRel)};
        k.aux = f2{slab_e0, __builtin_fabsf(dy)};
    }
    RayX rx = {};
    if constexpr (X) rx = ray_expand(ray, *(cv4f_t *)a.clusters);
    // the member pairs of an entered (sub-)cluster pair entry
    auto members = [&](v4f_t r2, bool in0, bool in1) {
        if (ps) ps->lane_pairs += (in0 ? 1u : 0u) + (in1 ? 1u : 0u);
        if (in0) member_pairs<W, REL, X>(ct, __float_as_uint(r2.x), __float_as_uint(r2.y), ray, rx, wave, k, own, ps);
        if (in1) member_pairs<W, REL, X>(ct, __float_as_uint(r2.z), __float_as_uint(r2.w), ray, rx, wave, k, own, ps);
    };
    // the sub-cluster pair entries [first, first + count) of an entered top cluster
    auto subs = [&](uint32_t first, uint32_t count) {
        if (ps) ps->cl_tested += count;
        for (uint32_t off = first * kEntryBytes, end = (first + count) * kEntryBytes; off != end; off += kEntryBytes) {
            cv4f_t *e = cl_entry(ct, off);
            uint64_t m0, m1;
            v4f_t r2;
            cluster_pair<REL, X>(e, ray, rx, k, m0, m1, r2, ps);
            members(r2, m0 != 0, m1 != 0);
        }
    };
    if (ps) ps->cl_tested += a.n_cpairs;
    // (every caller walks a table of at least one cluster-pair entry -- the run-time kernel tests
    // n_cpairs, the walk kernels are launched with one only: no zero-trip test in front of the loop)
    uint32_t off = 0;
    const uint32_t end = a.n_cpairs * kEntryBytes;
    do {
        cv4f_t *e = cl_entry(ct, off);
        uint64_t m0, m1;
        v4f_t r2;
        cluster_pair<REL, X>(e, ray, rx, k, m0, m1, r2, ps);
        if constexpr (kTwoLevels) {
            if (ps) ps->lane_pairs += (m0 != 0 ? 1u : 0u) + (m1 != 0 ? 1u : 0u);
            if (ps) ps->cl_top_entered += (m0 != 0 ? 1u : 0u) + (m1 != 0 ? 1u : 0u);
            if (m0 != 0) subs(__float_as_uint(r2.x), __float_as_uint(r2.y));
            if (m1 != 0) subs(__float_as_uint(r2.z), __float_as_uint(r2.w));
        } else {
            members(r2, m0 != 0, m1 != 0);
        }
        off += kEntryBytes;
    } while (off != end);
    cv4f_t *gp = (cv4f_t *)a.groups;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        uint64_t m = wave[w];
        while (m) {
            const uint32_t q = (uint32_t)__builtin_ctzll(m) & ~1u;  // first pair of the lowest flagged group
            const uint32_t g = 32u * (uint32_t)w + (q >> 1);
            // (both flags from one shift, each a 32-bit bit test; the 64-bit tests of bits q and q + 1
            // cost a shift, a mask and a 64-bit compare apiece on the scalar unit)
            const uint32_t pp = (uint32_t)(m >> q);
            const bool f01 = (pp & 1u) != 0u, f23 = (pp & 2u) != 0u;
            m &= ~(3ull << q);
            if (ps) ps->pairs += (f01 ? 1u : 0u) + (f23 ? 1u : 0u);
            recheck_pairs<SIMD>(a, load_group_exact_at(gp + kGroupF4 * g), g, ray, h, fast, f01, f23);
        }
    }
}

// The direction walk (kWalkCl1Dir: one-word scene-wide tables; rt_pack.cpp direction_table proves it, rt_layout.h
// has the block's layout).  In place of the cluster level -- five cluster-pair entries and the member entries of
// every cluster some lane may reach -- each lane of the round reads the pair mask of (the sphere its ray leaves,
// the cell of its direction), the wave ORs the masks of the round's lanes, and only the member entries of that
// union run the member test, entry p of the block being the sphere pair p.  The table only chooses the entries:
// the member test (near line, behind, own sphere), the wave mask it builds and the recheck in group order are
// those of member_pairs<1, false, true> and clustered_groups.  A pair outside a lane's mask is a proven miss for
// that lane, a pair outside the union one for every lane of the round, so the wave mask loses only pairs no lane
// of the round can accept and every accepted candidate is what it was.
// row: the slot the lane's ray leaves where the lane has measured that its origin lies on that sphere
// (origin_near), else kOwnNone: the lane then asks for every pair.
// The table's premise (c): |O - S_j| <= 1.008 r_j, measured as own_sphere measures its own rule, on the same
// cc (the compiler forms it once): |RN(rho_j - cc kOwnCc)| < RN(rho_j 2^-6); false for rho_j = +inf or NaN.
__device__ __forceinline__ bool origin_near(const Sample &p, float4 sc) {
    const float cx = sc.x - p.rx.x, cy = sc.y - p.ry.x, cz = sc.z - p.rz.x;
    const float cc = __builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz));
    return __builtin_fabsf(__builtin_fmaf(cc, -kOwnCc, sc.w)) < sc.w * 0x1p-6f;
}

// The OR of v over the active lanes, in an SGPR, as a fixed reduction: no loop, no branch.  A round runs under
// exec = the round's lanes, and a butterfly under partial exec loses words (lanes 0 and 3 alone: lane 0 reads
// lanes 1 and 2, which computed nothing -- a value cannot pass through an inactive lane).  So the block
// enables every lane, takes the word as 0 outside the saved exec mask, ORs within each row of 16 lanes by the
// four DPP controls of trace_kernel's parked_frontier (lane ^ 1, lane ^ 2, the other quad of the half row, the
// other half of the row), reads one lane per row and puts exec back.  Only t, the block's own register, is
// written while the inactive lanes are enabled.  Wait states inside the block: a VALU write of t, then a DPP
// read of t: 2 (s_nop 1); then the lane reads: 1 (s_nop 0).
// WIDE: both words of a 64-bit mask in the same all-lanes region (the second word's DPP step is one of the
// first's two wait states).
template <bool WIDE>
__device__ __forceinline__ uint64_t wave_or(uint32_t lo, uint32_t hi) {
    uint64_t keep;
    uint32_t t, u, r1, r2, r3;
    if constexpr (!WIDE) {
        asm volatile(
            "s_or_saveexec_b64 %[keep], -1\n\t"
            "v_cndmask_b32_e64 %[t], 0, %[v], %[keep]\n\t"
            "s_nop 1\n\t"
            "v_or_b32_dpp %[t], %[t], %[t] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "s_nop 1\n\t"
            "v_or_b32_dpp %[t], %[t], %[t] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "s_nop 1\n\t"
            "v_or_b32_dpp %[t], %[t], %[t] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
            "s_nop 1\n\t"
            "v_or_b32_dpp %[t], %[t], %[t] row_mirror row_mask:0xf bank_mask:0xf\n\t"
            "s_nop 0\n\t"
            "v_readlane_b32 %[u], %[t], 0\n\t"
            "v_readlane_b32 %[r1], %[t], 16\n\t"
            "v_readlane_b32 %[r2], %[t], 32\n\t"
            "v_readlane_b32 %[r3], %[t], 48\n\t"
            "s_mov_b64 exec, %[keep]\n\t"
            "s_or_b32 %[u], %[u], %[r1]\n\t"
            "s_or_b32 %[r2], %[r2], %[r3]\n\t"
            "s_or_b32 %[u], %[u], %[r2]"
            : [keep] "=&s"(keep), [t] "=&v"(t), [u] "=&s"(u), [r1] "=&s"(r1), [r2] "=&s"(r2), [r3] "=&s"(r3)
            : [v] "v"(lo)
            : "scc");
        return (uint64_t)u;
    } else {
        uint32_t t1, u1, q1, q2, q3;
        asm volatile(
            "s_or_saveexec_b64 %[keep], -1\n\t"
            "v_cndmask_b32_e64 %[t], 0, %[v], %[keep]\n\t"
            "v_cndmask_b32_e64 %[t1], 0, %[w], %[keep]\n\t"
            "s_nop 0\n\t"
            "v_or_b32_dpp %[t], %[t], %[t] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_or_b32_dpp %[t1], %[t1], %[t1] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "s_nop 0\n\t"
            "v_or_b32_dpp %[t], %[t], %[t] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_or_b32_dpp %[t1], %[t1], %[t1] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "s_nop 0\n\t"
            "v_or_b32_dpp %[t], %[t], %[t] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
            "v_or_b32_dpp %[t1], %[t1], %[t1] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
            "s_nop 0\n\t"
            "v_or_b32_dpp %[t], %[t], %[t] row_mirror row_mask:0xf bank_mask:0xf\n\t"
            "v_or_b32_dpp %[t1], %[t1], %[t1] row_mirror row_mask:0xf bank_mask:0xf\n\t"
            "s_nop 0\n\t"
            "v_readlane_b32 %[u], %[t], 0\n\t"
            "v_readlane_b32 %[r1], %[t], 16\n\t"
            "v_readlane_b32 %[r2], %[t], 32\n\t"
            "v_readlane_b32 %[r3], %[t], 48\n\t"
            "v_readlane_b32 %[u1], %[t1], 0\n\t"
            "v_readlane_b32 %[q1], %[t1], 16\n\t"
            "v_readlane_b32 %[q2], %[t1], 32\n\t"
            "v_readlane_b32 %[q3], %[t1], 48\n\t"
            "s_mov_b64 exec, %[keep]\n\t"
            "s_or_b32 %[u], %[u], %[r1]\n\t"
            "s_or_b32 %[r2], %[r2], %[r3]\n\t"
            "s_or_b32 %[u], %[u], %[r2]\n\t"
            "s_or_b32 %[u1], %[u1], %[q1]\n\t"
            "s_or_b32 %[q2], %[q2], %[q3]\n\t"
            "s_or_b32 %[u1], %[u1], %[q2]"
            : [keep] "=&s"(keep), [t] "=&v"(t), [t1] "=&v"(t1), [u] "=&s"(u), [r1] "=&s"(r1), [r2] "=&s"(r2),
              [r3] "=&s"(r3), [u1] "=&s"(u1), [q1] "=&s"(q1), [q2] "=&s"(q2), [q3] "=&s"(q3)
            : [v] "v"(lo), [w] "v"(hi)
            : "scc");
        return (uint64_t)u | ((uint64_t)u1 << 32);
    }
}

// The diagnostic build's count alone (RTK_STATS lane_pairs): the trips of the union loop wave_or replaced, in
// which the lowest lane with bits still missing from the union added its word until none had any.  The walk
// itself runs on wave_or's word.
__device__ __forceinline__ uint32_t wave_or_trips(uint32_t v) {
    uint32_t u = 0u, trips = 0u;
    for (;;) {
        const uint64_t b = __builtin_amdgcn_ballot_w64(v != 0u);
        if (b == 0ull) break;
        u |= (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_ctzll(b));
        v &= ~u;
        trips += 1u;
    }
    return trips;
}

// The member entries of the union `todo`, in pair order (member_pairs<1, false, true>'s body on each): the pairs
// some lane of the round may accept, as the wave mask of clustered_groups' recheck.  M: the mask's own width,
// uint32_t up to 32 pairs -- a 32-bit find, one bit cleared and a 32-bit test per entry -- else uint64_t.
// todo != 0 (every lane's own-pair bit is set): the loop is entered without a test.
template <typename M>
__device__ __forceinline__ uint64_t direction_members(cv4f_t *members, const RayX &rx, uint32_t own, M todo, PfStats *ps) {
    uint64_t wave = 0ull;
    __builtin_assume(todo != 0);
    do {
        uint32_t pr;
        if constexpr (sizeof(M) == 4) {
            pr = (uint32_t)__builtin_ctz(todo);
            // (todo &= ~(1u << pr) compiles to a shift and an and-not)
            asm("s_bitset0_b32 %0, %1" : "+s"(todo) : "s"(pr));
        } else {
            pr = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
        }
        const Rows4 er = load_rows4(cl_entry(members, pr * (16u * cl_entry_f4(1u))));
        const v4f_t r0 = er.r0, r1 = er.r1, r2 = er.r2, r3 = er.r3;
        f2 T;
        const f2 v = pair_prefilter_x(rx, f2{r0.x, r0.y}, f2{r0.z, r0.w}, f2{r1.x, r1.y}, T);
        const uint64_t n0m = __builtin_amdgcn_ballot_w64(!(v.x >= r1.z)), n1m = __builtin_amdgcn_ballot_w64(!(v.y >= r1.w));
        if (ps) ps->near_entries += (n0m | n1m) != 0 ? 1u : 0u;
        if (!any_lane(n0m, n1m)) continue;
        const uint64_t w0 = (uint64_t)__float_as_uint(r2.x) | ((uint64_t)__float_as_uint(r2.y) << 32);
        const uint64_t w1 = (uint64_t)__float_as_uint(r2.z) | ((uint64_t)__float_as_uint(r2.w) << 32);
        merge_word1(wave, n0m, __builtin_amdgcn_ballot_w64(!(T.x < r3.x)),
                    __builtin_amdgcn_ballot_w64(own != __float_as_uint(r3.z)), w0, n1m,
                    __builtin_amdgcn_ballot_w64(!(T.y < r3.y)), __builtin_amdgcn_ballot_w64(own != __float_as_uint(r3.w)), w1);
    } while (todo != 0);
    return wave;
}

// The union of the round's lanes' masks and the member entries of it.  WIDE: 64-bit masks (more than 16 groups).
template <bool WIDE>
__device__ __forceinline__ uint64_t direction_union_walk(const TraceArgs &a, cv4f_t *members, const uint32_t *rows,
                                                         uint32_t idx, bool near, const RayX &rx, uint32_t own, PfStats *ps) {
    uint32_t lo, hi = 0u;
    if constexpr (WIDE) {
        const uint2 m = ((const uint2 *)rows)[idx];
        lo = m.x;
        hi = m.y;
        if (!near) {  // every pair there is an entry for
            const uint32_t n_pairs = 2u * a.n_groups;
            const uint64_t every = n_pairs >= 64u ? ~0ull : (1ull << n_pairs) - 1ull;
            lo = (uint32_t)every, hi = (uint32_t)(every >> 32);
        }
    } else {
        lo = rows[idx];
        if (!near) lo = 0xFFFFFFFFu >> (32u - 2u * a.n_groups);  // (1 <= n_groups <= 16)
    }
    const uint64_t todo = wave_or<WIDE>(lo, hi);
    if (ps) {
        const uint64_t far = __builtin_amdgcn_ballot_w64(!near);
        ps->lane_pairs += wave_or_trips(lo) + (WIDE ? wave_or_trips(hi) : 0u);
        ps->groups += (uint32_t)__builtin_popcountll(todo);
        ps->cl_top_entered += far != 0ull ? 1u : 0u, ps->cl_tested += (uint32_t)__builtin_popcountll(far);
    }
    if constexpr (WIDE) return direction_members<uint64_t>(members, rx, own, todo, ps);
    else return direction_members<uint32_t>(members, rx, own, (uint32_t)todo, ps);
}

// ps (RTK_STATS): groups += member entries tested, near_entries as in member_pairs, pairs += sphere pairs
// rechecked exactly, lane_pairs += trips of the union loop (wave_or_trips); no cluster entry is tested, and the
// two cluster counters count the origin measurement instead: cl_top_entered += rounds with a lane that asks for
// every pair, cl_tested += such lanes.
// WIDE: the table's masks are 64 bits wide (dir_mask64(a.n_groups): the host routes by it, rtk_walk_kernel).
template <bool SIMD, bool WIDE>
__device__ __forceinline__ void direction_groups(const TraceArgs &a, const RayPk &ray, Hit &h, bool fast, uint32_t own,
                                                 uint32_t row, PfStats *ps) {
    const v4f_t c0 = *(cv4f_t *)a.clusters;
    const uint32_t at = __float_as_uint(c0.w);  // the block's offset in rows (rt_layout.h)
    cv4f_t *members = (cv4f_t *)a.clusters + at;
    // the lane's mask: row < 4 n_groups (a sphere the lane has hit) and cell < kDirCells (dir_cell clamps)
    const bool near = row != kOwnNone;
    // (the clamp costs one instruction and keeps the gather inside the table whatever a lane carries)
    const uint32_t idx = (near ? min(row, 4u * a.n_groups - 1u) : 0u) * kDirCells + dir_cell(ray.x.y, ray.y.y, ray.z.y);
    const uint32_t *rows = (const uint32_t *)(a.clusters + at + dir_member_f4(a.n_groups));
    const RayX rx = ray_expand(ray, c0);
    // (the mask's width is a fact of the kernel -- rt_kernel.h kWalkCl1Dir / kWalkCl1Dir64 -- so a round tests it
    // nowhere: as a run-time choice it was structurised into mask form around the gather and the walk)
    uint64_t wave = direction_union_walk<WIDE>(a, members, rows, idx, near, rx, own, ps);
    // (clustered_groups' recheck of a one-word mask)
    cv4f_t *gp = (cv4f_t *)a.groups;
    while (wave) {
        const uint32_t q = (uint32_t)__builtin_ctzll(wave) & ~1u;
        const uint32_t g = q >> 1;
        const uint32_t pp = (uint32_t)(wave >> q);
        const bool f01 = (pp & 1u) != 0u, f23 = (pp & 2u) != 0u;
        wave &= ~(3ull << q);
        if (ps) ps->pairs += (f01 ? 1u : 0u) + (f23 ? 1u : 0u);
        recheck_pairs<SIMD>(a, load_group_exact_at(gp + kGroupF4 * g), g, ray, h, fast, f01, f23);
    }
}

// All four spheres of group g; one wave-level branch per group, nested
// branches only for the (rare) lanes that pass the distance test.
template <bool SIMD>
__device__ __forceinline__ void test_group(const TraceArgs &a, const Group &G, uint32_t g, const RayPk &p, Hit &h, bool fast,
                                           uint32_t *hit_groups) {
    f2 T01, T23;
    const f2 d01 = pair_dist(p, f2{G.x[0], G.x[1]}, f2{G.y[0], G.y[1]}, f2{G.z[0], G.z[1]}, T01);
    const f2 d23 = pair_dist(p, f2{G.x[2], G.x[3]}, f2{G.y[2], G.y[3]}, f2{G.z[2], G.z[3]}, T23);
    bool h0, h1, h2, h3;
    if (SIMD) {  // HitMask = d < r^2 (main.cpp:409)
        h0 = d01.x < G.r2[0];
        h1 = d01.y < G.r2[1];
        h2 = d23.x < G.r2[2];
        h3 = d23.y < G.r2[3];
    } else {  // !(d > r^2) over the Count real spheres only (main.cpp:547,557)
        const uint32_t s0 = 4u * g;
        h0 = s0 + 0u < a.n_spheres && !(d01.x > G.r2[0]);
        h1 = s0 + 1u < a.n_spheres && !(d01.y > G.r2[1]);
        h2 = s0 + 2u < a.n_spheres && !(d23.x > G.r2[2]);
        h3 = s0 + 3u < a.n_spheres && !(d23.y > G.r2[3]);
    }
    if (hit_groups && __ballot(h0 | h1 | h2 | h3)) *hit_groups += 1;
    if (h0 | h1 | h2 | h3) {
        if (h0) candidate<SIMD, 0>(h, g, T01.x, d01.x, G.r2[0], fast);
        if (h1) candidate<SIMD, 1>(h, g, T01.y, d01.y, G.r2[1], fast);
        if (h2) candidate<SIMD, 2>(h, g, T23.x, d23.x, G.r2[2], fast);
        if (h3) candidate<SIMD, 3>(h, g, T23.y, d23.y, G.r2[3], fast);
    }
}

// pair_dist for rays that all start at the camera (primary rounds): C = S - O
// is the same on every lane, so its three packed subtractions come from the
// cull pass's table (TraceArgs.prim, computed with the same single f32
// rounding) and the C operands stay in SGPRs -- 16 packed ops instead of 19.
__device__ __forceinline__ f2 pair_dist_c(const RayPk &r, f2 cx, f2 cy, f2 cz, f2 &T) {
    f2 qx, qy, qz, t, d;
    asm("v_pk_mul_f32 %[t], %[cx], %[rx] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %[d], %[cy], %[ry] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[T], %[t], %[d]\n\t"
        "v_pk_mul_f32 %[t], %[cz], %[rz] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[T], %[T], %[t]\n\t"
        "v_pk_mul_f32 %[t], %[rx], %[T] op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[qx], %[cx], %[t] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t], %[ry], %[T] op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[qy], %[cy], %[t] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[t], %[rz], %[T] op_sel:[1,0] op_sel_hi:[1,1]\n\t"
        "v_pk_add_f32 %[qz], %[cz], %[t] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[d], %[qx], %[qx]\n\t"
        "v_pk_mul_f32 %[t], %[qy], %[qy]\n\t"
        "v_pk_add_f32 %[d], %[d], %[t]\n\t"
        "v_pk_mul_f32 %[t], %[qz], %[qz]\n\t"
        "v_pk_add_f32 %[d], %[d], %[t]"
        : [qx] "=&v"(qx), [qy] "=&v"(qy), [qz] "=&v"(qz), [t] "=&v"(t), [T] "=&v"(T), [d] "=&v"(d)
        : [cx] "s"(cx), [cy] "s"(cy), [cz] "s"(cz), [rx] "v"(r.x), [ry] "v"(r.y), [rz] "v"(r.z));
    return d;
}

// One sphere pair of a primary round (spheres L0, L0 + 1 of group g, camera-relative rows from
// TraceArgs.prim): test_group's two halves as separate pair tests.
template <bool SIMD, int L0>
__device__ __forceinline__ void test_half_prim(const TraceArgs &a, uint32_t g, const RayPk &p, Hit &h, bool fast, f2 cx, f2 cy,
                                               f2 cz, float r2a, float r2b) {
    f2 T;
    const f2 d = pair_dist_c(p, cx, cy, cz, T);
    bool ha, hb;
    if (SIMD) {  // HitMask = d < r^2 (main.cpp:409)
        ha = d.x < r2a;
        hb = d.y < r2b;
    } else {  // !(d > r^2) over the Count real spheres only (main.cpp:547,557)
        const uint32_t s0 = 4u * g + (uint32_t)L0;
        ha = s0 < a.n_spheres && !(d.x > r2a);
        hb = s0 + 1u < a.n_spheres && !(d.y > r2b);
    }
    if (ha | hb) {
        if (ha) candidate<SIMD, L0>(h, g, T.x, d.x, r2a, fast);
        if (hb) candidate<SIMD, L0 + 1>(h, g, T.y, d.y, r2b, fast);
    }
}

// Pair pr of a primary round's pair mask (half pr & 1 of group pr >> 1); the mask's pairs come in
// ascending order, the reference's sphere order, so the per-class minima and tie rules are those of
// the full group loop.
template <bool SIMD>
__device__ __forceinline__ void test_pair_prim(const TraceArgs &a, cv4f_t *prim, uint32_t pr, const RayPk &p, Hit &h, bool fast) {
    const uint32_t g = pr >> 1;
    cv4f_t *pg = prim + kPrimF4 * g;
    const v4f_t cx = pg[0], cy = pg[1], cz = pg[2], r2 = pg[3];
    if (pr & 1u) test_half_prim<SIMD, 2>(a, g, p, h, fast, f2{cx.z, cx.w}, f2{cy.z, cy.w}, f2{cz.z, cz.w}, r2.z, r2.w);
    else test_half_prim<SIMD, 0>(a, g, p, h, fast, f2{cx.x, cx.y}, f2{cy.x, cy.y}, f2{cz.x, cz.y}, r2.x, r2.y);
}

}  // namespace rtk
