// rt_layout.h — the memory the host packs (rt_pack.cpp) and the kernels read (rtk_*.h): sphere groups,
// sphere records and the clustered prefilter tables.  Plain C++, no HIP: the packer builds as a host
// program (tests/pack_check).  Internal; not part of include/.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr uint32_t kGroupF4 = 5;      // float4 rows per sphere group:
constexpr uint32_t kRowX = 0, kRowY = 1, kRowZ = 2;  //   centres
constexpr uint32_t kRowR2 = 3;        //   r*r (rows 0-3 = one s_load_dwordx16: all the exact test reads)
constexpr uint32_t kRowR2P = 4;       //   prefilter thresholds (the per-group prefilter loop only)
constexpr uint32_t kSphereF4 = 4;     // float4 rows per sphere record (TraceArgs.materials)
// Clustered secondary-ray prefilter (rt_pack.cpp cluster_table): entries of
// cl_entry_f4(W) float4 rows, read through the scalar cache --
//   cluster pair c : {qx0 qx1 qy0 qy1} {qz0 qz1 rc2p0 rc2p1} {first0 count0 first1 count1} {b0 b1 0 0} [padding]
//   member pair m  : {x0 x1 y0 y1}     {z0 z1 r2p0 r2p1}     {word-0 bits of member 0 (lo, hi), of member 1}
//                    {b0 b1 slot0 slot1}  then one row per further word w = 1 .. W-1: {word-w bits of member 0, of member 1}
// (slot = the member's sphere slot 4*group + lane as a u32, scene-wide tables only (else 0): a lane that has
// proven it cannot accept the sphere its ray leaves drops that slot from its own flags -- rtk_walk.h own_sphere)
// (b = behind threshold: a lane whose prefilter T = (centre - O).D is below
// it cannot accept any member -- rt_pack.cpp behind_of_slot, cluster_bounds)
// (first/count index member-pair entries; a member's pair q = sphere slot >> 1
// is its sphere pair in group order, the bit it sets in the wave's pair mask).
// The wave mask is kept in SGPRs, W = cl_words u64 words of it (1: n_groups <= 32,
// 2: <= 64, 4: <= 128): member k's pair q sets bit q & 63 of word q >> 6, and its
// entry holds that bit in the row of word q >> 6 and 0 in the others, so the kernel
// merges a flagged member into every word with one select and one OR each.
// With pf_relative the thresholds are per lane: rc2p / r2p hold R_c / r^2 and
// b the M-free behind bases (rt_pack.cpp cluster_bounds, "relative"), and a
// cluster pair also carries its height-slab bound (rtk_walk.h cluster_slab):
//   row 3 = {b0 b1 srho0 srho1}, row 4 = {ymid0 ymid1 yhalf0 yhalf1}
// (entries then have at least 5 rows; member entries leave row 4 to the bits).
// padding members: threshold -inf, bits 0.
constexpr uint32_t cl_entry_f4(uint32_t words, bool relative = false) {
    return words == 1u ? (relative ? 5u : 4u) : 3u + words;
}
// The float offsets of the fields above inside one entry; h = the half of the pair (0 or 1).
constexpr uint32_t cl_centre(uint32_t axis, uint32_t h) { return 2u * axis + h; }  // q / sphere centre, axis 0-2
constexpr uint32_t cl_threshold(uint32_t h) { return 6u + h; }                     // rc2p / r2p
constexpr uint32_t cl_first(uint32_t h) { return 8u + 2u * h; }                    // cluster pair: the range of
constexpr uint32_t cl_count(uint32_t h) { return 9u + 2u * h; }                    //   entries under the cluster
constexpr uint32_t kClRowBits0 = 2;                                                // member pair: row of the word-0 bits
constexpr uint32_t cl_behind(uint32_t h) { return 12u + h; }                       // b
constexpr uint32_t cl_slot(uint32_t h) { return 14u + h; }                         // member pair, scene-wide tables
constexpr uint32_t cl_srho(uint32_t h) { return 14u + h; }                         // cluster pair, per-lane tables:
constexpr uint32_t cl_ymid(uint32_t h) { return 16u + h; }                         //   the height slab
constexpr uint32_t cl_yhalf(uint32_t h) { return 18u + h; }
// member pair: where the row of mask word w starts (member h's u64 at + 2h, low half first)
constexpr uint32_t cl_bits(uint32_t word) { return 4u * (word == 0u ? kClRowBits0 : 3u + word); }
constexpr float kSlabRel = 0x1p-9f;  // the slab test's per-lane margin per unit of cc (rt_pack.cpp cluster_bounds)
constexpr uint32_t kClMaxGroups = 128;   // table built up to this many groups
constexpr uint32_t kClAutoGroups = 128;  // used by default up to this many (rt_plan.h Switches.clusters; RTWeekend's
                                         // 121 groups: 11.3k Mrays/s clustered against 9.4k per group)

// The direction table of a one-word scene-wide table (rt_pack.cpp direction_table; rtk_walk.h direction_groups):
// per sphere slot j and direction cell, the mask of the sphere pairs a ray that leaves ball j in a direction of
// that cell can be accepted on, in the layout of the wave's pair mask (bit p: spheres 2p, 2p + 1).  Masks are
// u32 for a scene of at most 32 pairs (16 groups), else u64; row j holds kDirCells of them.
// In front of the rows lie the member entries in PAIR order: entry p = the member pair {2p, 2p + 1} in the
// recentred form of the expanded table (the rows of a member pair above, thresholds and behind bounds copied
// from that table's own entry of each sphere), so that entry p is 4 p rows from the block's start.
// On the device the block follows the expanded table in the same buffer, and word 3 of that table's first row
// {c0, .} holds the block's offset from the row in float4 units (0: no block): TraceArgs does not grow.
// The cell of a direction D with |D|^2 within 2^-16 of 1: the face is D's largest component by magnitude and
// its sign (x wins ties over y over z), and the two other components a, b -- each at most sqrt((1 + 2^-16)/2) <
// kDirSpan in magnitude -- index a kDirN x kDirN grid over [-kDirSpan, kDirSpan]^2 as they are: no division, no
// reciprocal.  Every operation is an IEEE f32 compare, FMA, floor or clamp, so host and device agree bit for
// bit, and the host bounds a cell by the preimage of the index arithmetic itself (rt_pack.cpp cell_cone).
#if defined(__HIPCC__)
#define RT_LAYOUT_HD __host__ __device__
#else
#define RT_LAYOUT_HD
#endif
constexpr uint32_t kDirN = 16;  // cells per face edge (rt_pack.cpp direction_table has the measurement)
constexpr uint32_t kDirCells = 6u * kDirN * kDirN;
constexpr float kDirSpan = 0.7072f;
constexpr float kDirScale = (float)kDirN / (2.0f * kDirSpan), kDirHalf = 0.5f * (float)kDirN;
constexpr uint32_t kDirMaxGroups = 32;  // one mask word: at most 128 spheres
RT_LAYOUT_HD inline uint32_t dir_cell_axis(float v) {
    const float t = __builtin_floorf(__builtin_fmaf(v, kDirScale, kDirHalf));
    return (uint32_t)__builtin_fminf(__builtin_fmaxf(t, 0.0f), (float)(kDirN - 1u));
}
RT_LAYOUT_HD inline uint32_t dir_cell(float dx, float dy, float dz) {
    const float ax = __builtin_fabsf(dx), ay = __builtin_fabsf(dy), az = __builtin_fabsf(dz);
    const bool fx = ax >= ay && ax >= az, fy = !fx && ay >= az;
    const float m = fx ? dx : fy ? dy : dz;
    const float a = fx ? dy : dx, b = (fx || fy) ? dz : dy;
    const uint32_t face = (fx ? 0u : fy ? 2u : 4u) + (m < 0.0f ? 1u : 0u);
    return (face * kDirN + dir_cell_axis(a)) * kDirN + dir_cell_axis(b);
}
// float4 rows of the block's member entries, and the block's size in floats
constexpr uint32_t dir_member_f4(uint32_t n_groups) { return 2u * n_groups * cl_entry_f4(1u); }
constexpr bool dir_mask64(uint32_t n_groups) { return n_groups > 16u; }
constexpr size_t dir_block_floats(uint32_t n_groups) {
    return 4u * (size_t)dir_member_f4(n_groups) + 4u * (size_t)n_groups * kDirCells * (dir_mask64(n_groups) ? 2u : 1u);
}

// HBM layout of an uploaded scene (per rule set):
//   groups    : n_groups x 5 float4 = {x[4]}, {y[4]}, {z[4]}, {r*r[4]}, {r2p[4]}  (80 B/group)
//               rows 0-3 are what an exact test reads (the cluster walk's recheck: one scalar load);
//               r2p = prefilter threshold of the secondary-ray sphere loop (rt_pack.cpp prefilter_rows);
//               with pf_relative, r*r again (-inf: never hit) and the threshold is formed per lane
//   spheres   : 4*n_groups records of kSphereF4 float4 = {centre.xyz, rho}, {Color.xyz, Specular},
//               {Emissive.xyz, IOR}, {1/IOR, r0 outside, r0 inside, 0} (dielectrics; else 0)
//               rho = r*r where the own-sphere rule applies to the sphere, +inf where it is off
//               (rt_pack.cpp own_sphere_rho; rt_scene_own_sphere reports it)
//               (64 B/sphere: what shading gathers for the winning sphere,
//               addressed by one shift of its index; TraceArgs.materials)
// r*r is precomputed on the host with the same f32 multiply the reference
// repeats per test (main.cpp:406), so it is bit-identical.

// The largest scene a device takes (the primary cull masks are rtk_mask_words(kMaxGroups) = 128 words
// per wave tile; rt_kernel.h kMaxLdsGroups: how much of that the LDS image holds).
static const uint32_t kMaxGroups = 4096u;                                                    // 16,384 spheres
