// rtk_trace.h — CDNA4 (gfx950) trace kernel for the brute-force sphere path.
//
// Replaces the reference's tile callback RenderTile / RenderTileScalar
// (main.cpp:348-495 / 497-640) and its lane-4 math layer (x64_math.h,
// base.h:474-887).  A wave owns a small pixel tile with P lanes per pixel;
// each lane traces its pixel's samples k = j, j+P, ... and the pixel's owner
// lane folds every finished sample into the running mean strictly in sample
// order, so the result is bit-identical to one thread per pixel folding all
// of this launch's frames.  The reference's 4-wide SIMD lanes become the four
// per-residue-class minima each lane carries.
//
// Exactness: rtk_math.h.
//
// Work shape: lanes alternate between starting primary rays
// and gathering secondary segments (a hit is shaded at the start of the segment
// it feeds: the trip loop's comment); primary rays test only the sphere groups
// their tile's cone can reach (tiles whose cone reaches none fold their
// samples without tracing); secondary rays run an FMA prefilter with a proven
// error bound and re-test exactly only the sphere pairs it flags.  Sphere
// groups are wave-uniform: read through the scalar cache into SGPRs (SRC_SMEM)
// or, for A/B, from the block's LDS copy (SRC_LDS); per-lane gathers (winning
// sphere, material, r^2 of flagged groups, rsqrt table) hit the LDS copy.
#pragma once
#include "rtk_shape.h"
#include "rtk_walk.h"

namespace rtk {

// Scheduling counters (RT_STATS=1) are compiled in only with -DRTK_STATS
// (the diagnostic build, `make variant NAME=stats KFLAGS=-DRTK_STATS`): the
// production kernel carries no per-trip checks for them.
#ifdef RTK_STATS
constexpr bool kStats = true;
#else
constexpr bool kStats = false;
#endif

// The counters of one wave (rt_kernel.h kStat*; RT_STATS gives the launch a.stats).  TraceStats<false>,
// the production build, is empty: every call of it in trace_kernel compiles to nothing.
template <bool ON>
struct TraceStats {
    __device__ __forceinline__ explicit TraceStats(const unsigned long long *) {}
    __device__ __forceinline__ void setup_end() {}
    __device__ __forceinline__ void cull_end() {}
    __device__ __forceinline__ void sync_end() {}
    __device__ __forceinline__ void post_end() {}
    __device__ __forceinline__ void trip_begin() {}
    __device__ __forceinline__ void trip_end(bool, uint32_t) {}
    __device__ __forceinline__ void fold_begin() {}
    __device__ __forceinline__ void fold_end() {}
    __device__ __forceinline__ void round(uint32_t, uint64_t, uint64_t, uint32_t, bool) {}
    __device__ __forceinline__ void primary_mask(uint64_t) {}
    __device__ __forceinline__ void exact_round(float) {}
    __device__ __forceinline__ PfStats *pf_round() { return nullptr; }
    __device__ __forceinline__ uint32_t *sec_hit() { return nullptr; }
    __device__ __forceinline__ void flush(unsigned long long *, uint32_t) {}
};

template <>
struct TraceStats<true> {
    bool on;  // the launch collects them (a.stats set)
    uint32_t pri_it = 0, pri_lanes = 0, sec_it = 0, sec_lanes = 0, groups = 0, sec_hit_groups = 0;
    uint32_t sparse_it = 0, sparse_lanes = 0, tail_it = 0;
    uint32_t pri_blocked = 0, pri_waitsec = 0, pri_done = 0;
    uint32_t sec_done = 0, sec_waitpri = 0, done_trips = 0, done_lanes = 0;
    uint32_t sec_exact = 0, sec_badlanes = 0, sec_zerodir = 0, pf_rounds = 0;
    PfStats pf = {0, 0, 0, 0, 0, 0, 0};
    uint64_t cyc_pri = 0, cyc_sec = 0, cyc_fold = 0, cyc_setup = 0, cyc_cull = 0, cyc_sync = 0, cyc_post = 0;
    uint64_t t_entry = 0, t_setup = 0, t_cull = 0, t_sync = 0, t_trip = 0, t_fold = 0;  // clock readings

    __device__ __forceinline__ uint64_t now() const { return on ? __builtin_amdgcn_s_memtime() : 0; }
    __device__ __forceinline__ explicit TraceStats(const unsigned long long *stats) : on(stats != nullptr) { t_entry = now(); }
    // the kernel's head: LDS image loads issued and tile picked | cull mask read | barrier | empty-tile fold
    __device__ __forceinline__ void setup_end() { t_setup = now(); }
    __device__ __forceinline__ void cull_end() { t_cull = now(); }
    __device__ __forceinline__ void sync_end() { t_sync = now(); }
    __device__ __forceinline__ void post_end() {
        if (!on) return;
        cyc_setup = t_setup - t_entry;
        cyc_cull = t_cull - t_setup;
        cyc_sync = t_sync - t_cull;
        cyc_post = now() - t_sync;
    }
    // A traced trip's cycles go to the kind of its round.  The shade of a hit runs at the start of the
    // round that continues the path, so cyc_sec holds every shade with the walk (merged rounds: cyc_pri,
    // as all of their trips), and cyc_pri is sample start, pair tests, hit select and the park alone.
    __device__ __forceinline__ void trip_begin() { t_trip = now(); }
    __device__ __forceinline__ void trip_end(bool traced, uint32_t do_sec) {
        const uint64_t t = now();
        if (on && traced) (do_sec != 0u ? cyc_sec : cyc_pri) += t - t_trip;
    }
    __device__ __forceinline__ void fold_begin() { t_fold = now(); }
    __device__ __forceinline__ void fold_end() {
        if (on) cyc_fold += __builtin_amdgcn_s_memtime() - t_fold;
    }
    // one traced round (every lane active): its lanes, and where the other lanes are
    __device__ __forceinline__ void round(uint32_t do_sec, uint64_t pri, uint64_t sec, uint32_t mode, bool can_start) {
        if (!on) return;
        if (do_sec) { sec_it += 1; sec_lanes += __builtin_popcountll(sec); }
        if (do_sec && __builtin_popcountll(sec) < 16) { sparse_it += 1; sparse_lanes += __builtin_popcountll(sec); }
        if (do_sec && __ballot(mode == 0u) == 0) tail_it += 1;  // no lane has a sample to start
        if (do_sec) {  // a secondary round: where the other lanes are
            sec_done += __builtin_popcountll(__ballot(mode == 2u));
            sec_waitpri += __builtin_popcountll(__ballot(mode == 0u));
        }
        // trips with finished pixels (every sample started and traced) beside live ones
        const uint32_t nd = __builtin_popcountll(__ballot(mode == 2u));
        if (nd) { done_trips += 1; done_lanes += nd; }
        if (!do_sec) {  // a primary round: where the other lanes are
            pri_it += 1;
            pri_lanes += __builtin_popcountll(pri);
            pri_blocked += __builtin_popcountll(__ballot(mode == 0u && !can_start));
            pri_waitsec += __builtin_popcountll(sec);
            pri_done += __builtin_popcountll(__ballot(mode == 2u));
        }
    }
    // a word of the primary round's pair mask
    __device__ __forceinline__ void primary_mask(uint64_t m) {
        if (on) groups += __builtin_popcountll(m);
    }
    // a secondary round that left the prefilter's |D|^2 bound (u2 = the lane's |D|^2) and ran the exact loop
    __device__ __forceinline__ void exact_round(float u2) {
        if (!on) return;
        sec_exact += 1;
        sec_badlanes += __builtin_popcountll(__ballot(!(__builtin_fabsf(1.0f - u2) <= kPfDirTol)));
        sec_zerodir += __builtin_popcountll(__ballot(u2 == 0.0f));
    }
    // a prefiltered secondary round: counted, and the walk's own counters
    __device__ __forceinline__ PfStats *pf_round() {
        if (!on) return nullptr;
        pf_rounds += 1;
        return &pf;
    }
    __device__ __forceinline__ uint32_t *sec_hit() { return on ? &sec_hit_groups : nullptr; }
    __device__ __forceinline__ void flush(unsigned long long *stats, uint32_t lane) {
        if (!on || lane != 0) return;
        // rt_debug_stats has 32 slots and every one is taken: a -DRTK_STATS -DRTK_STATS_NEAR build reports the walk's
        // near-entry counts in the slots of the exact rounds' two lane counts (sec_badlanes: pf_near_entries,
        // member-pair entries with a near lane; sec_zerodir: cl_near_entries, the same of cluster-pair entries)
#ifdef RTK_STATS_NEAR
        const uint32_t s_bad = pf.near_entries, s_zero = pf.cl_near_entries;
#else
        const uint32_t s_bad = sec_badlanes, s_zero = sec_zerodir;
#endif
        const struct { uint32_t slot; unsigned long long v; } out[] = {
            {kStatPriIters, pri_it}, {kStatPriLanes, pri_lanes}, {kStatSecIters, sec_it}, {kStatSecLanes, sec_lanes},
            {kStatPriGroups, groups}, {kStatSecHitGroups, sec_hit_groups}, {kStatSecSparseIters, sparse_it},
            {kStatSecSparseLanes, sparse_lanes}, {kStatSecTailIters, tail_it}, {kStatPriCycles, cyc_pri},
            {kStatSecCycles, cyc_sec}, {kStatFoldCycles, cyc_fold}, {kStatSetupCycles, cyc_setup},
            {kStatCullCycles, cyc_cull}, {kStatSyncCycles, cyc_sync}, {kStatPostCycles, cyc_post},
            {kStatPfRounds, pf_rounds}, {kStatPfGroups, pf.groups}, {kStatClTested, pf.cl_tested},
            {kStatPfPairs, pf.pairs}, {kStatClTopEntered, pf.cl_top_entered}, {kStatPfLanePairs, pf.lane_pairs},
            {kStatPriBlocked, pri_blocked}, {kStatPriWaitSec, pri_waitsec}, {kStatPriDone, pri_done},
            {kStatSecDone, sec_done}, {kStatSecWaitPri, sec_waitpri}, {kStatDoneTrips, done_trips},
            {kStatDoneLaneTrips, done_lanes}, {kStatSecExact, sec_exact}, {kStatSecBadLanes, s_bad},
            {kStatSecZeroDir, s_zero}};
        for (const auto &o : out) atomicAdd(stats + o.slot, o.v);
    }
};

// Tile of this block: heaviest-first order from the previous launch's
// measured costs when the host supplies one (tile_order), so the long
// waves do not start last and form the launch's tail.  One-wave kernels
// rank waves (unit 4 * tile + quadrant), four-wave ones block tiles.
template <bool SOLO, typename Args>
__device__ __forceinline__ void wave_unit(const Args &a, uint32_t tid, uint32_t &tile, uint32_t &wave) {
    if (SOLO && a.unit_waves != 0u) {
        const uint32_t u = a.tile_order ? a.tile_order[blockIdx.x] : blockIdx.x;
        tile = u >> 2;
        wave = u & 3u;
    } else {
        const uint32_t blk = SOLO ? blockIdx.x >> 2 : blockIdx.x;
        tile = a.tile_order ? a.tile_order[blk] : blk;
        wave = SOLO ? blockIdx.x & 3u : tid >> 6;
    }
}

// GS: the scene (groups + materials) stays in HBM and per-lane gathers read it
// through the caches (scenes beyond the LDS image, or RT_SCENE_GLOBAL=1).
// SOLO: one wave per workgroup (block b traces quadrant b & 3 of block tile
// tile_order[b >> 2]).  A 4-wave workgroup's slots are held until its last wave
// ends, and a new workgroup needs four free slots at once: at C2 about a fifth
// of the wave slots sat idle mid-launch (scripts/wave_tail.py).  A one-wave
// workgroup is replaced as soon as it ends.  It keeps no LDS image (the scene
// and both tables are read through the caches, measured as fast at C2), only
// its ring and mask.
// WALK: the secondary-ray sphere walk compiled into the kernel (rt_kernel.h
// kWalk*): every variant selected at run time (kWalkAny), the per-group loops
// only (kWalkGroups), or one cluster walk (pair-mask words, per-lane or
// scene-wide thresholds).  One walk per kernel keeps the code and the SGPR
// pressure of the others out of the trace loop (C2 +4 % with only the W = 1
// walk compiled in).  The exact all-groups loop stays in every variant (rounds
// whose directions leave the prefilter's |D|^2 bound).
// WALKF: the walk, and with kWalkTileCounts OR'ed in the per-tile counts variant (rt_trace_tile_work):
// once the wave knows its block tile it takes the {PreviousRayCount, Frames} pair of the reference
// tile around it from the table rtk_tile_counts(a) (scalar loads) and overwrites its by-value a.prev_count /
// a.frames; nothing after that point differs.  The flag is off in every kWalk* value, so the kernels
// of uniform launches are the ones they were, symbol and code.
template <bool SIMD, int SRC, bool CULL, int P, bool GS, bool SOLO = false, int WALKF = kWalkAny>
__global__ __launch_bounds__(SOLO ? 64 : 256, SOLO ? solo_waves(WALKF & kWalkMask) : SRC == kSrcSmem ? RTK_MIN_WAVES_PER_SIMD : 1)
void trace_kernel(TraceArgs a) {
    constexpr int WALK = WALKF & kWalkMask;
    constexpr bool kTileCounts = (WALKF & kWalkTileCounts) != 0;
    static_assert(!GS || SRC == kSrcSmem, "a scene in HBM is read through the scalar cache");
    static_assert(!SOLO || GS, "a one-wave workgroup keeps no LDS image");
    constexpr uint32_t kWB = SOLO ? 1u : (uint32_t)kWavesPerBlock;  // waves (LDS slots) per workgroup
    constexpr uint32_t TW = Shape<P>::TW, TH = Shape<P>::TH, LP = Shape<P>::LP, Q = Shape<P>::Q;
    constexpr uint32_t NPIX = 64u / LP;  // pixels traced at a time
    constexpr bool kMergeable = Walk<WALK>::MERGEABLE;
    constexpr uint32_t kRing = Ring<LP>::N;
    // The candidate square root (candidate<>): a walk-specialised one-wave kernel is launched only for
    // scenes whose r^2 range the host proved (rt_kernel.h rtk_walk_kernel), so it holds sqrt_rn alone --
    // no flag test and no IEEE body at its candidate sites.  Every other kernel tests the flag
    // (C2 +0.6 % to +1.4 % over the flag tested at every site: profiles/r07a_scalar_diet_ab.txt, "ab" against "new").
    constexpr bool kFastSqrt = SOLO && WALK != kWalkAny;
    const bool fast = kFastSqrt || a.fast_sqrt != 0u;
    // Launch facts, by the same routing (rt_kernel.h rtk_walk_kernel lists them and why): max_bounce >= 1,
    // frames >= 1 and, for a cluster walk, a non-empty table over a non-empty scene.  Tested inside the
    // trip loop these were lane masks held in SGPRs across it (four of them spilled to VGPR lanes); the
    // run-time kernel (kWalkAny) keeps every test (C2 +2.8 %: profiles/r08a_trip_header_ab.txt, "facts").
    constexpr bool kFacts = SOLO && WALK != kWalkAny;
    if constexpr (kFacts) {
        __builtin_assume(a.max_bounce != 0u);
        __builtin_assume(a.frames != 0u);
        if constexpr (Walk<WALK>::CLUSTERS) {
            __builtin_assume(a.n_cpairs != 0u);
            __builtin_assume(a.n_groups != 0u);
        }
    }
    const bool bounces = kFacts || a.max_bounce != 0u;  // (false: nothing is traced, every frame folds black)
    extern __shared__ float4 smem[];
    // first launch of a key: the host has not read the live-tile count back, so
    // the grid covers every tile (live first) and blocks past the count leave
    if (a.live_total && (SOLO ? blockIdx.x >> 2 : blockIdx.x) >= (uint32_t)*a.live_total) return;
    if constexpr (kTileCounts) {
        // The block tile's own counts.  Taken first: the fold table below is filled from a.prev_count,
        // and every later reader (the mean's load, the sample hand-out, the weights, the fold and the ray
        // count) sees the pair as if the launch had carried it.  The block tile is workgroup-uniform
        // (wave_unit: one tile per four-wave workgroup, one wave per one-wave workgroup) and lies in one
        // reference tile (rtk_shape.h), as do a pixel-sorted wave's pixels and a P = 0 lane's four.
        uint32_t t0, w0;
        wave_unit<SOLO>(a, threadIdx.x, t0, w0);
        const uint32_t rt = (((t0 / a.tiles_x) * (2u * Shape<P>::TH)) / kRefTile) * a.sel_tiles_x +
                            ((t0 % a.tiles_x) * (2u * Shape<P>::TW)) / kRefTile;
        const uint32_t *pair = a.sel + a.tile_counts_at + 2u * rt;  // (rtk_tile_counts: the host launches these kernels with a table)
        a.prev_count = (uint32_t)__builtin_amdgcn_readfirstlane((int)pair[0]);
        a.frames = (uint32_t)__builtin_amdgcn_readfirstlane((int)pair[1]);
        // A resting tile (rt_trace_tile_counts: a listed tile whose device entry folds no frame) leaves
        // here, before any barrier, LDS fill or store: the block tile is workgroup-uniform, so every wave
        // of the workgroup takes the branch.  A launch that measures costs still needs one from this
        // unit -- the sort zeroed it, and cost 0 ranks with the dead tiles behind the live prefix the
        // next grid covers -- so it gets the smallest a launched unit can have (the end of the kernel).
        // Its pixels' costs (pix_cost) stay those of the tile's last traced launch.
        if (a.frames == 0u) {
            if (a.tile_cost && (threadIdx.x & 63u) == 0u) {
                if (SOLO && a.unit_waves != 0u)
                    a.tile_cost[4u * t0 + w0] = 1u;
                else
                    atomicMax(a.tile_cost + t0, 1u);
            }
            return;
        }
        // (so every tile that stays has Frames >= 1: the launch fact of the walk kernels holds per tile)
        if constexpr (SOLO && WALK != kWalkAny) __builtin_assume(a.frames != 0u);
    }
    TraceStats<kStats> st(a.stats);  // (the -DRTK_STATS build's counters; empty otherwise)
    // LDS image: [rsqrt table 512 float4][fold table 128 float4]
    //            [groups kGroupF4*n_groups float4][sphere records kSphereF4*4*n_groups float4]
    // the wave tile's primary group mask: one-wave workgroups keep no LDS image,
    // so theirs is the dynamic LDS the host sizes to the scene's words (static
    // kMaxGroups / 64 words would cost 512 B of every workgroup's allocation)
    __shared__ uint64_t s_mask_st[SOLO ? 1 : kWB][SOLO ? 1 : MaskWords<GS>::N];
    uint64_t *const s_maskw = SOLO ? reinterpret_cast<uint64_t *>(smem) : s_mask_st[SOLO ? 0u : threadIdx.x >> 6];
    // ring slot s of pixel pl at s * kRingStride + pl: the sample lanes of a
    // pixel (different slots) fall on different LDS banks (stride NPIX + 1)
    constexpr uint32_t kRingStride = NPIX + 1u;
    __shared__ float4 s_ring[LP > 1 ? kWB * kRing * kRingStride : 1];
    // (one-wave kernels keep no LDS image: both tables are theirs from HBM at compile time, so the
    // rsqrt gather is a global load with a scalar base, not a flat one through a selected pointer)
    const bool lut_lds = !SOLO && a.lut_in_lds != 0u;
    const uint32_t lut_f4 = lut_lds ? 512u : 0u;  // see rtk_lds_bytes
    const Lut lut = {reinterpret_cast<const float *>(smem), a.rsqrt_lut, lut_lds};
    float2 *fold = reinterpret_cast<float2 *>(smem + lut_f4);
    // running-mean weights of the first kFoldTable frames (large scenes: none, computed per sample)
    const uint32_t fold_n = !SOLO && a.fold_in_lds ? kFoldTable : 0u;
    float4 *lds_groups = smem + lut_f4 + fold_n / 2;
    float4 *lds_mats = lds_groups + kGroupF4 * a.n_groups;
    // per-lane gathers of the winner's centre and material: LDS image or HBM (GS)
    const float4 *mat_src = GS ? a.materials : lds_mats;
    {
        const float4 *glut = reinterpret_cast<const float4 *>(a.rsqrt_lut);
        for (uint32_t i = threadIdx.x; i < lut_f4; i += blockDim.x) smem[i] = glut[i];
        if (!GS) {
            for (uint32_t i = threadIdx.x; i < kGroupF4 * a.n_groups; i += blockDim.x) lds_groups[i] = a.groups[i];
            for (uint32_t i = threadIdx.x; i < 4u * kSphereF4 * a.n_groups; i += blockDim.x) lds_mats[i] = a.materials[i];
        }
        // running-mean weights of frame k (main.cpp:484-487): 1/(p+1), p/(p+1)
        for (uint32_t i = threadIdx.x; i < fold_n; i += blockDim.x) {
            const uint32_t pc = a.prev_count + i;
            fold[i] = make_float2(1.0f / (float)(pc + 1u), (float)pc / (float)(pc + 1u));
        }
    }

    // wave: quadrant of the block tile; sw: the wave's LDS slot in its workgroup
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t sw = SOLO ? 0u : tid >> 6;
    uint32_t tile, wave;
    wave_unit<SOLO>(a, tid, tile, wave);
    const uint32_t tile_x = tile % a.tiles_x, tile_y = tile / a.tiles_x;
    // The wave's start times go to memory and LDS, and the end of the kernel re-derives its tile
    // (wave_unit through the kernarg segment): nothing of the bookkeeping is held in SGPRs across the
    // trip loop, where the four-word walk spilled it around every secondary round.
    __shared__ uint64_t s_cost0[SOLO ? 1 : kWB];
    if (a.wave_times && lane == 0) a.wave_times[2u * ((uint64_t)tile * 4u + wave)] = __builtin_amdgcn_s_memrealtime();
    if (a.tile_cost && lane == 0) s_cost0[sw] = __builtin_amdgcn_s_memtime();
    st.setup_end();
    const uint32_t pl = lane / LP, j = lane % LP;  // pixel of the tile, sample lane of the pixel
    // wave tile: a TW x TH quadrant of the block tile, or (interleave) every
    // other pixel and row of the whole block tile, parity (wave & 1, wave >> 1);
    // Q > 1: pixel slot q of the lane is pixel pl of the tile's 8x8 quadrant q
    auto pixel_x = [&](uint32_t q) -> uint32_t {
        if (Q > 1) return tile_x * (2u * TW) + (wave & 1u) * TW + (pl & 7u) + 8u * (q & 1u);
        return a.interleave ? tile_x * (2u * TW) + 2u * (pl % TW) + (wave & 1u)
                            : tile_x * (2u * TW) + (wave & 1u) * TW + pl % TW;
    };
    auto pixel_ly = [&](uint32_t q) -> uint32_t {
        if (Q > 1) return tile_y * (2u * TH) + (wave >> 1) * TH + (pl >> 3) + 8u * (q >> 1);
        return a.interleave ? tile_y * (2u * TH) + 2u * (pl / TW) + (wave >> 1)
                            : tile_y * (2u * TH) + (wave >> 1) * TH + pl / TW;
    };
    uint32_t q_slot = 0;  // Q > 1: the lane's current pixel slot
    uint32_t x = pixel_x(0), ly = pixel_ly(0);
    bool valid = x < a.width && ly < a.local_rows;
    // (slot 0 outside the image puts every slot of the lane outside it: the
    // slots lie right of and below slot 0)
    auto global_y = [&](uint32_t l) -> uint32_t {
        return ((l / a.band_rows) * a.band_count + a.band_index) * a.band_rows + l % a.band_rows;
    };
    uint32_t y = global_y(ly);
    // pixels dealt to the block's waves by cost (rtk_launch_pixel_sort): wave-uniform
    const uint8_t *perm = Q == 1 && a.pix_perm && !a.interleave ? a.pix_perm + (size_t)tile * 64u : nullptr;
    const bool permuted = perm && perm[0] != 0xFFu;
    if (permuted) {
        const uint32_t li = perm[wave * NPIX + pl];
        x = tile_x * (2u * TW) + li % (2u * TW);
        ly = tile_y * (2u * TH) + li / (2u * TW);
        valid = x < a.width && ly < a.local_rows;
        y = global_y(ly);
    }
    const bool owner = j == 0;
    // The running mean of a pixel is one sequential chain per colour channel, so
    // with P >= 4 its lanes j = 0, 1, 2 each fold ONE channel (kept in accx) in
    // lockstep: a fold step then costs one multiply and one add per lane, and a
    // wave folds 3 chains per pixel at once (at P = 16 the owner's three-channel
    // fold was ~15 % of the wave's VALU instructions).  The owner gathers the
    // other two channels by DPP for the final store.
    constexpr bool FOLD3 = LP >= 4;
    const bool folder = FOLD3 ? j < 3u : owner;
    // the channel a lane reads from a ring slot (lanes j >= 3 of the whole-batch fold
    // read the ratio word and discard their sums)
    const uint32_t jc = j < 3u ? j : 3u;
    // every lane of a pixel keeps the fold cursor (whole-batch frontier fold)
    constexpr bool kCursorPerLane = LP > 1;
    float4 *ring = s_ring + sw * kRing * kRingStride + pl;

    const uint32_t n_words = rtk_mask_words(a.n_groups);
    if constexpr (kFacts && Walk<WALK>::CLUSTERS) __builtin_assume(n_words != 0u);  // (n_groups >= 1)
    // the wave tile's primary pair mask, from the cull pass (rtk_launch_cull)
    // (a permuted wave's pixels come from all four quadrants: the union of their masks)
    if (CULL)
        for (uint32_t wd = lane; wd < n_words; wd += 64u) {
            uint64_t m = a.masks[((size_t)tile * 4u + wave) * n_words + wd];
            if (permuted)
                for (uint32_t q = 0; q < 4u; ++q) m |= a.masks[((size_t)tile * 4u + q) * n_words + wd];
            s_maskw[wd] = m;
        }
    st.cull_end();
    __syncthreads();
    st.sync_end();

    float accx = 0.0f, accy = 0.0f, accz = 0.0f;  // FOLD3: accx = this folding lane's channel j
    // the running mean so far of the lane's current pixel (main.cpp:485)
    auto load_mean = [&]() {
        accx = accy = accz = 0.0f;
        if (valid && folder && a.prev_count > 0 && !(a.flags & kFlagAccumZero)) {
            const float4 pv = a.prev[(size_t)ly * a.width + x];
            if (FOLD3) {
                accx = j == 0u ? pv.x : j == 1u ? pv.y : pv.z;
            } else {
                accx = pv.x;
                accy = pv.y;
                accz = pv.z;
            }
        }
    };
    load_mean();
    // the blended mean and its RGBA8 (main.cpp:488-492) of the current pixel
    // (Q > 1 stores inside the trace loop, where the f64 pow of RT_FLAG_SRGB_POW
    // would cost registers: the host launches that flag with Q = 1 only)
    auto store_pixel = [&]() {
        const size_t pix = (size_t)ly * a.width + x;
        a.prev[pix] = make_float4(accx, accy, accz, 1.0f);
        if (!a.skip_cur) a.cur[pix] = rgba8(accx, accy, accz, Q == 1 && (a.flags & kFlagSrgbPow) != 0u);
    };

    // owner lanes of in-image pixels (they fold until every frame is folded)
    const uint64_t folding = ballot_and(owner, valid);
    // lane mode: 0 = next sample pending, 1 = path continues (a pending hit to shade, then its secondary
    // segment), 2 = no samples left
    // The P lanes of a pixel take its samples in order as they free up (kDynamic):
    // each trip the lanes wanting a sample are ranked inside the slice and take
    // next, next + 1, ...  A lane whose samples run short no longer idles while its
    // neighbours trace theirs: only the pixel's last few samples leave lanes idle.
    constexpr bool kDynamic = LP > 1;
    uint32_t k = j;            // this lane's next (or current) sample
    uint32_t next = 0;         // kDynamic: the pixel's first unassigned sample (same on its lanes)
    uint32_t folded = 0;       // owner: samples folded so far
    uint32_t mode = (valid && k < a.frames) ? 0u : 2u;
    const uint32_t slice_base = lane - j;

    uint64_t nrays = 0;  // wave total (uniform): segments traced by this wave
    uint32_t pseg = 0;   // segments this lane traced (pix_cost)
    Sample p;
    p.bounce = 0;
    p.cx = p.cy = p.cz = 0.0f;

    // Empty tile: no sphere group passes the tile's (conservative) cone test,
    // so every primary ray of every sample misses; without a sky term each
    // sample's Out is exactly 0 (main.cpp:433-440), its one segment still
    // counts (main.cpp:390), and its blend is Final = 0*(1/n) + Prev*((n-1)/n)
    // = RN(Prev*((n-1)/n)) -- folded here without generating the rays.
    bool empty_tile = CULL && !a.use_sky && bounces;
    if (CULL)
        for (uint32_t w = 0; w < n_words; ++w) empty_tile = empty_tile && s_maskw[w] == 0;
    // (an all-zero running mean stays exactly zero: nothing to fold)
    auto fold_zero_frames = [&]() {
        if (valid && folder && (accx != 0.0f || accy != 0.0f || accz != 0.0f)) {
            for (uint32_t q = 0; q < a.frames; ++q) {
                float ratio;
                if (q < fold_n) {
                    ratio = fold[q].y;
                } else {
                    ratio = fold_weights(a.prev_count + q).y;
                }
                accx = 0.0f + accx * ratio;
                accy = 0.0f + accy * ratio;
                accz = 0.0f + accz * ratio;
            }
        }
    };
    if (empty_tile) {
        if (Q > 1) {  // every pixel slot of the lane, each stored here
            for (uint32_t q = 0; q < Q; ++q) {
                if (q > 0) {
                    x = pixel_x(q);
                    ly = pixel_ly(q);
                    valid = x < a.width && ly < a.local_rows;
                    load_mean();
                }
                fold_zero_frames();
                nrays += (uint64_t)__builtin_popcountll(__ballot(valid)) * a.frames;
                if (valid) store_pixel();
            }
            valid = false;  // (nothing left for the final store)
        } else {
            fold_zero_frames();
            nrays = (uint64_t)__builtin_popcountll(__ballot(valid && owner)) * a.frames;
        }
        folded = a.frames;
        mode = 2u;
    }

    st.post_end();
    // A mode-1 lane's pending hit: the accepted hit of the segment p still describes (its tmin, and
    // the winning class's key as it stands: the sphere index with the inside flag in bit 31, rtk_walk.h
    // Hit), shaded at the start of the lane's next round.
    // Read only in mode 1 and written on every way into it, so a lane that finishes a sample (or a
    // Q > 1 lane moving to its next pixel slot) carries none over.
    float pend_t = 0.0f;
    uint32_t pend_s = 0u;
    uint32_t dir_row = kOwnNone;  // (kWalkCl1Dir: written by shade_hit, read by the same round's walk)
    // Re-derive the winner's HitNormal / NextRayOrigin exactly as they were
    // formed at acceptance (main.cpp:423-429), then shade and bounce.
    // Returns the slot the continued ray leaves and cannot accept (rtk_walk.h own_sphere: formed from the
    // centre row loaded here and the ray shade has just made), for the kernels that hold a scene-wide
    // cluster walk; kOwnNone in every other kernel, which computes nothing for it.
    constexpr bool kOwnRule = Walk<WALK>::CLUSTERS ? !Walk<WALK>::REL : WALK == kWalkAny;
    auto shade_hit = [&](float tmin, uint32_t sidx, bool inside) -> uint32_t {
        // the winner's record (rt_kernel.h kSphereF4): one shift of the sphere index addresses its
        // centre and both material rows
        const float4 *rec = mat_src + kSphereF4 * sidx;
        const float4 sc = rec[0];
        const float sx = sc.x, sy = sc.y, sz = sc.z;
        const float cx = sx - p.rx.x, cy = sy - p.ry.x, cz = sz - p.rz.x;
        const float ipx = p.rx.y * tmin, ipy = p.ry.y * tmin, ipz = p.rz.y * tmin;
        const float hx = ipx - cx, hy = ipy - cy, hz = ipz - cz;
        p.rx.x = p.rx.x + ipx;
        p.ry.x = p.ry.x + ipy;
        p.rz.x = p.rz.x + ipz;
        const float4 cs = rec[1];
        const float4 ei = rec[2];
        shade(lut, cs, ei, rec + 3, hx, hy, hz, inside, p);
        p.bounce += 1;
        if constexpr (kOwnRule) {
            // (the centre row is read again rather than held across shade: four VGPRs there; the index is
            // made opaque so that the two loads stay two)
            uint32_t again = sidx;
            asm volatile("" : "+v"(again));
            // (the direction walk's kernel: the row of its table this lane reads -- rtk_walk.h direction_groups)
            if constexpr (Walk<WALK>::DIR) dir_row = origin_near(p, mat_src[kSphereF4 * again]) ? sidx : kOwnNone;
            return own_sphere(p, mat_src[kSphereF4 * again], sidx);
        } else {
            return kOwnNone;
        }
    };
    // the pixel's owner lane's fold cursor (first of its P-lane slice) via DPP
    auto fold_cursor = [&]() -> uint32_t {
        return kCursorPerLane ? folded
               : LP == 4 ? (uint32_t)__builtin_amdgcn_update_dpp(0, (int)folded, 0x00, 0xf, 0xf, false)    // quad_perm 0,0,0,0
               : LP == 2 ? (uint32_t)__builtin_amdgcn_update_dpp(0, (int)folded, 0xA0, 0xf, 0xf, false)  // quad_perm 0,0,2,2
               : LP > 4 ? (uint32_t)__shfl((int)folded, (int)(lane - j), 64)
                        : folded;
    };
    // The pixel's parked frontier: every sample below it is in the ring.  A lane's
    // samples below its cursor k are parked (mode 0: k not started yet; 1: k in
    // flight; 2: k >= frames), so it is the minimum of k over the pixel's P lanes
    // -- a DPP reduction inside the lane slice (quads, half rows, rows; a
    // cross-row shuffle only for P = 32), run with every lane active.
    auto parked_frontier = [&]() -> uint32_t {
        // (kDynamic: samples below next are all assigned; those not in flight are parked)
        uint32_t f = kDynamic && mode != 1u ? next : k;
#define RTK_DMIN(CTRL) f = min(f, (uint32_t)__builtin_amdgcn_update_dpp((int)f, (int)f, CTRL, 0xf, 0xf, false))
        if (LP >= 2) RTK_DMIN(0xB1);   // quad_perm 1,0,3,2 (lane ^ 1)
        if (LP >= 4) RTK_DMIN(0x4E);   // quad_perm 2,3,0,1 (lane ^ 2)
        if (LP >= 8) RTK_DMIN(0x141);  // row_half_mirror (the other quad of the 8)
        if (LP >= 16) RTK_DMIN(0x140); // row_mirror (the other half of the row)
#undef RTK_DMIN
        if (LP >= 32) f = min(f, (uint32_t)__shfl_xor((int)f, 16, 64));
        return min(f, a.frames);
    };
    auto fold_ring = [&]() {
        if (LP == 1) return;
        // ---- running-mean blend (main.cpp:484-489) of every parked sample, in
        // order: Final = Out*(1/n) + Prev*((n-1)/n), the first product done by the
        // sample's lane.  Slots [folded, F) are all parked: no per-slot flags, no
        // clearing writes.  Whole batches of four slots aligned to 4 (kRing is a
        // multiple of 4, so a batch never wraps; its LDS reads take immediate
        // offsets), each slot folded straight with no per-slot test; the ragged end
        // once every sample is parked.  A lane that waits for ring space still gets
        // it: the lane holding the frontier sample F < folded + 4 <= folded + kRing
        // is never blocked, so the frontier keeps moving.  Every lane of the pixel
        // runs the loop (F is uniform over them), so each keeps the fold cursor
        // itself; only the folding lanes' sums are used.
        const uint32_t F = parked_frontier();  // (every lane active: a DPP reduction)
        if (!valid) return;
        const uint32_t Fb = F >= a.frames ? F : (F & ~3u);
        while (folded + 4u <= Fb) {
            const float4 *base = ring + (folded % kRing) * kRingStride;
            float v[4], w[4];
            float4 r4[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                if (FOLD3) {
                    const float *slot = reinterpret_cast<const float *>(base + i * kRingStride);
                    v[i] = slot[jc];
                    w[i] = slot[3];
                } else {
                    r4[i] = base[i * kRingStride];
                }
            }
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                if (FOLD3) {
                    accx = v[i] + accx * -w[i];
                } else {
                    accx = r4[i].x + accx * -r4[i].w;
                    accy = r4[i].y + accy * -r4[i].w;
                    accz = r4[i].z + accz * -r4[i].w;
                }
            }
            folded += 4u;
        }
        while (folded < Fb) {
            const float4 *s4 = ring + (folded % kRing) * kRingStride;
            if (FOLD3) {
                const float *slot = reinterpret_cast<const float *>(s4);
                accx = slot[jc] + accx * -slot[3];
            } else {
                const float4 r = *s4;
                accx = r.x + accx * -r.w;
                accy = r.y + accy * -r.w;
                accz = r.z + accz * -r.w;
            }
            folded += 1u;
        }
    };
    // The trip loop.  A hit is shaded at the start of the segment it feeds, not at the end of the one
    // that found it: a lane whose segment hit and whose path goes on keeps p as it was for that
    // segment, notes the hit (pend_t, pend_s) and turns to mode 1; the round that next traces the
    // lane first runs shade_hit on the note.  The lanes of a secondary round are exactly the lanes
    // with such a note, so the shade block is issued in secondary rounds only, for all of the round's
    // lanes; primary rounds (about 83 % of their lanes hit) issue none, and secondary rounds no
    // longer issue one for the fifth of their lanes that hit.  Rounds, their lanes and their order
    // are what they were, trip for trip: nothing in the header looks at anything the shade writes.
    // Exactness: per lane the f32 operations, table gathers and PCG draws of a path are the same, in
    // the same order on the same values -- shade_hit reads only the lane's own p and the hit, and
    // between the hit and its shade the lane takes part in no round.  Only the wave-level moment of
    // the shade moves, and no result depends on it.  The one place that is not the same code is a hit
    // at the bounce limit, which feeds no segment: it takes shade's emission term alone (its first
    // three statements, on the attenuation before the colour multiplies it: same operands, same
    // order, unfused) and ends the path; the normal, draws and direction it skips reached nothing
    // (the sample's RNG state and ray die with it).
    for (;;) {
        // ring space: sample k may start once k < folded + kRing (the oldest
        // unfolded sample's lane is never blocked, so this cannot deadlock)
        // the pixel's owner lane (first of its P-lane quad slice) via DPP
        uint32_t folded_g = fold_cursor();
        uint32_t want_n = 0;  // kDynamic: the slice's lanes wanting a sample
        // The trip's lane masks, each predicate balloted once (the header runs on the CU's one scalar
        // unit for every trip): want = the lanes whose next sample is pending, before the hand-out
        // and after it (lanes past the last frame have left)
        uint64_t want = __builtin_amdgcn_ballot_w64(mode == 0u);
        if (kDynamic) {
            const uint32_t sw_bits = (uint32_t)((want >> slice_base) & ((1ull << LP) - 1ull));
            want_n = __builtin_popcount(sw_bits);
            if (mode == 0u) {
                k = next + __builtin_popcount(sw_bits & ((1u << j) - 1u));
                if (k >= a.frames) mode = 2u;
            }
            want = __builtin_amdgcn_ballot_w64(mode == 0u);
        }
        // (lane masks from single compares: see ballot_and)
        bool ring_ok = LP == 1 || k < folded_g + kRing;
        bool can_start = mode == 0u && ring_ok;
        const uint64_t sec = __builtin_amdgcn_ballot_w64(mode == 1u);
        // (one lane per pixel folds each sample as it ends: nothing left to fold then); the fold
        // cursors are looked at only once no lane has anything left to trace
        if (any_lane(want, sec) == 0u && (LP == 1 || (folding & __builtin_amdgcn_ballot_w64(folded < a.frames)) == 0)) break;
        st.trip_begin();
        // Secondary segments run the full sphere loop; let them gather until
        // enough lanes share one (or no primary work is ready).  Merged rounds
        // (scenes of one or two groups, TraceArgs.merge_rounds): every round
        // starts new samples AND continues paths, all through the exact loop.
        const bool merged = kMergeable && a.merge_rounds != 0u;
        // pri = the lanes that can start their sample; do_sec = sec != 0 && (pri == 0 ||
        // popcount(sec) >= sec_threshold); round = the lanes this round traces (round_select)
        uint64_t pri, round;
        uint32_t do_sec;
        round_select(want, LP == 1 ? ~0ull : __builtin_amdgcn_ballot_w64(ring_ok), sec, a.sec_threshold, pri, do_sec, round);
        if (merged) do_sec = 0u;
        if (do_sec == 0u) {
            // The owners fold only before a primary round: a secondary round starts no sample, so
            // it needs no ring space.  Lazy: only when some lane waits for ring space (pri is a
            // subset of want) or nothing is left to trace: pri | sec == 0.  With split rounds a
            // primary round with pri == 0 has sec == 0 too (round_select), so pri alone is tested;
            // merged rounds (do_sec forced to 0) keep paths going with no lane wanting a sample,
            // and do not fold then.
            if (want != pri || (kMergeable ? (pri | sec) == 0 : pri == 0)) {
                st.fold_begin();
                fold_ring();
                st.fold_end();
                folded_g = fold_cursor();
                ring_ok = LP == 1 || k < folded_g + kRing;
                can_start = mode == 0u && ring_ok;
                pri = LP == 1 ? want : want & __builtin_amdgcn_ballot_w64(ring_ok);
            }
            if (merged) pri |= sec;  // (the lanes a merged round traces)
            round = pri;
            // the slice's lanes that start now are its lowest-ranked wanting ones (none: no change)
            if (kDynamic) next = min(next + want_n, min(a.frames, folded_g + kRing));
        }
        if (round != 0) {  // (else: every lane is done and the fold above took the last parked samples)
            st.round(do_sec, pri, sec, mode, can_start);
            if (bounces) nrays += (uint32_t)__builtin_popcountll(round);
            if (__builtin_amdgcn_inverse_ballot_w64(round)) {  // (the mask itself becomes exec)
                pseg += 1u;
                // The round's lanes are in mode 1 (a pending hit to shade) or 0 (a sample to start).  Split
                // rounds hold one kind, so the choice is the round's own; merged rounds hold both.
                uint32_t own = kOwnNone;  // (lives for this round only: pend_s is dead once shaded)
                if (kMergeable ? mode == 1u : do_sec != 0u)
                    own = shade_hit(pend_t, pend_s & ~kKeyInside, (pend_s & kKeyInside) != 0u);
                else
                    start_sample(kernel_args(), x, y, a.prev_count + k, p);
                bool done;
                if (!bounces) {
                    done = true;  // no segment is traced; the frame folds black
                } else {
                    Hit h;
                    hit_reset(h);
                    const RayPk ray = {p.rx, p.ry, p.rz};
                    if (CULL && !do_sec && !merged) {
                        // (the table's address is loaded here from the kernarg segment, as
                        // the camera fields are: held in an SGPR pair across the trip loop it
                        // cost the RTWeekend kernel SGPR spills, v_readlane in the loop)
                        cv4f_t *prim = (cv4f_t *)kernel_args().prim;
                        for (uint32_t w = 0; w < n_words; ++w) {
                            // (readfirstlane returns int: widen each half as u32, or
                            // bit 31 would sign-extend into groups 32..63)
                            const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)s_maskw[w]);
                            const uint32_t hi =
                                (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(s_maskw[w] >> 32));
                            uint64_t m = (uint64_t)lo | ((uint64_t)hi << 32);
                            st.primary_mask(m);
                            while (m) {  // the tile's sphere pairs, in the reference's order
                                const uint32_t pr = w * 64u + (uint32_t)__builtin_ctzll(m);
                                m &= m - 1;
                                test_pair_prim<SIMD>(a, prim, pr, ray, h, fast);
                            }
                        }
                    } else {
                        // Secondary rays: the prefiltered loop, whose error bound
                        // needs |D|^2 within 2^-16 of 1 on every lane (else exact).
                        const float u2 = __builtin_fmaf(p.rx.y, p.rx.y, __builtin_fmaf(p.ry.y, p.ry.y, p.rz.y * p.rz.y));
                        // (a cluster-walk kernel runs only with the prefilter and a cluster table: rt_host.cpp)
                        const bool pf = do_sec && (Walk<WALK>::CLUSTERS || a.prefilter) &&
                                        !__ballot(!(__builtin_fabsf(1.0f - u2) <= kPfDirTol));
                        if (do_sec && !pf) st.exact_round(u2);
                        if (SRC == kSrcSmem && pf && (Walk<WALK>::CLUSTERS || a.n_cpairs)) {
                            PfStats *ps = st.pf_round();
                            if constexpr (Walk<WALK>::DIR) {
                                direction_groups<SIMD, Walk<WALK>::DIR64>(a, ray, h, fast, own, dir_row, ps);
                            } else if constexpr (Walk<WALK>::CLUSTERS) {
                                // (the scene-wide walk kernels hold the expanded prefilter: rtk_walk.h pair_prefilter_x)
                                clustered_groups<SIMD, Walk<WALK>::W, GS, Walk<WALK>::REL, !Walk<WALK>::REL>(a, lds_groups, ray, h, fast,
                                                                                                            own, ps);
                            } else if constexpr (WALK == kWalkGroups) {
                                __builtin_unreachable();  // the host runs kWalkGroups kernels without a cluster table
                            } else if (a.pf_relative) {
                                if (a.cl_words == 1u) clustered_groups<SIMD, 1, GS, true>(a, lds_groups, ray, h, fast, own, ps);
                                else if (a.cl_words == 2u) clustered_groups<SIMD, 2, GS, true>(a, lds_groups, ray, h, fast, own, ps);
                                else clustered_groups<SIMD, 4, GS, true>(a, lds_groups, ray, h, fast, own, ps);
                            } else {
                                if (a.cl_words == 1u) clustered_groups<SIMD, 1, GS, false>(a, lds_groups, ray, h, fast, own, ps);
                                else if (a.cl_words == 2u) clustered_groups<SIMD, 2, GS, false>(a, lds_groups, ray, h, fast, own, ps);
                                else clustered_groups<SIMD, 4, GS, false>(a, lds_groups, ray, h, fast, own, ps);
                            }
                        } else if (SRC == kSrcSmem && pf && a.pf_relative && !Walk<WALK>::CLUSTERS) {
                            all_groups_smem<SIMD, true, GS, true>(a, lds_groups, ray, h, fast, nullptr, st.pf_round());
                        } else if (SRC == kSrcSmem && pf && !Walk<WALK>::CLUSTERS) {
                            all_groups_smem<SIMD, true, GS>(a, lds_groups, ray, h, fast, nullptr, st.pf_round());
                        } else if (SRC == kSrcSmem) {
                            all_groups_smem<SIMD, false, GS>(a, lds_groups, ray, h, fast, st.sec_hit());
                        } else {
                            // software-pipelined: group g+1's load is in flight while
                            // g is tested (the array carries padding groups)
                            Group next = load_group<SRC>(a, lds_groups, 0);
                            for (uint32_t g = 0; g < a.n_groups; ++g) {
                                const Group G = next;
                                next = load_group<SRC>(a, lds_groups, g + 1u);
                                test_group<SIMD>(a, G, g, ray, h, fast, st.sec_hit());
                            }
                        }
                    }
                    // ---- hit select (x64_math.h:579-585 HorizontalMin + first equal lane)
                    // key: the winner's sphere index sidx with its inside flag in bit 31 (rtk_walk.h Hit), the
                    // word a pending hit carries
                    float tmin;
                    uint32_t key, sidx;
                    if (SIMD) {
                        // Every t is kFMax or a finite value above kEps (candidate): never NaN, never a
                        // zero of either sign, so the hardware minimum returns the bits the reference's
                        // chain of < selects does.
                        asm("v_min3_f32 %0, %1, %2, %3\n\t"
                            "v_min_f32 %0, %0, %4"
                            : "=&v"(tmin)
                            : "v"(h.t0), "v"(h.t1), "v"(h.t2), "v"(h.t3));
                        // the lowest class that holds the minimum: one select per class, no lane-masked region
                        key = h.t0 == tmin ? h.k0 : h.t1 == tmin ? h.k1 : h.t2 == tmin ? h.k2 : h.k3;
                        sidx = key & ~kKeyInside;
                    } else {
                        tmin = h.t0;
                        sidx = h.k0;
                        key = sidx | (h.ins != 0 ? kKeyInside : 0u);
                    }
                    if (tmin == kFMax) {
                        if (at_use(a.use_sky)) {  // main.cpp:434-438
                            const float s = (p.ry.y + 1.0f) * 0.5f;
                            const float w = (1.0f - s) * 1.0f;
                            p.cx = p.cx + (w + s * 0.5f) * p.ax;
                            p.cy = p.cy + (w + s * 0.7f) * p.ay;
                            p.cz = p.cz + (w + s * 1.0f) * p.az;
                        }
                        done = true;
                    } else if (p.bounce + 1u == a.max_bounce) {
                        // a hit at the bounce limit: its emission term is all that reaches the output
                        // (shade's first three statements, main.cpp:446-448)
                        const float4 ei = mat_src[kSphereF4 * sidx + 2u];
                        p.cx = p.cx + ei.x * p.ax;
                        p.cy = p.cy + ei.y * p.ay;
                        p.cz = p.cz + ei.z * p.az;
                        done = true;
                    } else {
                        pend_t = tmin;
                        pend_s = key;
                        done = false;
                    }
                }
                if (done) {
                    const float ox = bounces ? p.cx : 0.0f;
                    const float oy = bounces ? p.cy : 0.0f;
                    const float oz = bounces ? p.cz : 0.0f;
                    if (LP == 1) {
                        // ---- running-mean blend (main.cpp:484-489), in order by construction
                        const uint32_t pc = a.prev_count + k;
                        const float2 fw = SOLO ? (pc < kWeightsN ? a.weights[pc] : fold_weights(pc))
                                               : k < fold_n ? fold[k] : fold_weights(pc);
                        const float inv = fw.x, ratio = fw.y;
                        accx = ox * inv + accx * ratio;
                        accy = oy * inv + accy * ratio;
                        accz = oz * inv + accz * ratio;
                        folded = k + 1u;
                    } else {
                        // park Out*(1/n) and the ratio (n-1)/n of sample k's blend; the
                        // sign bit of .w marks the slot ready (the ratio is >= 0)
                        float2 w;
                        if (SOLO) {  // the static table of the first kWeightsN frames (TraceArgs.weights)
                            const uint32_t pc = a.prev_count + k;
                            w = pc < kWeightsN ? a.weights[pc] : fold_weights(pc);
                        } else {
                            w = fold[k < fold_n ? k : 0u];  // (fold_n = 0: an unused in-bounds read)
                            if (__builtin_expect(k >= fold_n, 0)) w = fold_weights(a.prev_count + k);
                        }
                        ring[(k % kRing) * kRingStride] = make_float4(ox * w.x, oy * w.x, oz * w.x, -w.y);
                    }
                    k += kDynamic ? 0u : LP;
                    mode = kDynamic || k < a.frames ? 0u : 2u;
                    if (Q > 1 && mode == 2u) {
                        // the pixel is complete: store it and move to the lane's next pixel
                        // slot inside the image (its samples start from k = 0)
                        store_pixel();
                        while (mode == 2u && q_slot + 1u < Q) {
                            q_slot += 1u;
                            x = pixel_x(q_slot);
                            ly = pixel_ly(q_slot);
                            if (x < a.width && ly < a.local_rows) {
                                y = global_y(ly);
                                k = 0;
                                folded = 0;
                                load_mean();
                                mode = 0u;
                            }
                        }
                    }
                } else {
                    mode = 1u;
                }
            }
        }
        st.trip_end(round != 0, do_sec);
    }

    if (FOLD3) {  // channels 1 and 2 from lanes j = 1, 2 of the pixel's quad (quad_perm 1,1,1,1 / 2,2,2,2)
        accy = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(accx), 0x55, 0xf, 0xf, false));
        accz = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(accx), 0xAA, 0xf, 0xf, false));
    }
    if (Q == 1 && valid && owner && a.frames > 0) store_pixel();  // (Q > 1: stored as each pixel completes)

    cargs_t &ka = kernel_args();  // (the end's fields from the kernarg segment: see wave_unit above)
    if (ka.pix_cost) {  // the pixel's traced segments over its P lanes (every lane active here)
        for (uint32_t off = 1; off < LP; off <<= 1) pseg += (uint32_t)__shfl_xor((int)pseg, (int)off, 64);
        if (Q == 1 && valid && owner) ka.pix_cost[(size_t)ly * ka.width + x] = pseg;
    }
    // ---- ray counter (RaysCastInThread, main.cpp:390): one atomic per wave
    if (lane == 0 && nrays) atomicAdd(ka.rays, (unsigned long long)nrays);
    if ((ka.tile_cost || ka.wave_times) && lane == 0) {
        uint32_t tile_e, wave_e;
        wave_unit<SOLO>(ka, tid, tile_e, wave_e);
        if (ka.tile_cost) {
            const uint64_t c = __builtin_amdgcn_s_memtime() - s_cost0[sw];
            const uint32_t c32 = (uint32_t)(c < 0xFFFFFFFFull ? c : 0xFFFFFFFFull);
            if (SOLO && ka.unit_waves != 0u)
                ka.tile_cost[4u * tile_e + wave_e] = c32 | 1u;  // (>= 1: a launched wave never ranks with dead ones)
            else
                atomicMax(ka.tile_cost + tile_e, c32);
        }
        if (ka.wave_times) ka.wave_times[2u * ((uint64_t)tile_e * 4u + wave_e) + 1u] = __builtin_amdgcn_s_memrealtime();
    }
    st.flush(a.stats, lane);
}

}  // namespace rtk

// F: 0, or kWalkTileCounts for a launch with per-tile counts (a->tile_counts_at set).  Each translation
// unit instantiates the F it launches: the per-tile kernels are compiled in units of their own
// (rt_trace_tc.hip; P = 16 beside the uniform ones in rt_trace_p16.hip), in parallel with these.
template <int P, int F = 0>
static void launch_p(const TraceArgs *a, int simd, int src, int cull, uint32_t n_blocks, hipStream_t stream) {
    const dim3 block(256), grid(n_blocks);
    const size_t lds = rtk_lds_bytes(a);
    const size_t solo_lds = 8u * rtk_mask_words(a->n_groups);  // one-wave kernels: the cull mask words
#define RTK_LAUNCH(S, R, C, G) \
    hipLaunchKernelGGL((rtk::trace_kernel<S, R, C, P, G, false, F>), grid, block, lds, stream, *a)
#define RTK_LAUNCH_SOLO(S, C, K) \
    hipLaunchKernelGGL((rtk::trace_kernel<S, kSrcSmem, C, P, true, true, (K) | F>), dim3(4u * n_blocks), dim3(64), solo_lds, \
                       stream, *a)
    if (a->solo) {  // one wave per workgroup, no LDS image (the host clears the *_in_lds flags)
        // One walk per kernel where the launch has every fact such a kernel takes at compile time; else
        // the run-time kernel.  rt_kernel.h rtk_walk_kernel is the whole rule: no condition here.
        // (The walk kernels are instantiated for their shapes only: rtk_walk_shape.)
        if constexpr (rtk_walk_shape(P)) {
#define RTK_WALKS(S)                                                          \
    switch (rtk_walk_kernel(*a, cull, P)) {                                   \
        case kWalkGroups: RTK_LAUNCH_SOLO(S, true, kWalkGroups); return;      \
        case kWalkCl1: RTK_LAUNCH_SOLO(S, true, kWalkCl1); return;            \
        case kWalkCl2: RTK_LAUNCH_SOLO(S, true, kWalkCl2); return;            \
        case kWalkCl4: RTK_LAUNCH_SOLO(S, true, kWalkCl4); return;            \
        case kWalkCl1Rel: RTK_LAUNCH_SOLO(S, true, kWalkCl1Rel); return;      \
        case kWalkCl2Rel: RTK_LAUNCH_SOLO(S, true, kWalkCl2Rel); return;      \
        case kWalkCl4Rel: RTK_LAUNCH_SOLO(S, true, kWalkCl4Rel); return;      \
        case kWalkCl1Dir: RTK_LAUNCH_SOLO(S, true, kWalkCl1Dir); return;      \
        case kWalkCl1Dir64: RTK_LAUNCH_SOLO(S, true, kWalkCl1Dir64); return;  \
        default: break;                                                       \
    }
            if (simd) { RTK_WALKS(true) } else { RTK_WALKS(false) }
#undef RTK_WALKS
        }
        const int key = (simd ? 2 : 0) | (cull ? 1 : 0);
        switch (key) {
            case 0: RTK_LAUNCH_SOLO(false, false, kWalkAny); break;
            case 1: RTK_LAUNCH_SOLO(false, true, kWalkAny); break;
            case 2: RTK_LAUNCH_SOLO(true, false, kWalkAny); break;
            default: RTK_LAUNCH_SOLO(true, true, kWalkAny); break;
        }
        return;
    }
#undef RTK_LAUNCH_SOLO
    if constexpr (F != 0) {
        // Four-wave per-tile kernels exist for a scene in the LDS image read through the scalar cache
        // only (rt_kernel.h rtk_tile_counts_four_wave): the host routes every other four-wave
        // per-tile launch to the one-wave run-time kernel above, so nothing else arrives here.
        const int key = (simd ? 2 : 0) | (cull ? 1 : 0);
        switch (key) {
            case 0: RTK_LAUNCH(false, kSrcSmem, false, false); break;
            case 1: RTK_LAUNCH(false, kSrcSmem, true, false); break;
            case 2: RTK_LAUNCH(true, kSrcSmem, false, false); break;
            default: RTK_LAUNCH(true, kSrcSmem, true, false); break;
        }
        return;
    } else {
    if (!a->scene_in_lds) {  // the scene in HBM (the host picks the SMEM source for it)
        const int key = (simd ? 2 : 0) | (cull ? 1 : 0);
        switch (key) {
            case 0: RTK_LAUNCH(false, kSrcSmem, false, true); break;
            case 1: RTK_LAUNCH(false, kSrcSmem, true, true); break;
            case 2: RTK_LAUNCH(true, kSrcSmem, false, true); break;
            default: RTK_LAUNCH(true, kSrcSmem, true, true); break;
        }
        return;
    }
    const int key = (simd ? 4 : 0) | (src == kSrcLds ? 2 : 0) | (cull ? 1 : 0);
    switch (key) {
        case 0: RTK_LAUNCH(false, kSrcSmem, false, false); break;
        case 1: RTK_LAUNCH(false, kSrcSmem, true, false); break;
        case 2: RTK_LAUNCH(false, kSrcLds, false, false); break;
        case 3: RTK_LAUNCH(false, kSrcLds, true, false); break;
        case 4: RTK_LAUNCH(true, kSrcSmem, false, false); break;
        case 5: RTK_LAUNCH(true, kSrcSmem, true, false); break;
        case 6: RTK_LAUNCH(true, kSrcLds, false, false); break;
        default: RTK_LAUNCH(true, kSrcLds, true, false); break;
    }
    }
#undef RTK_LAUNCH
}

// The P = 16 launches are compiled in a translation unit of their own (rt_trace_p16.hip), the
// launches with per-tile counts of every other shape in another (rt_trace_tc.hip)
extern "C" void rtk_launch_p16(const TraceArgs *a, int simd, int src, int cull, uint32_t n_blocks,
                               hipStream_t stream);
extern "C" void rtk_launch_tile_counts(const TraceArgs *a, int simd, int src, int cull, int lanes_per_pixel,
                                       uint32_t n_blocks, hipStream_t stream);
