// rt_kernel.h — launch contract between the C-ABI host (rt_host.cpp, its launch decisions rt_plan.cpp) and the
// gfx950 kernels (rt_trace.hip, rt_trace_p16.hip, rt_trace_tc.hip, rt_sched.hip, rt_first_hit.hip).  Internal; not part of include/.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rt_layout.h"

enum { kSrcSmem = 0, kSrcLds = 1 };  // where the sphere loop reads its groups
enum { kFlagAccumZero = 1, kFlagSrgbPow = 2 };
// (the scene and table layouts the host packs: rt_layout.h)
struct TraceArgs {
    const float4 *groups;
    const float4 *materials;
    const float *rsqrt_lut;      // 2048 f32
    float4 *prev;                // compact band image, local_rows x width
    uint32_t *cur;               // compact band image, local_rows x width
    unsigned long long *rays;    // accumulated bounce segments
    float cam_pos[3], cam_x[3], cam_y[3], film_center[3];
    float film_w, film_h;
    float inv_width, inv_height;  // RN(1/(f32)width), RN(1/(f32)height)
    float width_f, height_f;      // (f32)width, (f32)height: the divisors themselves (start_sample)
    uint32_t width, height, local_rows;
    uint32_t prev_count, frames, max_bounce;
    uint32_t n_groups, n_spheres, use_sky, flags;  // n_spheres: scalar rule set only
    uint32_t band_rows, band_count, band_index;
    uint32_t sec_threshold;      // lanes that must wait for a secondary iteration
    uint32_t prefilter;          // secondary sphere loop: FMA prefilter + exact recheck (r2p valid); kPrefilter*
    uint32_t fast_sqrt;          // every hittable r^2 is 0 or in [2^-36, 2^60] (candidate sqrt_rn)
    unsigned long long *stats;   // optional (RT_STATS): kStat* counters, NULL = off
    unsigned long long *wave_times;  // optional (RT_WAVETIMES): per-wave {start, end} s_memrealtime
    const uint32_t *tile_order;  // optional: block -> tile map (heaviest first), NULL = identity
    uint32_t *tile_cost;         // optional: per-tile cost (max wave shader cycles), atomicMax'd
    const uint64_t *masks;       // CULL: per wave tile (4*tile + wave) n_words primary group masks
    uint32_t tiles_x;            // block tiles per row (2TW x 2TH pixels each)
    const float4 *clusters;      // optional: clustered prefilter table (cl_entry_f4(cl_words) rows per entry)
    uint32_t n_cpairs;           // cluster-pair entries at its start; 0 = per-group prefilter loop
    uint32_t cl_words;           // u64 words of the clustered loop's pair mask (1 or 2)
    uint32_t interleave;         // wave tiles interleave over the block tile (P >= 2 only)
    uint32_t lut_in_lds;         // rsqrt table in the LDS image (else read from HBM: rtk_lut_in_lds)
    uint32_t fold_in_lds;        // running-mean weight table in the LDS image (else computed: rtk_fold_in_lds)
    uint32_t scene_in_lds;       // groups + materials copied into the LDS image (else read from HBM: GS kernels)
    uint32_t pf_relative;        // prefilter: row kRowR2P holds r^2 and the threshold is per lane (rtk_walk.h kPfRel)
    uint32_t solo;               // one wave per workgroup (4 x tiles workgroups of 64 threads; needs no LDS image)
    uint32_t walk;               // kWalk*: the one-wave kernel specialised for this launch's secondary walk
    // optional: live block tiles of the cull pass, on the device (kCullTotals).  Set while the host
    // has not read the count back: the grid then covers every tile and blocks past the count exit.
    const unsigned long long *live_total;
    // one-wave kernels (solo): tile_order / tile_cost index WAVES (4 * block tile + quadrant),
    // so the heaviest-first order ranks every wave on its own cost (rt_plan.cpp plan_launch, LaunchPlan.unit_waves)
    uint32_t unit_waves;
    // optional (rt_device_options PixelSort): the block tile's pixels dealt to its four waves by cost,
    // cheapest first: pix_perm[64 * tile + NPIX * wave + pl] = the pixel's index in the
    // block tile (row-major, 2TW wide); pix_perm[64 * tile] == 0xFF: not permuted
    const uint8_t *pix_perm;
    // optional: segments each pixel traced in this launch (band-local rows x width), the
    // cost the next launch's permutation sorts by (rtk_launch_pixel_sort)
    uint32_t *pix_cost;
    // 1: every round starts new samples and continues paths together through the exact
    // sphere loop (scenes of at most kMergeGroups groups: the cull mask and the prefilter
    // save nothing there, and split rounds leave most lanes idle at one frame per launch)
    uint32_t merge_rounds;
    // pixels per dealt unit of the pixel sort (1, 2 or 4; capped at the wave's pixel count): the
    // sort ranks row segments of pix_seg pixels by their summed cost, so each wave's owner
    // lanes store whole 4-pixel runs (a 64-B half line of the v4 image) instead of single
    // pixels of lines other waves -- on other XCDs -- also write
    uint32_t pix_seg;
    // 1: the trace and empty-tile kernels store only the running mean; the RGBA8 image is
    // encoded from it by one coalesced pass after the launch (rtk_launch_encode), so its 4-B
    // pixels are not written as scattered partial lines from several XCDs (rt_device_options EncodePass)
    uint32_t skip_cur;
    // CULL (required): the primary rounds' group rows, written by the cull pass for its camera
    // (rtk_launch_cull): per group kPrimF4 float4 = {cx[4]}, {cy[4]}, {cz[4]}, {r*r[4]} with
    // c = RN(centre - CameraPosition), the first three f32 ops of every primary sphere test
    // (main.cpp:401), identical on every lane of a primary round (one s_load_dwordx16)
    float4 *prim;
    // the running-mean weights {RN(1/(n+1)), RN(n/(n+1))} of frames n < kWeightsN (main.cpp:484-487),
    // one table per device computed once (rt_device_create): a finished sample's two weights are one
    // gather instead of two conversions, a reciprocal and a division (one-wave kernels)
    const float2 *weights;
    // optional (rt_trace_tiles): the launch covers only the listed reference tiles (kRefTile x kRefTile
    // pixels, main.cpp:9).  One bit per reference tile, bit t & 31 of word t >> 5 with
    // t = TileY * sel_tiles_x + TileX; NULL = every tile.  Read by the scheduling kernels only
    // (rt_sched.hip: cull / select, pixel sort, encode): every launch shape's block tile divides a
    // reference tile (rtk_shape.h), so a selection is a set of whole block tiles and the trace
    // kernels see nothing but a shorter live prefix of tile_order.
    const uint32_t *sel;
    uint32_t sel_tiles_x;        // reference tiles per image row: ceil(width / kRefTile)
    // optional (rt_trace_tile_work, with sel): each listed reference tile's own counts, two words per
    // tile of the image -- {PreviousRayCount, Frames} at 2 * (TileY * sel_tiles_x + TileX) of the table
    // rtk_tile_counts(a); 0 = none: the launch's prev_count / frames hold for every tile.  A block tile
    // lies in one reference tile, so a wave takes one pair: the trace kernels compiled with
    // kWalkTileCounts overwrite their by-value prev_count / frames with it before anything reads them,
    // and rtk_launch_empty_counts folds each dead tile by its own pair.  In a host-built table every listed
    // tile's Frames is >= 1 (the host drops the others); in a device-built one (rtk_launch_counts_table) a
    // listed tile may hold 0 frames: it rests, and both kernels leave it before any store.  The launch's own
    // frames field holds the largest Frames of the table, or a bound of them.
    // The table is named by its word offset from `sel` -- it lies behind the bitmap in the same device
    // buffer (rtk_sel_table_at) -- and not by a pointer of its own, because a u32 fits the struct's tail
    // padding: sizeof(TraceArgs) stays what it was, and with it the kernarg offsets of everything
    // behind the struct (the scheduling kernels' other arguments, the hidden arguments the four-wave
    // kernels read blockDim from).  An appended pointer moved those by 8 in every such kernel and
    // renumbered select_kernel's SGPRs; this way no kernel of a uniform launch changes by a bit.
    uint32_t tile_counts_at;
};
static_assert(sizeof(TraceArgs) == 360, "the kernarg layout of the kernels that take it (see tile_counts_at)");
static inline __host__ __device__ const uint32_t *rtk_tile_counts(const TraceArgs &a) {
    return a.tile_counts_at ? a.sel + a.tile_counts_at : nullptr;
}
// the selection buffer of an image of n reference tiles: the bitmap's words, then (8-byte aligned) the
// counts table's 2 n words, then (8-byte aligned again) a second bitmap of the same size: the listed
// tiles that fold at least one frame in a launch whose table the device built (rtk_launch_counts_table)
static inline uint32_t rtk_sel_table_at(uint32_t n_ref_tiles) { return 2u * ((n_ref_tiles + 63u) / 64u); }
static inline size_t rtk_sel_active_at(uint32_t n_ref_tiles) { return rtk_sel_table_at(n_ref_tiles) + 2u * (size_t)n_ref_tiles; }
static inline size_t rtk_sel_buffer_words(uint32_t n_ref_tiles) { return rtk_sel_active_at(n_ref_tiles) + rtk_sel_table_at(n_ref_tiles); }
// The frames a tile folds from a caller's device entry {prev, frames} in a launch of at most max_frames
// (rt_trace_tile_counts, rt_tile_counts_step): the entry's frames clamped to the launch's, and 0 -- the
// tile rests -- where prev + that many no longer fits the u32 frame count.  The device cannot refuse an
// entry as the host refuses an rt_tile_work one, so an impossible entry folds nothing.
static inline __host__ __device__ uint32_t rtk_effective_frames(uint32_t prev, uint32_t frames, uint32_t max_frames) {
    const uint32_t f = frames < max_frames ? frames : max_frames;
    return prev > 0xFFFFFFFFu - f ? 0u : f;
}
constexpr uint32_t kRefTile = 32;  // the reference's TileSize (main.cpp:9; RT_TILE_SIZE of rt_trace.h)
// live[] values of a block tile (rtk_launch_cull / rtk_launch_select): dead (folded by rtk_launch_empty),
// live (traced), or outside the launch's tile selection (neither: no byte of it is written)
enum { kTileDead = 0, kTileLive = 1, kTileSkipped = 2 };
constexpr uint32_t kWeightsN = 65536;
constexpr uint32_t kPrimF4 = 4;
constexpr uint32_t kMergeGroups = 2;
// Cull pass counters (rtk_launch_cull): [0, 64) striped live block tiles, [64, 128)
// striped image pixels of dead block tiles, then the two totals at kCullTotals
// (live tiles, dead pixels), summed on the device after the pass.
constexpr uint32_t kCullCounterWords = 132;
constexpr uint32_t kCullTotals = 128;
constexpr uint32_t kCullFolded = 130;  // a per-tile launch's folded segments (rtk_launch_empty_counts), per launch
// TraceArgs.prefilter: off, on, or on with `clusters` naming the expanded table -- the scene-wide
// table recentred on c0, `clusters` naming the float4 row {c0, 0} and entry 0 the row behind it, its thresholds those of the
// 7-op estimate (rtk_walk.h pair_prefilter_x; rt_pack.cpp expand_table).  The host sets
// the last only where that table exists and is proven and useful for the scene, and only for a
// launch of a kernel that reads it (below); every other kernel tests the field as a boolean.
// kPrefilterDirection: the expanded table, and behind it in the same buffer the direction block of a one-word
// table (rt_layout.h; word 3 of the row {c0, .} is its offset): the launch fact of the direction walk below.
enum { kPrefilterOff = 0, kPrefilterOn = 1, kPrefilterExpanded = 2, kPrefilterDirection = 3 };
static inline bool rtk_prefilter_expanded(uint32_t prefilter) { return prefilter >= (uint32_t)kPrefilterExpanded; }
// Secondary-ray walk variants (rtk_shape.h Walk<>): any (run-time dispatch),
// the per-group loops, or a cluster walk with 1/2/4 pair-mask words and
// scene-wide or per-lane ("Rel") thresholds
enum { kWalkAny = 0, kWalkGroups, kWalkCl1, kWalkCl2, kWalkCl4, kWalkCl1Rel, kWalkCl2Rel, kWalkCl4Rel,
       // kWalkCl1 with the direction table choosing the member entries (rtk_walk.h direction_groups): a kernel of
       // its own, never a request -- TraceArgs.walk and rt_trace_info.Walk stay kWalkCl1, rtk_walk_kernel picks it
       kWalkCl1Dir,
       // the same with 64-bit masks (more than 16 groups: rt_layout.h dir_mask64): the mask's width is a fact of
       // the kernel, so a round tests it nowhere
       kWalkCl1Dir64 };
// Compile-time flag of trace_kernel, off in every value above: OR'ed into the kernel's WALK template
// value it compiles the per-tile counts variant (TraceArgs.tile_counts_at).  A flag bit of an existing
// parameter rather than a parameter of its own, so that the kernels without it keep their symbols.
enum { kWalkMask = 0xFF, kWalkTileCounts = 0x100 };
// The four-wave kernels exist with the flag for a scene in the LDS image read through the scalar cache
// (the default four-wave device); a per-tile launch of any other four-wave device (SphereSourceLds,
// SceneInHbm, a scene beyond the LDS image) runs the one-wave run-time kernel (rt_plan.cpp route_kernel).
static inline bool rtk_tile_counts_four_wave(uint32_t scene_in_lds, int src) { return scene_in_lds != 0u && src == kSrcSmem; }

// ---- Routing of the walk-specialised one-wave kernels (trace_kernel<..., SOLO = true, WALK != kWalkAny>).
// Such a kernel holds one secondary walk and takes these facts of its launch at compile time
// (rtk_trace.h trace_kernel, kFastSqrt and kFacts); a launch without one of them computes garbage
// in it, so every launch goes through the two functions below and nothing else decides:
//   fast_sqrt       every hittable r^2 is 0 or in [2^-36, 2^60], so a candidate's r^2 - dist is 0
//                   or inside sqrt_rn's verified range [2^-60, 2^60]: the walk kernels hold the
//                   short square root alone, the run-time kernel keeps the IEEE one beside it
//   max_bounce >= 1 the walk kernels hold no zero-bounce path (such a launch traces nothing and
//                   folds every frame black: the run-time kernel keeps that path)
//   frames >= 1     (rt_trace returns before the launch at Frames == 0, and no part of a split
//                   launch is empty)
//   cluster walks   run only with a non-empty table over a non-empty scene: clusters set,
//                   n_cpairs >= 1, n_groups >= 1 (their top loop has no zero-trip test), and with the
//                   prefilter on (they do not test it; plan_launch sets clusters only with it)
//   expanded table  the scene-wide cluster walks (kWalkCl1 / Cl2 / Cl4) hold the expanded prefilter alone:
//                   they run only where `clusters` is the expanded table (prefilter == kPrefilterExpanded:
//                   it exists, every value of it is finite, and its extra slack G stays within a quarter
//                   of each entry's own E -- rt_pack.cpp expand_table).  A scene-wide table without that
//                   (a scene placed far from its own extent's scale) is walked by the run-time kernel
//                   on the table as it always was.
//   direction table the one-word scene-wide walk (kWalkCl1) has a second kernel, kWalkCl1Dir, which chooses its
//                   member entries by the direction block behind the expanded table.  It runs where that block
//                   exists (prefilter == kPrefilterDirection: the expanded table is in use, the host built the
//                   block -- rt_device_options DirectionTable -- and lays it behind the table), the walk has one
//                   mask word and the scene at most kDirMaxGroups groups (128 spheres); else kWalkCl1 as before.
//                   The width of the table's masks (dir_mask64) is a fact too: kWalkCl1Dir holds the 32-bit union
//                   and walk, kWalkCl1Dir64 the 64-bit ones, chosen here by the function the packer lays the table out by.
//                   The host offers the block by default to the shapes of at most 8 lanes per pixel
//                   (rtk_direction_default): the 16-lane shape is the 8-rank band share's, launches of half a
//                   millisecond, which measured 3.5 % slower with it; DirectionTable on offers it there too.
// and the kernels exist only for the culled production shapes (rtk_walk_shape).  Every other launch
// runs the run-time kernel (kWalkAny), which tests each fact where it matters and dispatches the
// walk the table asks for.
// The walk a launch asks for (rt_plan.cpp route_kernel; TraceArgs.walk, rt_trace_info.Walk) of a one-wave launch, from the
// scene's table and the facts the host decides by; walk_any: rt_device_options WalkAny.
static inline uint32_t rtk_walk_request(const TraceArgs &a, bool walk_any) {
    if (walk_any || !a.fast_sqrt || a.max_bounce == 0u) return kWalkAny;
    if (!a.clusters) return kWalkGroups;
    if (!a.pf_relative && !rtk_prefilter_expanded(a.prefilter)) return kWalkAny;
    if (a.cl_words == 1u) return a.pf_relative ? kWalkCl1Rel : kWalkCl1;
    if (a.cl_words == 2u) return a.pf_relative ? kWalkCl2Rel : kWalkCl2;
    return a.pf_relative ? kWalkCl4Rel : kWalkCl4;
}
// the launch shapes (lanes per pixel; 0: kPixelsPerLane pixels per lane) with walk kernels
constexpr bool rtk_walk_shape(int lanes_per_pixel) {
    return lanes_per_pixel == 0 || lanes_per_pixel == 4 || lanes_per_pixel == 8 || lanes_per_pixel == 16;
}
// The WALK template value of the kernel a launch runs: the request, when the launch has every fact
// above (all tested here, whatever the request was derived from), else kWalkAny.
static inline uint32_t rtk_walk_kernel(const TraceArgs &a, int cull, int lanes_per_pixel) {
    if (!a.solo || !rtk_walk_shape(lanes_per_pixel) || !cull) return kWalkAny;
    if (!a.fast_sqrt || a.max_bounce == 0u || a.frames == 0u) return kWalkAny;
    if (a.walk >= (uint32_t)kWalkCl1 && (a.clusters == nullptr || a.n_cpairs == 0u || a.n_groups == 0u || !a.prefilter))
        return kWalkAny;
    if (a.walk >= (uint32_t)kWalkCl1 && a.walk <= (uint32_t)kWalkCl4 && !rtk_prefilter_expanded(a.prefilter))
        return kWalkAny;
    if (a.walk == (uint32_t)kWalkCl1 && a.prefilter == (uint32_t)kPrefilterDirection && a.cl_words == 1u &&
        a.n_groups <= kDirMaxGroups)
        return dir_mask64(a.n_groups) ? kWalkCl1Dir64 : kWalkCl1Dir;
    // (and the expanded table is read by no other kernel: the host decides with rtk_walk_expanded)
    return a.walk <= (uint32_t)kWalkCl4Rel ? a.walk : (uint32_t)kWalkAny;
}
// Whether the launch's kernel walks the expanded table: route_kernel (rt_plan.cpp) offers it (clusters = the expanded
// table, prefilter = kPrefilterExpanded), asks this, and puts the plain table back where the answer is no.
static inline bool rtk_walk_expanded(const TraceArgs &a, int cull, int lanes_per_pixel) {
    const uint32_t k = rtk_walk_kernel(a, cull, lanes_per_pixel);
    return (k >= (uint32_t)kWalkCl1 && k <= (uint32_t)kWalkCl4) || k == (uint32_t)kWalkCl1Dir || k == (uint32_t)kWalkCl1Dir64;
}
// The launch shapes the direction block is offered to without being asked for (rt_plan.cpp route_kernel).
constexpr bool rtk_direction_default(int lanes_per_pixel) { return lanes_per_pixel <= 8; }
// Whether it is the direction walk's kernel (rt_trace_last_direction_table).
static inline bool rtk_walk_direction(const TraceArgs &a, int cull, int lanes_per_pixel) {
    const uint32_t k = rtk_walk_kernel(a, cull, lanes_per_pixel);
    return k == (uint32_t)kWalkCl1Dir || k == (uint32_t)kWalkCl1Dir64;
}

enum { kStatPriIters = 0, kStatPriLanes, kStatSecIters, kStatSecLanes, kStatPriGroups, kStatSecHitGroups,
       kStatSecSparseIters, kStatSecSparseLanes, kStatSecTailIters, kStatPriCycles, kStatSecCycles, kStatFoldCycles,
       kStatSetupCycles, kStatCullCycles, kStatSyncCycles, kStatPostCycles, kStatPfRounds, kStatPfGroups,
       kStatClTested, kStatPfPairs, kStatClTopEntered, kStatPfLanePairs, kStatPriBlocked, kStatPriWaitSec,
       kStatPriDone, kStatSecDone, kStatSecWaitPri, kStatDoneTrips, kStatDoneLaneTrips,
       kStatSecExact, kStatSecBadLanes, kStatSecZeroDir, kStatCount = 32 };
constexpr uint32_t kStatSlots = 32;  // rt_debug_stats copies this many

// Dynamic LDS per block: [rsqrt table] + fold table + groups + materials.
// The 8 KB table stays in LDS up to 32 groups; a larger scene's image would
// cost occupancy (C5's 64 groups: 5 -> 7 blocks per CU without it and the
// weight table), so the table is then read from HBM through the caches.
// The 2 KB weight table of the first 256 frames goes the same way (the
// weights are then two divisions per sample): C5 fits 7 blocks per CU.
// The cull pass's primary masks hold one bit per sphere PAIR (spheres 2p, 2p + 1: half p & 1 of group
// p >> 1), so a primary round tests only the pairs its tile's cone may reach -- half of the group-level
// masks' pair tests at C2 (1.17 of 2.33 pairs per live 4x4 tile); words per wave tile:
static inline __host__ __device__ uint32_t rtk_mask_words(uint32_t n_groups) { return (2u * n_groups + 63u) / 64u; }
static inline bool rtk_lut_in_lds(uint32_t n_groups) { return n_groups <= 32u; }
static inline bool rtk_fold_in_lds(uint32_t n_groups) { return n_groups <= 32u; }
static inline size_t rtk_scene_lds_bytes(uint32_t n_groups) {
    return (size_t)n_groups * (16u * kGroupF4 + 64u * kSphereF4);
}
static inline size_t rtk_lds_bytes(const TraceArgs *a) {
    return (a->lut_in_lds ? 8192u : 0u) + (a->fold_in_lds ? 2048u : 0u) +
           (a->scene_in_lds ? rtk_scene_lds_bytes(a->n_groups) : 0u);
}
// The largest scene the LDS image holds (64 KB of dynamic LDS per block with
// the two tables): 265 groups = 1,060 spheres.  Larger scenes stay in HBM
// (scene_in_lds = 0): the sphere loop reads groups through the scalar cache as
// always, and the per-lane gathers go through L1/L2.  Up to kMaxGroups groups (rt_layout.h).
static const uint32_t kMaxLdsGroups = (65536u - 8192u - 2048u) / (16u * kGroupF4 + 64u * kSphereF4);  // 164 groups

extern "C" int rtk_launch_trace(const TraceArgs *a, int simd, int src, int cull, int lanes_per_pixel,
                                hipStream_t stream);
// One wave of the direction walk's union under exec = lanes (rt_direction_union; rt_trace.hip):
// in = 64 low words, 64 high words, 64 canaries; out = the union's two words, 64 canaries.
extern "C" int rtk_launch_direction_union(const uint32_t *in, uint64_t lanes, uint32_t wide, uint32_t *out,
                                          hipStream_t stream);
// Heaviest-first tile order for the next launch from this launch's costs
// (resets the costs); n = rtk_tile_count(...) of the launch geometry.
// scratch: rtk_tile_sort_scratch(n) bytes of device memory
extern "C" size_t rtk_tile_sort_scratch(uint32_t n);
extern "C" int rtk_launch_tile_sort(uint32_t *cost, uint32_t *order, uint32_t *scratch, uint32_t n, hipStream_t stream);
// One-wave kernels' wave order: the live prefix (4 x live_tiles[0] units) of a sorted
// order_in partitioned stably by XCD group (every eighth live tile by its heaviest
// wave's rank) and interleaved so that every wave of a block tile runs on one XCD
// (rt_sched.hip, "XCD grouping"); the rest copied.  scratch: rtk_tile_sort_scratch(
// n_units) bytes (8 n_blk + 9 words used); aux: 2 x n_units / 4 words.
extern "C" int rtk_launch_xcd_group(const uint32_t *order_in, uint32_t *order_out, uint32_t n_units,
                                    const unsigned long long *live_tiles, uint32_t *scratch, uint32_t *aux,
                                    hipStream_t stream);
// (host arithmetic on the launch shapes of rtk_shape.h: defined in rt_plan.cpp)
extern "C" uint32_t rtk_tile_count(uint32_t width, uint32_t local_rows, int lanes_per_pixel);
extern "C" uint32_t rtk_tiles_x(uint32_t width, int lanes_per_pixel);
// grid: blocks of the trace launch (tile_order[0..grid) when tile_order is set)
extern "C" int rtk_launch_trace_grid(const TraceArgs *a, int simd, int src, int cull, int lanes_per_pixel,
                                     uint32_t grid, hipStream_t stream);
// Primary-ray cone culling of every wave tile -> a->masks, and the camera-relative
// group rows of the primary rounds -> a->prim (both must be set);
// per block tile live[t] (some wave tile has a candidate group, or
// !empty_capable) and cost[t] = live ? 2 : 0 (so a tile sort puts live tiles
// first); counters[0, 64) sum to the live tiles, counters[64, 128) to the
// image pixels of dead tiles (zeroed by the call), and counters[kCullTotals],
// counters[kCullTotals + 1] receive the two sums (kCullCounterWords words).
// With a selection (a->sel) a block tile outside it leaves before any of that:
// live[t] = kTileSkipped, cost 0, no mask words written and nothing counted --
// whether or not the launch is empty_capable -- so the totals are those of the
// selected tiles and the sorted order's prefix holds selected live tiles only.
extern "C" int rtk_launch_cull(const TraceArgs *a, int lanes_per_pixel, uint32_t *live, uint32_t *cost,
                               unsigned long long *counters, int empty_capable, hipStream_t stream);
// The cull pass's stand-in for a selection on a device without culling (a->sel set):
// live[t] = kTileLive / kTileSkipped and cost 2 / 0 per unit from the bitmap, so that a tile
// sort puts the selected tiles first (the caller sets the totals: it knows the count).
extern "C" int rtk_launch_select(const TraceArgs *a, int lanes_per_pixel, uint32_t *live, uint32_t *cost,
                                 hipStream_t stream);
// rtk_launch_encode over the pixels of the selected reference tiles of a full image
// (a->prev -> a->cur, a->width x a->local_rows, a->sel set): no other RGBA8 pixel is written.
extern "C" int rtk_launch_encode_selected(const TraceArgs *a, hipStream_t stream);
// rtk_launch_encode_selected that also writes, per selected reference tile t, delta[t] = the rt_tile_delta
// (rt_trace.h; 16 B, 16-byte aligned) between the RGBA8 a->cur held and the RGBA8 it stores there
// (rt_trace_tile_work_delta; a->sel set; entries of unselected tiles are not written).
extern "C" int rtk_launch_tile_delta_encode(const TraceArgs *a, void *delta, hipStream_t stream);
// The same statistics between two RGBA8 images, for every reference tile of a width x height image;
// nothing else is written (rt_tile_delta_rgba8).
extern "C" int rtk_launch_tile_delta(const uint32_t *old_img, const uint32_t *new_img, uint32_t width, uint32_t height,
                                     void *delta, hipStream_t stream);
// rt_trace_tile_counts' table pass: counts (the caller's DEVICE rt_tile_counts array, one entry per
// reference tile) and the key's bitmap sel -> table (rtk_sel_table_at: {prev, rtk_effective_frames} for a
// listed tile, {0, 0} for every other, whose entry is not read) and active (rtk_sel_active_at: the bitmap of
// the listed tiles that fold a frame; the closing pass takes it for its selection, so a resting tile gets
// no RGBA8 and no statistics).  All three lie in the selection buffer; read and written in stream order.
extern "C" int rtk_launch_counts_table(const void *counts, const uint32_t *sel, uint32_t n_ref_tiles, uint32_t max_frames,
                                       uint32_t *table, uint32_t *active, hipStream_t stream);
// rt_tile_counts_step: the per-tile stopping rule over counts (rt_tile_counts) and delta (rt_tile_delta) of
// n_ref_tiles tiles, one block; summary (rt_tile_step_summary, optional) is written, never accumulated.
extern "C" int rtk_launch_tile_counts_step(void *counts, const void *delta, uint32_t n_ref_tiles, uint32_t max_round,
                                           uint32_t max_tile, uint32_t rest_max_delta, uint32_t rest_sum_squares,
                                           void *summary, hipStream_t stream);
// rt_trace_first_hit (rt_first_hit.hip): the first segment of frame a->prev_count of every pixel of the selected
// reference tiles (a->sel, or every tile), under the rule set `simd`, culled in the kernel (`cull`) or tested
// against every pair; centre: RT_HIT_PIXEL_CENTRE.  Reads of *a: the camera and the image size, groups,
// materials, n_groups, n_spheres, fast_sqrt, sel, sel_tiles_x and tiles_x (= rtk_tiles_x(width, 1)).  The planes
// (DEVICE; rt_first_hit, v4 f32, v4 f32; each may be NULL, not all) are arguments of their own: TraceArgs does not grow.
extern "C" int rtk_launch_first_hit(const TraceArgs *a, int simd, int cull, int centre, void *hit, float *normal,
                                    float *albedo, hipStream_t stream);
// One pass of rt_denoise (rt_denoise.hip; the filter is defined in rt_trace.h): src -> dst at `step`.
struct DenoiseArgs {
    const float *src;     // I_i (pass 0: Mean), v4 f32
    float *dst;           // I_{i+1}
    const void *hit;      // rt_first_hit per pixel
    const float *normal;  // read when normal_power != 0
    const float *albedo;  // read when demod_in or remod_out
    uint32_t *rgba8;      // written when non-NULL (the last pass alone names it)
    uint32_t width, height, step;
    uint32_t normal_power;   // k: d^(2^k)
    float sigma_depth, ic;   // 0: that stop is off
    uint32_t demod_in;       // pass 0 of RT_DENOISE_DEMODULATE: every tap read is Mean / a
    uint32_t remod_out;      // its last pass: the result is multiplied by the centre's a
    uint32_t srgb_pow;
};
extern "C" int rtk_launch_denoise_pass(const DenoiseArgs *a, hipStream_t stream);
// rt_reproject (rt_reproject.hip; the pass is defined in rt_trace.h): one launch, one thread per pixel.  Both
// cameras and the host's constants (rt_plan.cpp plan_reproject) travel by value.
struct ReprojectArgs {
    const float *mean;            // v4 f32, the fresh mean
    const void *hit;              // rt_first_hit per pixel, at the new camera
    const float *history;         // v4 f32, or NULL: no history (history_hit and history_count are NULL with it)
    const void *history_hit;      // rt_first_hit per pixel, at the previous camera
    const uint32_t *history_count;
    float *out;
    uint32_t *out_count;
    uint32_t *rgba8;              // written when non-NULL
    uint32_t width, height, frames, max_history;
    float depth_tolerance;        // 0: no depth test
    uint32_t srgb_pow;
    float cam_pos[3], cam_x[3], cam_y[3], film_center[3], film_w, film_h;  // the new camera
    float prev_pos[3], prev_x[3], prev_y[3], prev_film_w, prev_film_h;     // the previous camera
    float fv[3], ff;              // FilmCenter' - CameraPosition' and its squared length
    float wf, hf, hw, hh;         // (f32)Width, (f32)Height and their halves
};
extern "C" int rtk_launch_reproject(const ReprojectArgs *a, hipStream_t stream);
// rt_reproject_clip (rt_reproject.hip): rt_reproject's launch with the clamp of the gathered history to the fresh
// neighbourhood's band before the fold.  One launch; a block stages its tile of mean and hit in LDS.
struct ReprojectClipArgs {
    ReprojectArgs rp;             // everything rt_reproject's launch takes
    uint32_t radius;              // 1..3: the window is (2 * radius + 1)^2 pixels of mean and hit
    float gamma;                  // the band's half-width in standard deviations
};
extern "C" int rtk_launch_reproject_clip(const ReprojectClipArgs *c, hipStream_t stream);
// Pixels of dead block tiles (live[t] == kTileDead; never kTileSkipped ones): every sample misses with no sky,
// so fold zeros into the running mean, store both images; adds
// dead_pixels[0] x a->frames segments to the ray counter once (dead_pixels:
// the cull pass's device total, so the host need not read it back).
// With a->tile_counts_at every dead block tile folds by its reference tile's own pair, and the segments
// are summed on the device: in-image pixels x the tile's frames over the dead selected block tiles,
// added to the ray counter and to *folded (required then; the caller zeroes it; dead_pixels is not read).
extern "C" int rtk_launch_empty_counts(const TraceArgs *a, int lanes_per_pixel, const uint32_t *live,
                                       unsigned long long *folded, hipStream_t stream);
extern "C" int rtk_launch_empty(const TraceArgs *a, int lanes_per_pixel, const uint32_t *live,
                                const unsigned long long *dead_pixels, hipStream_t stream);
// Per block tile, deal its pixels to its four waves by the costs the last launch
// measured (TraceArgs.pix_cost), cheapest to wave 0, so each wave's pixels finish
// their samples at about the same time; blocks with a quadrant the cull pass
// left empty keep their pixels (that quadrant's wave folds without tracing).
// perm: 64 bytes per block tile (TraceArgs.pix_perm).  P in {4, 8, 16, 32}.
extern "C" int rtk_launch_pixel_sort(const TraceArgs *a, int lanes_per_pixel, uint8_t *perm, hipStream_t stream);
// dst[0] += sum of slots[0, n) (the gathered per-device ray counters)
extern "C" int rtk_launch_sum_u64(const uint64_t *slots, uint32_t n, uint64_t *dst, hipStream_t stream);
// Restores the caller's current HIP device when a C-ABI entry point returns:
// entry points switch to their device's ordinal (hipSetDevice), and the
// caller's own HIP work must keep targeting the device it had selected.
struct DeviceGuard {
    int saved = -1;
    DeviceGuard() {
        if (hipGetDevice(&saved) != hipSuccess) {
            saved = -1;
            (void)hipGetLastError();
        }
    }
    ~DeviceGuard() {
        if (saved >= 0) (void)hipSetDevice(saved);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
extern "C" int rtk_launch_encode(const void *accum, void *out, uint64_t n, uint32_t pow_mode, hipStream_t stream);
extern "C" int rtk_launch_assemble(const void *src, uint64_t rank_stride, void *dst, uint32_t width, uint32_t height,
                                   uint32_t elem, uint32_t band_rows, uint32_t band_count, hipStream_t stream);
