// rt_plan.h — what a launch decides before it touches a device (rt_plan.cpp): the device's switches
// from rt_device_options, the uploaded scene's facts, a validated tile list, the launch plan and the
// first-launch split.  Arithmetic on plain values, no HIP call: rt_host.cpp carries a plan out,
// tests/plan_check runs the rules as a plain host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "rt_kernel.h"
#include "rt_trace.h"

// sets rt_last_error()'s text and returns `code` (rt_host.cpp)
int rt_fail(int code, const char *fmt, ...);

// rt_device_options as the launch code reads them (rt_trace.h: 0 = the default, RT_OPT_ON / RT_OPT_OFF).
struct Switches {
    int cull = 1;
    int src = kSrcSmem;
    uint32_t sec_threshold = 0;  // 0: per scene (plan_launch), else options SecondaryThreshold
    int prefilter = -1;          // options Prefilter: -1 auto, 0 off, 1 on
    int pf_rel = -1;  // options PrefilterRelative: -1 auto (where the scene-wide bound does not pay), 0 never, 1 always
    // options Clusters off (0): per-group prefilter loop only; on (2): clustered loop up to
    // kClMaxGroups groups; default 1: up to kClAutoGroups (measured: clusters
    // win 13-15 % at 16/24/32 groups on C2 geometry, and at C5's 64 groups
    // 32.4k against 28.6k Mrays/s once the behind rule and the 7-block LDS
    // image are in)
    int clusters = 1;
    int interleave = 0;     // options Interleave: wave tiles interleaved over the block tile (P >= 2)
    int scene_global = 0;   // options SceneInHbm: keep the scene in HBM even when the LDS image could hold it
    int tables_global = 0;  // options TablesInLds off: the rsqrt and fold-weight tables stay out of the LDS image
    int solo = 1;           // options OneWaveGroups off: four waves per workgroup sharing an LDS image (TraceArgs.solo)
    int wave_order = 1;     // options WaveOrder off: one-wave kernels order block tiles, not waves (A/B)
    int walk_any = 0;       // options WalkAny: the one-wave kernel dispatches the walk at run time (A/B)
    int lanes_per_pixel = 0;  // 0 = auto per launch (plan_launch), else forced by options LanesPerPixel
    // options PixelsPerLane: 0 auto (4 pixels per lane for one-lane-per-pixel launches of one
    // frame), 1 never, 4 for every one-lane-per-pixel launch (A/B and the parity suite)
    int pixels_per_lane = 0;
    // each block tile's pixels dealt to its waves by the cost the last launch
    // measured (rtk_launch_pixel_sort), at P >= 4; options PixelSort off turns it off.
    // Same box: C2 158.7-159.3k -> 164.6-166.4k Mrays/s, RTWeekend 22.4k -> 23.3k
    int pixel_sort = 1;
    // pixels per dealt unit (TraceArgs.pix_seg), options PixelSegment 1/2/4: 4-pixel row segments keep
    // each wave's stores to whole 64-B runs of the v4 image (HBM writes per launch: C2 20.9 ->
    // 17.5 MB, RTWeekend 80.2 -> 57.3 MB) but deal costs coarser: C2 -2.2 %, RTWeekend -4 %
    // (profiles/r05b_pixel_seg_ab.txt), so single pixels stay the default
    uint32_t pixel_seg = 1;
    // options XcdGroup: every wave of a block tile on one XCD (rtk_launch_xcd_group), so its lines'
    // partial stores merge in one L2 before they are written back
    // off/on forces it; by default it is on for launches of at most 4 lanes per pixel (the
    // whole frame, where it halves the trace kernel's HBM writes at no cost) and off for the multi-GPU shares
    // (8 and 16 lanes per pixel: small launches, whose partial-line writes are a few MB, and the 8-rank share
    // -2.3 % without it at the final kernel, profiles/r05z6_xcd_group_ab.txt)
    int xcd_group = -1;
    // RGBA8 encoded from the running mean by a coalesced pass after the launch (TraceArgs.skip_cur),
    // at P >= 2: trace-kernel HBM writes C2 21.0 -> 15.7 MB, RTWeekend 80.6 -> 54.1 MB, C2 +0.7 %
    // (profiles/r05e_cur_pass_ab.txt); options EncodePass off stores RGBA8 in the trace kernel
    uint32_t cur_pass = 1;
    int merge = -1;  // options MergeRounds: -1 auto (scenes of at most kMergeGroups groups), 0 never, 1 always
    // heaviest-first tile order learned from the previous launch of the same
    // geometry (options TileOrder off disables); launches must be stream-ordered
    int tile_sched = 1;
    int split = 1;              // options SplitFirstLaunch off: a key's first launch is not split (split_schedule)
    uint32_t head_samples = 8;  // samples per lane of the split's head (options HeadSamples)
    uint32_t split_parts = 2;   // launches of a split first launch (options SplitParts, <= 8)
    uint32_t split_growth = 3;  // each leading part this many times the previous (options SplitGrowth)
    // options OrderLaunches: re-sorts per key before the order is kept.  4 (a key's split first launch
    // sorts twice, then two more launches): as fast as 6 at steady state on C2 and the 8-rank share,
    // 3 is slower (profiles/r05q_order_launches_ab.txt), and a bench's timed launches are past the
    // sorting ones after two warm-ups
    uint32_t order_launches = 4;
    uint32_t cluster_k = 0, sub_spheres = 0;  // cluster_table's K and sub-cluster size (0: per scene)
    // options DirectionTable off (0): rt_scene_upload builds no direction block, so every one-word scene-wide launch
    // runs the cluster walk (kWalkCl1) as before (A/B and the parity variants); default 1: the direction walk for
    // the shapes of rtk_direction_default; on (2): for every shape with walk kernels
    int dir_table = 1;
};

// What rt_device_create_ex refuses in its options (o == NULL: nothing), before anything touches a device.
int check_options(const rt_device_options *o);
// The switches of checked options.
Switches from_options(const rt_device_options &o);

// What rt_scene_upload keeps of one rule set of the uploaded scene (the tables themselves are on the device).
struct SceneFacts {
    uint32_t n_groups = 0;
    uint32_t prefilter = 0;      // decided at upload (options Prefilter, or where it pays)
    uint32_t pf_relative = 0;    // the threshold row holds r^2, per-lane thresholds (rtk_walk.h kPfRel)
    uint32_t fast_sqrt = 0;      // candidate sqrt in sqrt_rn's verified range
    uint32_t n_cpairs = 0;       // 0: per-group prefilter loop
    uint32_t cl_words = 0;
    bool clusters_x_ok = false;  // the expanded table is proven and useful for the scene (kPrefilterExpanded)
    bool dir_table = false;      // the direction block lies behind the expanded table (kPrefilterDirection)
    // of the scene, the same in both rule sets' facts
    uint32_t n_spheres = 0;
    bool use_sky = false;
    uint64_t scene_gen = 0;      // bumped by every rt_scene_upload
};

// A validated rt_trace_tiles list (build_selection): the bitmap the kernels read and what the
// host derives from the list -- the pixels it covers (the lanes-per-pixel choice) and, by clipped
// size, how many tiles it names (the block tiles inside them, for any launch shape).
struct TileSelection {
    const uint32_t *bits = nullptr;  // one bit per reference tile (TraceArgs.sel's layout)
    uint32_t n_words = 0, tiles_x = 0, n_tiles = 0;  // bitmap words, TilesX, the image's reference tiles
    uint64_t pixels = 0;             // of the listed tiles, clipped to the image (main.cpp:362-368)
    // listed tiles by clipped size: [0] 32 x 32, [1] the ragged right column (clip_w x 32),
    // [2] the ragged bottom row (32 x clip_h), [3] the corner of both (clip_w x clip_h)
    uint32_t n_class[4] = {0, 0, 0, 0};
    uint32_t clip_w = RT_TILE_SIZE, clip_h = RT_TILE_SIZE;
    // block tiles of launch shape `lpp` inside the listed tiles
    uint32_t block_tiles(int lpp) const {
        const uint32_t T = RT_TILE_SIZE;
        return n_class[0] * rtk_tile_count(T, T, lpp) + n_class[1] * rtk_tile_count(clip_w, T, lpp) +
               n_class[2] * rtk_tile_count(T, clip_h, lpp) + n_class[3] * rtk_tile_count(clip_w, clip_h, lpp);
    }
};

// Validates a tile list against a width x height image and builds its bitmap into `bits`
// (no allocation beyond the vector's growth).  Returns 0, or -1 for an index past the image's
// tiles (*bad = its position in the list), -2 for an index named twice.
int build_selection(const uint32_t *tiles, uint32_t n_tiles, uint32_t width, uint32_t height,
                    std::vector<uint32_t> &bits, TileSelection &sel, uint32_t *bad);

// How an entry point spells its list in an error text: "rt_trace_tiles" and tiles[%u], or
// "rt_trace_tile_work" and work[%u].Tile.
struct ListName {
    const char *api, *open, *close;
};
// build_selection with its two refusals as the entry point `name` words them.
int select_tiles(const ListName &name, const uint32_t *tiles, uint32_t n_tiles, uint32_t width, uint32_t height,
                 std::vector<uint32_t> &bits, TileSelection &sel);

// What rt_trace refuses before it looks at the images (rt_trace_tiles and rt_trace_tile_work refuse
// the same).  have_device, lut_set, scene_set: the rt_device handle's state.
int check_trace_args(bool have_device, bool lut_set, bool scene_set, const rt_camera_info *cam,
                     const rt_trace_desc *desc, const uint64_t *d_rays);

// rt_trace_tile_work's list without the device: the kept entries (Frames > 0) as a selection and a
// counts table (TraceArgs.tile_counts_at's layout; {0, 0} for a tile outside the selection, which
// nothing reads).  The vectors are the caller's, reused from call to call.
struct TileWorkList {
    std::vector<uint32_t> tiles, bits, table;
    TileSelection sel;
    uint32_t kept = 0;        // 0: nothing to launch
    bool uniform = true;      // the kept entries share one pair: `first`
    rt_tile_work first{};
    uint32_t max_frames = 0;  // the launch shape's frames when they do not
};
int plan_tile_work(const rt_tile_work *work, uint32_t n_work, uint32_t width, uint32_t height, TileWorkList &out);

// rt_trace_tile_counts without the device: everything the call refuses (rt_trace_tiles' refusals, a NULL
// table, max_frames 0, a misaligned d_delta; the pointers are compared, never followed), its list as a
// selection (the launch key's, as rt_trace_tiles builds it: nothing of the table enters it) and the
// descriptor the launch is planned with -- desc with PreviousRayCount 0 and Frames = max_frames, the bound
// that takes the place of the list's largest Frames in the launch shape.  `bits` is the caller's, reused.
struct TileCountsCall {
    TileSelection sel;
    rt_trace_desc desc{};
    bool nothing = false;  // n_tiles == 0: RT_OK, nothing to launch
};
int plan_tile_counts(bool have_device, bool lut_set, bool scene_set, const rt_camera_info *cam, const rt_trace_desc *desc,
                     const uint32_t *tiles, uint32_t n_tiles, const void *d_counts, uint32_t max_frames,
                     const void *d_delta, const uint64_t *d_rays, std::vector<uint32_t> &bits, TileCountsCall &out);
// What rt_tile_counts_step refuses; *n_tiles = the image's reference tiles.
int check_tile_step(const void *d_counts, const void *d_delta, uint32_t width, uint32_t height, const rt_tile_rule *rule,
                    uint32_t *n_tiles);

// rt_trace_first_hit without the device: everything the call refuses (the planes' pointers are compared,
// never followed) and its list as a selection, built by select_tiles as rt_trace_tiles builds its own.
// `bits` is the caller's, reused; it belongs to this pass (the launch key's bitmap is another vector).
struct FirstHitCall {
    TileSelection sel;     // (all: no bitmap, only the image's tile counts)
    bool all = false;      // tiles == NULL with n_tiles == 0: every tile of the image
    bool nothing = false;  // a list with n_tiles == 0: RT_OK, nothing to launch
};
int plan_first_hit(bool have_device, bool scene_set, const rt_camera_info *cam, const rt_trace_desc *desc,
                   const uint32_t *tiles, uint32_t n_tiles, uint32_t flags, const rt_first_hit_planes *out,
                   std::vector<uint32_t> &bits, FirstHitCall &call);

// rt_denoise without a device: everything the call refuses (the planes' pointers are compared, never followed)
// and its passes in launch order.  Pass i reads `src` and writes `dst` at step 1 << i with the colour stop's
// ic = ic0 * (float)step (ic0 = 1.0f / SigmaColor, or 0 without a colour stop); pass 0 reads Mean, every later
// pass what the one before it wrote, and Scratch and Out alternate so that the last pass writes Out.
struct DenoisePass {
    const float *src = nullptr;
    float *dst = nullptr;
    uint32_t step = 0;
    float ic = 0.0f;
};
struct DenoisePlan {
    DenoisePass pass[RT_DENOISE_MAX_ITERATIONS];
    uint32_t n_passes = 0;
    float ic0 = 0.0f;
};
int plan_denoise(const rt_denoise_desc *desc, DenoisePlan &plan);

// rt_reproject without a device: everything the call refuses (the planes' pointers are compared, never followed;
// the two cameras are HOST structs and are read) and the launch's arguments: the planes, the counts, both
// cameras' fields and the constants the host forms once, each one f32 operation as rt_trace.h lists them --
// fv = FilmCenter' - CameraPosition', ff = dot3(fv, fv), wf = (float)Width, hf = (float)Height, hw = wf * 0.5f,
// hh = hf * 0.5f.  A refused call leaves `args` as it was.
int plan_reproject(const rt_reproject_desc *desc, ReprojectArgs &args);
// rt_reproject_clip without a device, on plan_reproject: the outer desc's own refusals (NULL, Size, Radius outside
// 1..3, a Gamma that is not finite or not > 0), then everything plan_reproject refuses for desc->Reproject, with its
// texts; args.rp is plan_reproject's result, radius and gamma the desc's.  A refused call leaves `args` as it was.
int plan_reproject_clip(const rt_reproject_clip_desc *desc, ReprojectClipArgs &args);

// Which table TraceArgs.clusters names.
enum { kTableNone = 0, kTablePlain, kTableExpanded };
// The rule set's two cluster tables on the device: opaque to the plan, which only chooses between them.
struct TablePointers {
    const float4 *plain = nullptr, *expanded = nullptr;
};

struct LaunchPlan {
    uint32_t lanes = 0;  // lanes per pixel (the sample chains of a pixel)
    int lpp = 0;         // the launch shape code of rtk_* (0: pixels per lane)
    uint32_t pixels_per_lane = 1;
    uint32_t interleave = 0, lut_in_lds = 0, fold_in_lds = 0, scene_in_lds = 0;
    uint32_t solo = 0, walk = 0;
    int table = kTableNone;
    uint32_t prefilter = 0;  // kPrefilter*
    uint32_t merge_rounds = 0, sec_threshold = 0;
    int src = kSrcSmem;
    uint32_t unit_waves = 0;
    // block tiles of the band, units of the heaviest-first order, block tiles inside the listed
    // tiles (every tile's without a list), block tiles per row
    uint32_t n_tiles = 0, n_units = 0, n_selected = 0, tiles_x = 0;
    uint32_t n_words = 0;   // cull-mask words per wave tile
    size_t mask_words = 0;  // of the whole launch
    bool cull = false, empty_capable = false, sched = false, pixel_sort = false, xcd_group = false;
    uint32_t skip_cur = 0;
};

// Every decision of a launch that needs no device.  `a` holds the camera and the descriptor
// (rt_host.cpp fill_args) and receives the decided fields; `key` receives the words the launch's
// masks, live list and order depend on (cleared first; the caller keeps and reuses the vector, so
// nothing is allocated per launch once it has grown).  counts, delta: rt_trace_tile_work with
// mixed pairs, rt_trace_tile_work_delta -- neither enters the key.
LaunchPlan plan_launch(const Switches &sw, const SceneFacts &sf, int rs, uint32_t cu_count, const rt_trace_desc &desc,
                       uint32_t local_rows, const TileSelection *sel, bool counts, bool delta,
                       const TablePointers &tables, TraceArgs &a, std::vector<uint32_t> &key);

// One launch, or the split of a key's first launch: the frames of each part in order
// (n_parts >= 1, none empty) and the frames of the leading parts together.
struct SplitSchedule {
    uint32_t parts[8];
    uint32_t n_parts = 0;
    uint32_t head_frames = 0;
};
SplitSchedule split_schedule(uint32_t frames, uint32_t lanes, uint32_t head_samples, uint32_t split_parts,
                             uint32_t split_growth, bool may_split);
