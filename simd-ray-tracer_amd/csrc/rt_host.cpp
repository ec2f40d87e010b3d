// rt_host.cpp — C-ABI host side: device context, scene upload, trace launch,
// band assembly.  Plain HIP runtime; no torch types cross this boundary.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rt_kernel.h"
#include "rt_pack.h"
#include "rt_trace.h"

// Two pinned slots the library owns, from which words a launch reads on the device are uploaded.
// Each slot is guarded by an event recorded after its copy and is rewritten only once that copy has
// finished (staged_upload), so the caller's array is free when the call returns and back-to-back
// calls do not wait for each other.
struct StagedWords {
    uint32_t *h[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool in_flight[2] = {false, false};
    uint32_t slot = 0;
};

struct rt_device {
    int ordinal = 0;
    hipStream_t stream = nullptr;
    float *d_lut = nullptr;                // 2048 f32
    bool lut_set = false;
    // SIMD rule set (SIMDSpheres + Materials) and scalar rule set (ScalarSpheres)
    float4 *d_groups[2] = {nullptr, nullptr};
    float2 *d_weights = nullptr;  // TraceArgs.weights: kWeightsN running-mean weight pairs
    // the primary rounds' camera-relative group rows (TraceArgs.prim), written by the cull pass
    float4 *d_prim[2] = {nullptr, nullptr};
    float4 *d_mats[2] = {nullptr, nullptr};
    uint32_t n_groups[2] = {0, 0};
    uint32_t n_spheres = 0;
    size_t cap_groups[2] = {0, 0};
    bool scene_set = false;
    bool use_sky = false;
    int src = kSrcSmem;
    int cull = 1;
    uint32_t sec_threshold = 0;  // 0: per scene (rt_trace), else rt_device_options SecondaryThreshold
    int prefilter_env = -1;  // options Prefilter: -1 auto, 0 off, 1 on
    uint32_t prefilter[2] = {0, 0};  // per rule set, decided at upload
    uint32_t pf_relative[2] = {0, 0};  // per rule set: the threshold row holds r^2, per-lane thresholds (rtk_walk.h kPfRel)
    int pf_rel_env = -1;  // options PrefilterRelative: -1 auto (where the scene-wide bound does not pay), 0 never, 1 always
    uint32_t fast_sqrt[2] = {0, 0};  // per rule set: candidate sqrt in sqrt_rn's verified range
    float4 *d_clusters[2] = {nullptr, nullptr};  // clustered prefilter tables (rt_pack.cpp cluster_table)
    size_t cap_clusters[2] = {0, 0};             // float4 capacity
    uint32_t n_cpairs[2] = {0, 0};               // 0: per-group prefilter loop
    float4 *d_clusters_x[2] = {nullptr, nullptr};  // the expanded tables, {c0, 0} then the entries (rt_pack.cpp expand_table)
    size_t cap_clusters_x[2] = {0, 0};             // float4 capacity
    bool clusters_x_ok[2] = {false, false};        // proven and useful for the uploaded scene (kPrefilterExpanded)
    uint32_t cl_words[2] = {0, 0};
    // options Clusters off (0): per-group prefilter loop only; on (2): clustered loop up to
    // kClMaxGroups groups; default 1: up to kClAutoGroups (measured: clusters
    // win 13-15 % at 16/24/32 groups on C2 geometry, and at C5's 64 groups
    // 32.4k against 28.6k Mrays/s once the behind rule and the 7-block LDS
    // image are in)
    int clusters_env = 1;
    int interleave_env = 0;  // options Interleave: wave tiles interleaved over the block tile (P >= 2)
    int scene_global_env = 0;  // options SceneInHbm: keep the scene in HBM even when the LDS image could hold it
    int tables_global_env = 0;  // options TablesInLds off: the rsqrt and fold-weight tables stay out of the LDS image
    int solo_env = 1;           // options OneWaveGroups off: four waves per workgroup sharing an LDS image (TraceArgs.solo)
    int wave_order_env = 1;     // options WaveOrder off: one-wave kernels order block tiles, not waves (A/B)
    int walk_any_env = 0;       // options WalkAny: the one-wave kernel dispatches the walk at run time (A/B)
    int lanes_per_pixel = 0;  // 0 = auto per launch (rt_trace), else forced by options LanesPerPixel
    // options PixelsPerLane: 0 auto (4 pixels per lane for one-lane-per-pixel launches of one
    // frame), 1 never, 4 for every one-lane-per-pixel launch (A/B and the parity suite)
    int pixels_per_lane_env = 0;
    // each block tile's pixels dealt to its waves by the cost the last launch
    // measured (rtk_launch_pixel_sort), at P >= 4; options PixelSort off turns it off.
    // Same box: C2 158.7-159.3k -> 164.6-166.4k Mrays/s, RTWeekend 22.4k -> 23.3k
    int pixel_sort_env = 1;
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
    int xcd_group_env = -1;
    // RGBA8 encoded from the running mean by a coalesced pass after the launch (TraceArgs.skip_cur),
    // at P >= 2: trace-kernel HBM writes C2 21.0 -> 15.7 MB, RTWeekend 80.6 -> 54.1 MB, C2 +0.7 %
    // (profiles/r05e_cur_pass_ab.txt); options EncodePass off stores RGBA8 in the trace kernel
    uint32_t cur_pass = 1;
    int merge_env = -1;  // options MergeRounds: -1 auto (scenes of at most kMergeGroups groups), 0 never, 1 always
    uint8_t *d_pix_perm = nullptr;  // 64 B per block tile (TraceArgs.pix_perm)
    uint32_t *d_pix_cost = nullptr; // per band pixel (TraceArgs.pix_cost)
    size_t pix_perm_cap = 0, pix_cost_cap = 0;
    // heaviest-first tile order learned from the previous launch of the same
    // geometry (options TileOrder off disables); launches must be stream-ordered
    int tile_sched = 1;
    uint32_t n_sorts = 0;             // re-sorts done for the current tile key
    int split_env = 1;                // options SplitFirstLaunch off: a key's first launch is not split (below)
    uint32_t head_samples = 8;        // samples per lane of the split's head (options HeadSamples)
    uint32_t split_parts = 2;         // launches of a split first launch (options SplitParts, <= 8)
    uint32_t split_growth = 3;        // each leading part this many times the previous (options SplitGrowth)
    // options OrderLaunches: re-sorts per key before the order is kept.  4 (a key's split first launch
    // sorts twice, then two more launches): as fast as 6 at steady state on C2 and the 8-rank share,
    // 3 is slower (profiles/r05q_order_launches_ab.txt), and a bench's timed launches are past the
    // sorting ones after two warm-ups
    uint32_t order_launches = 4;
    uint32_t *d_tile_cost = nullptr, *d_tile_order = nullptr, *d_tile_scratch = nullptr;
    uint32_t *d_tile_order_sorted = nullptr;  // the sort's output before XCD grouping (rtk_launch_xcd_group)
    uint32_t *d_tile_aux = nullptr;           // XCD grouping: per block tile, first sorted position and group
    uint32_t *d_tile_live = nullptr;
    unsigned long long *d_cull_counters = nullptr;  // kCullCounterWords: striped counters + device totals of the cull pass
    uint64_t *d_masks = nullptr;  // cull pass output: per wave tile primary group masks
    size_t tile_cap = 0, mask_cap = 0;
    // rt_device_reserve: the most block tiles (over every lanes-per-pixel shape)
    // and band pixels of any geometry reserved so far (0: none)
    uint32_t reserve_tiles = 0;
    size_t reserve_pixels = 0;
    size_t mask_words = 0;  // words the last cull pass wrote (rt_debug_masks)
    // the launch (camera, scene, geometry) the masks / live list / order were made for
    std::vector<uint32_t> tile_key;
    bool tile_order_valid = false;
    // The cull pass's totals travel to the host asynchronously (pinned h_counts,
    // event ev_counts): a new key never blocks the host.  Until they have
    // landed (counts_known), launches size their grids for every tile and read
    // the live count on the device (TraceArgs.live_total).
    uint32_t n_live = 0;
    uint64_t dead_pixels = 0;
    bool counts_known = true;
    unsigned long long *h_counts = nullptr;  // pinned {live tiles, dead pixels}
    hipEvent_t ev_counts = nullptr;
    // rt_trace_tiles: the selection bitmap of the current tile key on the device (TraceArgs.sel; its
    // words are part of tile_key, so keys compare by the lists' content).  A new key's bitmap is
    // uploaded from one of two pinned slots, each guarded by an event recorded after its copy: a
    // slot is rewritten only once that copy has finished (staged_upload).
    // rt_trace_tile_work: the per-tile {PreviousRayCount, Frames} table of a launch with mixed counts
    // (TraceArgs.tile_counts_at: two words per reference tile of the image) lies behind the bitmap in
    // d_sel (rt_kernel.h rtk_sel_table_at) and is uploaded on EVERY such call -- the counts are no part
    // of the key -- through two pinned slots of its own, by the same scheme
    uint32_t *d_sel = nullptr;
    StagedWords sel, counts;
    uint32_t sel_cap = 0;            // reference tiles d_sel and the pinned slots are sized for
    uint32_t reserve_ref_tiles = 0;  // rt_device_reserve: the most reference tiles of any geometry reserved
    std::vector<uint32_t> sel_bits;  // rt_trace_tiles builds the call's bitmap here (no allocation per call)
    std::vector<uint32_t> work_tiles, counts_table;  // the call's tile list and table (no allocation per call)
    // such a launch's folded segments are summed on the device (d_cull_counters[kCullFolded]) and
    // follow to the host like the cull totals: pinned h_folded, event ev_folded
    unsigned long long *h_folded = nullptr;
    hipEvent_t ev_folded = nullptr;
    bool last_folded_on_device = false;  // the last launch's SegmentsFolded is h_folded's (rt_trace_last_info)
    bool last_tile_counts = false;       // the last launch took per-tile counts (rt_trace_last_tile_counts)
    uint64_t scene_gen = 0;  // bumped by every rt_scene_upload
    // the last stream rt_trace ran on (a switch waits for the device: below)
    hipStream_t tile_stream = nullptr;
    bool tile_stream_set = false;
    // what rt_trace_last_info resolves lazily (the folded segments need the counts)
    uint32_t last_n_tiles = 0, last_frames = 0;
    bool last_empty_capable = false;
    uint32_t cu_count = 256;
    unsigned long long *d_stats = nullptr;  // RT_STATS=1: per-launch scheduling counters
    unsigned long long *d_wave_times = nullptr;  // RT_WAVETIMES=1: per-wave start/end of the last launch
    size_t wave_times_cap = 0;
    bool want_wave_times = false;
    rt_trace_info last{};  // what the last rt_trace launched (rt_trace_last_info)
    rt_device_options opt{};  // as created (rt_device_get_options)
    uint32_t cluster_k = 0, sub_spheres = 0;  // cluster_table's K and sub-cluster size (0: per scene)
};

static thread_local char g_err[512];

static int vfail(int code, const char *fmt, va_list ap) {
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    return code;
}

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfail(code, fmt, ap);
    va_end(ap);
    return code;
}

// rt_pack.h: the error text other translation units (rt_pack.cpp, rt_multi.cpp) report
int rt_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfail(code, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_OK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(RT_EIO, "%s: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

extern "C" const char *rt_last_error(void) { return g_err; }

extern "C" int rt_device_create(int hip_device, rt_device **out) { return rt_device_create_ex(hip_device, nullptr, out); }

// rt_device_options -> the device's switches (rt_trace.h: 0 = the default, RT_OPT_ON / RT_OPT_OFF)
static int apply_options(rt_device *d, const rt_device_options *o) {
    if (!o) return RT_OK;
    if (o->Size != 0 && o->Size != sizeof(rt_device_options))
        return fail(RT_EINVAL, "rt_device_options: Size %u, this library's is %zu", o->Size, sizeof(rt_device_options));
    const int32_t tri[] = {o->Cull, o->Prefilter, o->PrefilterRelative, o->Clusters, o->OneWaveGroups,
                           o->SphereSourceLds, o->SceneInHbm, o->TablesInLds, o->WalkAny, o->Interleave,
                           o->MergeRounds, o->TileOrder, o->WaveOrder, o->PixelSort, o->XcdGroup,
                           o->SplitFirstLaunch, o->EncodePass};
    for (const int32_t v : tri)
        if (v < -1 || v > 1) return fail(RT_EINVAL, "rt_device_options: a switch is %d (RT_OPT_DEFAULT/ON/OFF)", v);
    const int32_t lpp = o->LanesPerPixel;
    if (!(lpp == 0 || lpp == 1 || lpp == 2 || lpp == 4 || lpp == 8 || lpp == 16 || lpp == 32))
        return fail(RT_EINVAL, "rt_device_options: LanesPerPixel %d", lpp);
    if (!(o->PixelsPerLane == 0 || o->PixelsPerLane == 1 || o->PixelsPerLane == 4))
        return fail(RT_EINVAL, "rt_device_options: PixelsPerLane %d", o->PixelsPerLane);
    if (!(o->PixelSegment == 0 || o->PixelSegment == 1 || o->PixelSegment == 2 || o->PixelSegment == 4))
        return fail(RT_EINVAL, "rt_device_options: PixelSegment %d", o->PixelSegment);
    if (o->SplitParts < 0 || o->SplitParts > 8 || o->HeadSamples < 0 || o->SplitGrowth < 0 || o->OrderLaunches < -1 ||
        o->SecondaryThreshold < 0 || o->SecondaryThreshold > 64 || o->ClusterCount < 0 || o->ClusterCount == 1 ||
        o->SubClusterSpheres < 0)
        return fail(RT_EINVAL, "rt_device_options: a count is out of range");
    auto on = [](int32_t v, bool dflt) { return v == RT_OPT_DEFAULT ? dflt : v == RT_OPT_ON; };
    d->opt = *o;
    d->opt.Size = sizeof(rt_device_options);
    d->cull = on(o->Cull, true) ? 1 : 0;
    d->prefilter_env = o->Prefilter == RT_OPT_DEFAULT ? -1 : o->Prefilter == RT_OPT_ON ? 1 : 0;
    d->pf_rel_env = o->PrefilterRelative == RT_OPT_DEFAULT ? -1 : o->PrefilterRelative == RT_OPT_ON ? 1 : 0;
    d->clusters_env = o->Clusters == RT_OPT_DEFAULT ? 1 : o->Clusters == RT_OPT_ON ? 2 : 0;
    d->cluster_k = (uint32_t)o->ClusterCount;
    d->sub_spheres = (uint32_t)o->SubClusterSpheres;
    d->sec_threshold = (uint32_t)o->SecondaryThreshold;
    d->lanes_per_pixel = lpp;
    d->pixels_per_lane_env = o->PixelsPerLane;
    d->solo_env = on(o->OneWaveGroups, true) ? 1 : 0;
    d->src = on(o->SphereSourceLds, false) ? kSrcLds : kSrcSmem;
    d->scene_global_env = on(o->SceneInHbm, false) ? 1 : 0;
    d->tables_global_env = on(o->TablesInLds, true) ? 0 : 1;
    d->walk_any_env = on(o->WalkAny, false) ? 1 : 0;
    d->interleave_env = on(o->Interleave, false) ? 1 : 0;
    d->merge_env = o->MergeRounds == RT_OPT_DEFAULT ? -1 : o->MergeRounds == RT_OPT_ON ? 1 : 0;
    d->tile_sched = on(o->TileOrder, true) ? 1 : 0;
    d->wave_order_env = on(o->WaveOrder, true) ? 1 : 0;
    d->pixel_sort_env = on(o->PixelSort, true) ? 1 : 0;
    if (o->PixelSegment) d->pixel_seg = (uint32_t)o->PixelSegment;
    d->xcd_group_env = o->XcdGroup == RT_OPT_DEFAULT ? -1 : o->XcdGroup == RT_OPT_ON ? 1 : 0;
    d->split_env = on(o->SplitFirstLaunch, true) ? 1 : 0;
    if (o->HeadSamples) d->head_samples = (uint32_t)o->HeadSamples;
    if (o->SplitParts) d->split_parts = (uint32_t)o->SplitParts;
    if (o->SplitGrowth) d->split_growth = (uint32_t)o->SplitGrowth;
    if (o->OrderLaunches) d->order_launches = o->OrderLaunches < 0 ? 0u : (uint32_t)o->OrderLaunches;
    d->cur_pass = on(o->EncodePass, true) ? 1u : 0u;
    return RT_OK;
}

extern "C" int rt_device_get_options(rt_device *d, rt_device_options *out) {
    if (!d || !out) return fail(RT_EINVAL, "rt_device_get_options: NULL argument");
    *out = d->opt;
    return RT_OK;
}

extern "C" int rt_device_create_ex(int hip_device, const rt_device_options *options, rt_device **out) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!out) return fail(RT_EINVAL, "rt_device_create: out is NULL");
    {  // options are checked before anything touches a device (a host-only rt_device)
        rt_device probe;
        if (const int rc = apply_options(&probe, options)) return rc;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(RT_ENODEV, "rt_device_create: no HIP device visible");
    if (hip_device < 0 || hip_device >= count) return fail(RT_EINVAL, "rt_device_create: bad device %d", hip_device);
    HIP_OK(hipSetDevice(hip_device));
    rt_device *d = new rt_device();
    d->ordinal = hip_device;
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&d->d_lut, 2048 * sizeof(float)) != hipSuccess ||
        hipMalloc(&d->d_weights, kWeightsN * sizeof(float2)) != hipSuccess ||
        hipHostMalloc(&d->h_counts, 2 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_counts, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(&d->h_folded, sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_folded, hipEventDisableTiming) != hipSuccess) {
        rt_device_destroy(d);
        return fail(RT_ENOMEM, "rt_device_create: stream/LUT/event allocation failed");
    }
    {
        // IEEE f32 divisions (this file is built with -ffp-contract=off): the bits of the kernel's
        // rcp_rn / div_rn weights, which reproduce the reference's divisions (main.cpp:484-487)
        std::vector<float2> w(kWeightsN);
        for (uint32_t n = 0; n < kWeightsN; ++n) {
            const float d1 = (float)(n + 1u);
            w[n] = make_float2(1.0f / d1, (float)n / d1);
        }
        if (hipMemcpy(d->d_weights, w.data(), kWeightsN * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) {
            rt_device_destroy(d);
            return fail(RT_EIO, "rt_device_create: weight table upload failed");
        }
    }
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, hip_device) == hipSuccess && prop.multiProcessorCount > 0)
            d->cu_count = (uint32_t)prop.multiProcessorCount;
    }
    if (const int rc = apply_options(d, options)) {
        rt_device_destroy(d);
        return rc;
    }
    // diagnostic hooks only (the -DRTK_STATS build's counters, per-wave timestamps): what is
    // computed, and how, is fixed by the options
    const char *wt = getenv("RT_WAVETIMES");
    d->want_wave_times = wt && wt[0] == '1';
    const char *st = getenv("RT_STATS");
    if (st && st[0] == '1' && hipMalloc(&d->d_stats, kStatSlots * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(d->d_stats, 0, kStatSlots * sizeof(unsigned long long));
    *out = d;
    return RT_OK;
}

extern "C" int rt_device_destroy(rt_device *d) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d) return RT_OK;
    (void)hipSetDevice(d->ordinal);
    // the caller's trace stream may already be gone: wait for the whole device
    (void)hipDeviceSynchronize();
    for (int r = 0; r < 2; ++r) {
        (void)hipFree(d->d_groups[r]);
        (void)hipFree(d->d_prim[r]);
        (void)hipFree(d->d_mats[r]);
        (void)hipFree(d->d_clusters[r]);
        (void)hipFree(d->d_clusters_x[r]);
    }
    (void)hipFree(d->d_lut);
    (void)hipFree(d->d_weights);
    (void)hipFree(d->d_stats);
    (void)hipFree(d->d_wave_times);
    (void)hipFree(d->d_tile_cost);
    (void)hipFree(d->d_tile_order);
    (void)hipFree(d->d_tile_order_sorted);
    (void)hipFree(d->d_tile_aux);
    (void)hipFree(d->d_tile_scratch);
    (void)hipFree(d->d_tile_live);
    (void)hipFree(d->d_cull_counters);
    (void)hipFree(d->d_masks);
    (void)hipFree(d->d_pix_perm);
    (void)hipFree(d->d_pix_cost);
    (void)hipFree(d->d_sel);
    for (StagedWords *w : {&d->sel, &d->counts}) {
        for (int i = 0; i < 2; ++i) {
            if (w->h[i]) (void)hipHostFree(w->h[i]);
            if (w->ev[i]) (void)hipEventDestroy(w->ev[i]);
        }
    }
    if (d->h_folded) (void)hipHostFree(d->h_folded);
    if (d->ev_folded) (void)hipEventDestroy(d->ev_folded);
    if (d->h_counts) (void)hipHostFree(d->h_counts);
    if (d->ev_counts) (void)hipEventDestroy(d->ev_counts);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
    return RT_OK;
}

static int apply_reserve(rt_device *d);  // (rt_device_reserve, below)

// rt_trace is asynchronous on the caller's stream, while uploads go through
// the device's own non-blocking stream: before a buffer a trace may still
// read (scene groups, materials, cluster table, rsqrt table) is overwritten,
// every launch issued so far must have finished.  The wait is for the whole
// device, not on the caller's stream, which the caller may have destroyed
// since (and no per-launch event is recorded for it: an event marker between
// consecutive launches measured 4.6 us of dispatch gap, 0.6 % of an 8-GPU
// band share).  Uploads are rare; the extra wait for unrelated work is the price.
static int quiesce(rt_device *d) {
    (void)d;
    HIP_OK(hipDeviceSynchronize());
    return RT_OK;
}

// Brings the cull pass's totals to the host once they have landed (wait:
// block until they have).  Returns whether they are known.
static bool resolve_counts(rt_device *d, bool wait) {
    if (d->counts_known) return true;
    if (wait) {
        if (hipEventSynchronize(d->ev_counts) != hipSuccess) return false;
    } else {
        const hipError_t q = hipEventQuery(d->ev_counts);
        if (q != hipSuccess) {
            (void)hipGetLastError();  // "not ready" must not reach a later launch check
            return false;
        }
    }
    d->n_live = (uint32_t)d->h_counts[0];
    d->dead_pixels = d->h_counts[1];
    d->counts_known = true;
    return true;
}

extern "C" int rt_set_rsqrt_table(rt_device *d, const float table[2048]) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !table) return fail(RT_EINVAL, "rt_set_rsqrt_table: NULL argument");
    HIP_OK(hipSetDevice(d->ordinal));
    if (const int rc = quiesce(d)) return rc;
    HIP_OK(hipMemcpyAsync(d->d_lut, table, 2048 * sizeof(float), hipMemcpyHostToDevice, d->stream));
    HIP_OK(hipStreamSynchronize(d->stream));
    d->lut_set = true;
    return RT_OK;
}

// One packed rule set's group rows and sphere records (rt_pack.cpp pack_set; rt_layout.h) to the device.
static int upload_set(rt_device *d, int rs, const std::vector<float> &groups, const std::vector<float> &mats,
                      uint32_t n_groups) {
    if (n_groups > d->cap_groups[rs]) {
        (void)hipFree(d->d_groups[rs]);
        (void)hipFree(d->d_mats[rs]);
        (void)hipFree(d->d_prim[rs]);
        d->d_groups[rs] = nullptr;
        d->d_mats[rs] = nullptr;
        d->d_prim[rs] = nullptr;
        // +2 padding groups: the kernel's loops prefetch up to group g+2 while testing g
        if (hipMalloc(&d->d_groups[rs], (size_t)(n_groups + 2) * kGroupF4 * 16) != hipSuccess ||
            hipMalloc(&d->d_mats[rs], (size_t)n_groups * 64u * kSphereF4) != hipSuccess ||
            hipMalloc(&d->d_prim[rs], (size_t)n_groups * kPrimF4 * 16) != hipSuccess)
            return fail(RT_ENOMEM, "rt_scene_upload: device allocation failed");
        d->cap_groups[rs] = n_groups;
    }
    HIP_OK(hipMemsetAsync(d->d_groups[rs] + kGroupF4 * (size_t)n_groups, 0, 2 * kGroupF4 * 16, d->stream));
    HIP_OK(hipMemcpyAsync(d->d_groups[rs], groups.data(), (size_t)n_groups * kGroupF4 * 16, hipMemcpyHostToDevice,
                          d->stream));
    HIP_OK(hipMemcpyAsync(d->d_mats[rs], mats.data(), (size_t)n_groups * 64u * kSphereF4, hipMemcpyHostToDevice,
                          d->stream));
    d->n_groups[rs] = n_groups;
    return RT_OK;
}

// A cluster table's device buffer grown to hold `tab` (the stream's copies into the old one wait first),
// and the table, if there is one, copied into it on the device's stream.
static int upload_table(rt_device *d, float4 *&buf, size_t &cap, const std::vector<float> &tab) {
    const size_t nf4 = tab.size() / 4u;
    if (nf4 > cap) {
        HIP_OK(hipStreamSynchronize(d->stream));
        (void)hipFree(buf);
        buf = nullptr;
        cap = 0;
        if (hipMalloc(&buf, nf4 * 16u) != hipSuccess) return fail(RT_ENOMEM, "rt_scene_upload: device allocation failed");
        cap = nf4;
    }
    if (nf4) HIP_OK(hipMemcpyAsync(buf, tab.data(), nf4 * 16u, hipMemcpyHostToDevice, d->stream));
    return RT_OK;
}

extern "C" int rt_scene_upload(rt_device *d, const rt_scene *scene) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !scene) return fail(RT_EINVAL, "rt_scene_upload: NULL argument");
    PackedSet ps[2];
    for (int rs = 0; rs < 2; ++rs) {
        const int rc = pack_set(scene, rs, ps[rs], d->pf_rel_env, d->cluster_k, d->sub_spheres);
        if (rc) return rc;
    }
    HIP_OK(hipSetDevice(d->ordinal));
    if (const int rc = quiesce(d)) return rc;
    for (int rs = 0; rs < 2; ++rs) {
        d->prefilter[rs] = d->prefilter_env < 0 ? ((ps[rs].prefilter_pays || ps[rs].relative) ? 1u : 0u)
                                                : (uint32_t)d->prefilter_env;
        d->pf_relative[rs] = ps[rs].relative ? 1u : 0u;
        d->fast_sqrt[rs] = ps[rs].fast_sqrt;
        const int rc = upload_set(d, rs, ps[rs].groups, ps[rs].mats, ps[rs].n_groups);
        if (rc) return rc;
        const ClusterTable &cl = ps[rs].cl;  // (without a table, tab and xtab are empty: rt_pack.h)
        d->n_cpairs[rs] = 0;
        if (const int rc2 = upload_table(d, d->d_clusters[rs], d->cap_clusters[rs], cl.tab)) return rc2;
        if (!cl.tab.empty()) {
            d->n_cpairs[rs] = cl.n_cpairs;
            d->cl_words[rs] = cl.words;
        }
        d->clusters_x_ok[rs] = false;
        if (const int rc2 = upload_table(d, d->d_clusters_x[rs], d->cap_clusters_x[rs], cl.xtab)) return rc2;
        d->clusters_x_ok[rs] = !cl.xtab.empty() && cl.x_ok;
    }
    HIP_OK(hipStreamSynchronize(d->stream));
    d->n_spheres = scene->ScalarSpheres.Count;
    d->use_sky = scene->UseSkyColor;
    d->scene_set = true;
    d->scene_gen += 1;
    // a reserved geometry keeps its promise for the new scene's mask words (the
    // device is quiescent here: the upload waited for every launch).  The scene
    // is committed by now, so a failure here does not fail the upload: the
    // reservation is dropped and later launches grow their buffers lazily.
    if (apply_reserve(d) != RT_OK) {
        (void)hipGetLastError();
        d->reserve_tiles = 0;
        d->reserve_pixels = 0;
    }
    return RT_OK;
}

// Launch buffers for n_tiles block tiles (cost, order, live flags, sort
// scratch, cull counters) and for mask_words cull-mask words.  Growing frees
// buffers earlier launches may still read, so `sync` (the caller's stream, or
// the whole device when NULL) is waited for first; growing clears the tile key.
static int ensure_tile_buffers(rt_device *d, uint32_t n_tiles, hipStream_t sync, bool device_wide) {
    if (n_tiles <= d->tile_cap && d->d_cull_counters) return RT_OK;
    if (device_wide) HIP_OK(hipDeviceSynchronize());
    else HIP_OK(hipStreamSynchronize(sync));
    if (n_tiles > d->tile_cap) {
        for (uint32_t **b : {&d->d_tile_cost, &d->d_tile_order, &d->d_tile_scratch, &d->d_tile_live,
                             &d->d_tile_order_sorted, &d->d_tile_aux}) {
            (void)hipFree(*b);
            *b = nullptr;
        }
        d->tile_cap = 0;
        // cost / order / sort scratch per unit: up to 4 per block tile (wave units)
        if (hipMalloc(&d->d_tile_cost, 4u * n_tiles * 4u) != hipSuccess ||
            hipMalloc(&d->d_tile_order, 4u * n_tiles * 4u) != hipSuccess ||
            hipMalloc(&d->d_tile_order_sorted, 4u * n_tiles * 4u) != hipSuccess ||
            hipMalloc(&d->d_tile_aux, 2u * n_tiles * 4u) != hipSuccess ||
            hipMalloc(&d->d_tile_live, n_tiles * 4u) != hipSuccess ||
            hipMalloc(&d->d_tile_scratch, rtk_tile_sort_scratch(4u * n_tiles)) != hipSuccess)
            return fail(RT_ENOMEM, "rt_trace: tile order buffers");
        d->tile_cap = n_tiles;
        d->last.BufferGrowths += 1;
    }
    if (!d->d_cull_counters && hipMalloc(&d->d_cull_counters, kCullCounterWords * 8u) != hipSuccess)
        return fail(RT_ENOMEM, "rt_trace: tile order buffers");
    d->tile_key.clear();
    return RT_OK;
}

static int ensure_masks(rt_device *d, size_t mask_words, hipStream_t sync, bool device_wide) {
    if (mask_words <= d->mask_cap) return RT_OK;
    if (device_wide) HIP_OK(hipDeviceSynchronize());
    else HIP_OK(hipStreamSynchronize(sync));
    (void)hipFree(d->d_masks);
    d->d_masks = nullptr;
    d->mask_cap = 0;
    if (hipMalloc(&d->d_masks, mask_words * 8u) != hipSuccess) return fail(RT_ENOMEM, "rt_trace: cull masks");
    d->mask_cap = mask_words;
    d->last.BufferGrowths += 1;
    d->tile_key.clear();
    return RT_OK;
}

static int ensure_pixel_sort(rt_device *d, uint32_t n_tiles, size_t pixels, hipStream_t sync, bool device_wide) {
    if ((size_t)n_tiles * 64u <= d->pix_perm_cap && pixels * 4u <= d->pix_cost_cap) return RT_OK;
    if (device_wide) HIP_OK(hipDeviceSynchronize());
    else HIP_OK(hipStreamSynchronize(sync));
    if ((size_t)n_tiles * 64u > d->pix_perm_cap) {
        (void)hipFree(d->d_pix_perm);
        d->d_pix_perm = nullptr;
        d->pix_perm_cap = 0;
        if (hipMalloc(&d->d_pix_perm, (size_t)n_tiles * 64u) != hipSuccess) return fail(RT_ENOMEM, "rt_trace: pixel order");
        d->pix_perm_cap = (size_t)n_tiles * 64u;
    }
    if (pixels * 4u > d->pix_cost_cap) {
        (void)hipFree(d->d_pix_cost);
        d->d_pix_cost = nullptr;
        d->pix_cost_cap = 0;
        if (hipMalloc(&d->d_pix_cost, pixels * 4u) != hipSuccess) return fail(RT_ENOMEM, "rt_trace: pixel costs");
        d->pix_cost_cap = pixels * 4u;
    }
    d->last.BufferGrowths += 1;
    d->tile_key.clear();
    return RT_OK;
}

// The selection buffer for images of up to `ref_tiles` reference tiles: the device copy of the
// bitmap and of rt_trace_tile_work's counts table behind it, and the two pinned slots each of them
// is uploaded from.  Growing waits first, as above (a copy out of a slot is work of that stream
// too), so no slot is in flight afterwards.
static int ensure_sel(rt_device *d, uint32_t ref_tiles, hipStream_t sync, bool device_wide) {
    if (ref_tiles <= d->sel_cap) return RT_OK;
    if (device_wide) HIP_OK(hipDeviceSynchronize());
    else HIP_OK(hipStreamSynchronize(sync));
    (void)hipFree(d->d_sel);
    d->d_sel = nullptr;
    d->sel_cap = 0;
    const size_t slot_words[2] = {rtk_sel_table_at(ref_tiles), 2u * (size_t)ref_tiles};  // bitmap, table
    StagedWords *staged[2] = {&d->sel, &d->counts};
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 2; ++i) {
            StagedWords &w = *staged[k];
            if (w.h[i]) (void)hipHostFree(w.h[i]);
            w.h[i] = nullptr;
            w.in_flight[i] = false;
            if (!w.ev[i] && hipEventCreateWithFlags(&w.ev[i], hipEventDisableTiming) != hipSuccess)
                return fail(RT_ENOMEM, "rt_trace_tiles: upload event");
            if (hipHostMalloc(&w.h[i], slot_words[k] * 4u, hipHostMallocDefault) != hipSuccess)
                return fail(RT_ENOMEM, "rt_trace_tiles: pinned staging");
        }
    if (hipMalloc(&d->d_sel, rtk_sel_buffer_words(ref_tiles) * 4u) != hipSuccess)
        return fail(RT_ENOMEM, "rt_trace_tiles: selection buffer");
    d->sel_cap = ref_tiles;
    d->last.BufferGrowths += 1;
    d->tile_key.clear();
    return RT_OK;
}

// n words -> dst (device) on `s`, through the pinned slot not used last.  The slot's previous copy
// (two uploads ago) has normally finished long since; if not, the host waits for it here -- the
// one place rt_trace_tiles and rt_trace_tile_work may block beyond rt_trace's own.
static int staged_upload(StagedWords &w, uint32_t *dst, const uint32_t *words, size_t n, hipStream_t s) {
    const uint32_t slot = w.slot ^ 1u;
    if (w.in_flight[slot]) HIP_OK(hipEventSynchronize(w.ev[slot]));
    w.in_flight[slot] = false;
    memcpy(w.h[slot], words, n * 4u);
    HIP_OK(hipMemcpyAsync(dst, w.h[slot], n * 4u, hipMemcpyHostToDevice, s));
    HIP_OK(hipEventRecord(w.ev[slot], s));
    w.in_flight[slot] = true;
    w.slot = slot;
    return RT_OK;
}

// The buffers of every launch rt_trace may make at the reserved geometry:
// the most block tiles over every lanes-per-pixel shape (rt_trace picks P per
// launch) and the current scene's mask words, so no later launch allocates.
static int apply_reserve(rt_device *d) {
    if (!d->reserve_tiles) return RT_OK;
    const uint32_t n_tiles = d->reserve_tiles;
    uint32_t n_words = 1;
    if (d->scene_set)
        for (int rs = 0; rs < 2; ++rs) n_words = std::max(n_words, rtk_mask_words(d->n_groups[rs]));
    if (const int rc = ensure_tile_buffers(d, n_tiles, nullptr, true)) return rc;
    if (const int rc = ensure_sel(d, d->reserve_ref_tiles, nullptr, true)) return rc;  // (rt_trace_tiles, rt_trace_tile_work)
    if (d->pixel_sort_env)
        if (const int rc = ensure_pixel_sort(d, n_tiles, d->reserve_pixels, nullptr, true))
            return rc;
    return ensure_masks(d, (size_t)n_tiles * 4u * n_words, nullptr, true);
}

extern "C" int rt_device_reserve(rt_device *d, uint32_t width, uint32_t local_rows) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || width == 0 || local_rows == 0 || width > 65536 || local_rows > 65536)
        return fail(RT_EINVAL, "rt_device_reserve: bad argument");
    HIP_OK(hipSetDevice(d->ordinal));
    uint32_t n_tiles = 0;
    for (const int p : {1, 2, 4, 8, 16, 32}) n_tiles = std::max(n_tiles, rtk_tile_count(width, local_rows, p));
    d->reserve_tiles = std::max(d->reserve_tiles, n_tiles);
    d->reserve_pixels = std::max(d->reserve_pixels, (size_t)width * local_rows);
    // (rt_trace_tiles' bitmap and rt_trace_tile_work's table: the reference tiles of a width x local_rows image)
    d->reserve_ref_tiles = std::max(d->reserve_ref_tiles, rt_tile_count(width, local_rows, nullptr));
    return apply_reserve(d);
}

extern "C" uint32_t rt_tile_count(uint32_t width, uint32_t height, uint32_t *out_tiles_x) {
    const bool ok = width != 0 && height != 0 && width <= 65536 && height <= 65536;
    const uint32_t tx = ok ? (width + RT_TILE_SIZE - 1u) / RT_TILE_SIZE : 0u;
    if (out_tiles_x) *out_tiles_x = tx;
    return ok ? tx * ((height + RT_TILE_SIZE - 1u) / RT_TILE_SIZE) : 0u;
}
static_assert(kRefTile == RT_TILE_SIZE, "the kernels' reference tile is the header's");

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

// A launch's per-tile counts (rt_trace_tile_work with mixed pairs): the table the kernels read
// (TraceArgs.tile_counts_at's layout; {0, 0} for a tile outside the selection, which nothing reads).
struct TileCounts {
    const uint32_t *table = nullptr;
    size_t n_words = 0;  // 2 x the image's reference tiles
};

// Validates a tile list against a width x height image and builds its bitmap into `bits`
// (plain host code: no device, no allocation beyond the vector's growth).  Returns 0, or -1 for an
// index past the image's tiles (*bad = its position in the list), -2 for an index named twice.
static int build_selection(const uint32_t *tiles, uint32_t n_tiles, uint32_t width, uint32_t height,
                           std::vector<uint32_t> &bits, TileSelection &sel, uint32_t *bad) {
    uint32_t tiles_x = 0;
    const uint32_t total = rt_tile_count(width, height, &tiles_x);
    const uint32_t tiles_y = tiles_x ? total / tiles_x : 0u;
    sel = TileSelection();
    sel.tiles_x = tiles_x;
    sel.n_words = (total + 31u) / 32u;
    sel.n_tiles = total;
    sel.clip_w = width - (tiles_x - 1u) * RT_TILE_SIZE;   // the last column's and row's clipped
    sel.clip_h = height - (tiles_y - 1u) * RT_TILE_SIZE;  // size (32 when the image is not ragged)
    bits.assign(sel.n_words, 0u);
    for (uint32_t i = 0; i < n_tiles; ++i) {
        const uint32_t t = tiles[i];
        *bad = i;
        if (t >= total) return -1;
        if ((bits[t >> 5] >> (t & 31u)) & 1u) return -2;
        bits[t >> 5] |= 1u << (t & 31u);
        const bool right = t % tiles_x == tiles_x - 1u && sel.clip_w != RT_TILE_SIZE;
        const bool bottom = t / tiles_x == tiles_y - 1u && sel.clip_h != RT_TILE_SIZE;
        sel.n_class[(right ? 1u : 0u) + (bottom ? 2u : 0u)] += 1u;
        sel.pixels += (uint64_t)(right ? sel.clip_w : RT_TILE_SIZE) * (bottom ? sel.clip_h : RT_TILE_SIZE);
    }
    sel.bits = bits.data();
    return 0;
}

// What rt_trace refuses before it looks at the images (rt_trace_tiles refuses the same).
static int check_trace_args(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, uint64_t *d_rays) {
    if (!d || !cam || !desc || !d_rays) return fail(RT_EINVAL, "rt_trace: NULL argument");
    if (!d->lut_set) return fail(RT_EINVAL, "rt_trace: rsqrt table not set (rt_set_rsqrt_table)");
    if (!d->scene_set) return fail(RT_EINVAL, "rt_trace: no scene uploaded (rt_scene_upload)");
    if (desc->SeedMode != RT_SEED_PIXEL) return fail(RT_EINVAL, "rt_trace: only RT_SEED_PIXEL runs on the GPU");
    if (desc->Flags & ~(RT_FLAG_ACCUM_ZERO | RT_FLAG_SRGB_POW))
        return fail(RT_EINVAL, "rt_trace: unknown Flags 0x%x", desc->Flags);
    if (desc->Width == 0 || desc->Height == 0 || desc->Width > 65536 || desc->Height > 65536)
        return fail(RT_EINVAL, "rt_trace: bad image size %ux%u", desc->Width, desc->Height);
    const uint32_t band_rows = desc->BandRows ? desc->BandRows : 32u;
    const uint32_t band_count = desc->BandCount ? desc->BandCount : 1u;
    if (desc->BandIndex >= band_count) return fail(RT_EINVAL, "rt_trace: BandIndex >= BandCount");
    if (band_rows % 8u) return fail(RT_EINVAL, "rt_trace: BandRows must be a multiple of 8");
    if ((uint64_t)desc->PreviousRayCount + desc->Frames > 0xFFFFFFFFull)
        return fail(RT_EINVAL, "rt_trace: PreviousRayCount + Frames exceeds the u32 frame count");
    return RT_OK;
}

// rt_trace, over every tile of the band (sel == NULL) or over the listed reference tiles of the
// full image (rt_trace_tiles: one band, sel validated against desc's image and not empty).
// counts (rt_trace_tile_work with mixed pairs; needs sel): every listed tile folds its own frames from
// its own count.  desc then carries the LARGEST Frames of the list, by which the launch shape is chosen
// (never more lanes than frames; 4 pixels per lane at one frame), and PreviousRayCount 0; the kernels
// take each tile's pair from the table.  Nothing of the counts enters the key.
// d_delta (rt_trace_tile_work_delta; needs sel): the RGBA8 image is left to the closing pass whatever the
// launch shape, and that pass also writes each listed tile's change statistics.  No part of the key either.
static int trace_launch(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, const TileSelection *sel,
                        const TileCounts *counts, uint64_t *d_rays, void *stream, rt_tile_delta *d_delta = nullptr) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (const int rc = check_trace_args(d, cam, desc, d_rays)) return rc;
    const uint32_t band_rows = desc->BandRows ? desc->BandRows : 32u;
    const uint32_t band_count = desc->BandCount ? desc->BandCount : 1u;
    const uint32_t local_rows = rt_band_local_rows(desc->Height, band_rows, band_count, desc->BandIndex);
    if (desc->Frames == 0 || local_rows == 0) return RT_OK;
    if (!cam->CurrentImage.Data || !cam->PreviousImage.Data)
        return fail(RT_EINVAL, "rt_trace: CurrentImage/PreviousImage device pointers missing");
    const int rs = desc->EnableSIMD ? 0 : 1;
    TraceArgs a;
    memset(&a, 0, sizeof(a));
    a.groups = d->d_groups[rs];
    a.materials = d->d_mats[rs];
    a.rsqrt_lut = d->d_lut;
    a.weights = d->d_weights;
    a.prev = (float4 *)cam->PreviousImage.Data;
    a.cur = (uint32_t *)cam->CurrentImage.Data;
    a.rays = (unsigned long long *)d_rays;
    const rt_v3 *v[4] = {&cam->CameraPosition, &cam->CameraX, &cam->CameraY, &cam->FilmCenter};
    float *dst[4] = {a.cam_pos, a.cam_x, a.cam_y, a.film_center};
    for (int i = 0; i < 4; ++i) {
        dst[i][0] = v[i]->x;
        dst[i][1] = v[i]->y;
        dst[i][2] = v[i]->z;
    }
    a.film_w = cam->FilmW;
    a.film_h = cam->FilmH;
    a.width = desc->Width;
    a.height = desc->Height;
    // f64 division then rounding to f32 is the correctly rounded f32 quotient
    // (53 >= 2*24 + 2: double rounding is innocuous for division)
    a.inv_width = (float)(1.0 / (double)(float)desc->Width);
    a.inv_height = (float)(1.0 / (double)(float)desc->Height);
    // the divisors themselves: the u32 -> f32 conversion (round to nearest even; exact here, sizes are
    // at most 65536) the kernel otherwise repeats for every sample
    a.width_f = (float)desc->Width;
    a.height_f = (float)desc->Height;
    a.local_rows = local_rows;
    a.prev_count = desc->PreviousRayCount;
    a.frames = desc->Frames;
    a.max_bounce = desc->MaxBounce;
    a.n_groups = d->n_groups[rs];
    a.n_spheres = d->n_spheres;
    a.use_sky = d->use_sky ? 1u : 0u;
    a.flags = ((desc->Flags & RT_FLAG_ACCUM_ZERO) ? kFlagAccumZero : 0u) |
              ((desc->Flags & RT_FLAG_SRGB_POW) ? kFlagSrgbPow : 0u);
    a.band_rows = band_rows;
    a.band_count = band_count;
    a.band_index = desc->BandIndex;
    a.prefilter = d->prefilter[rs];
    a.pf_relative = d->pf_relative[rs];
    a.fast_sqrt = d->fast_sqrt[rs];
    if (a.prefilter && d->n_cpairs[rs] &&
        (d->clusters_env == 2 || (d->clusters_env == 1 && d->n_groups[rs] <= kClAutoGroups))) {
        a.clusters = d->d_clusters[rs];
        a.n_cpairs = d->n_cpairs[rs];
        a.cl_words = d->cl_words[rs];
    }
    // Lanes that must wait before a secondary round runs: the dearer a wave's
    // secondary round (cluster pairs, or groups without clusters), the more it
    // pays to fill it first.  Measured (same box, Mrays/s, threshold 16/32/40/48):
    // RTWeekend (20 cluster pairs) 18.6k/19.4k/19.5k/19.5k, C5 at 512 spp (16)
    // 44.7k/46.3k/46.4k/46.4k, C2 (5) 153.8k/151.2k/150.4k/149.9k.  Round 4 (in-pixel
    // sample hand-out, 40/44/48/52): RTWeekend (per-lane thresholds) 25.61k/25.73k/25.74k/
    // 25.71k, C5 (scene-wide) 52.74k/52.44k/52.58k/52.38k: 48 for per-lane walks.
    a.merge_rounds = d->merge_env == 1 || (d->merge_env == -1 && d->n_groups[rs] <= kMergeGroups) ? 1u : 0u;
    // Round 5 (primary table, steady state): 24 for the small walks, against 16 / 32: C2 +1.2 %, C3 +1.0 %, the
    // 4-rank share -2.7 %, the 8-rank share -0.8 % (profiles/r05r_sec_threshold_ab.txt).
    // (never 0 in the kernel, whose round decision compares the count of secondary lanes against it: round_select)
    a.sec_threshold = d->sec_threshold;
    if (a.sec_threshold == 0)
        a.sec_threshold = (a.clusters ? a.n_cpairs : a.n_groups) >= 12u ? (a.pf_relative ? 48u : 40u) : 24u;
    a.stats = d->d_stats;
    HIP_OK(hipSetDevice(d->ordinal));
    hipStream_t s = (hipStream_t)stream;  // NULL = the HIP null stream
    // Lanes per pixel (measured on MI355X at 1/2/4/8-way band splits of C2,
    // bench.py --sim-ranks, heaviest-first order at every P): 4 while the band
    // has >= 6k pixels per CU, 8 down to 3k, else 16 (round 4, with the in-pixel
    // sample hand-out: the 4-rank share 1.19-1.23 ms at P = 16 against 1.25-1.28
    // at P = 8; the 2-rank share 2.26-2.27 at P = 8, 2.29 at P = 16; more lanes per pixel
    // shorten the per-lane sample chains that form the launch tail; C2 rank
    // shares: 1 GPU P=4 6.21 ms (P=8 6.29, P=16 6.62); 2 ranks P=8 3.26 ms
    // (P=4 3.35); 4 ranks P=8 = P=16 1.81 ms; 8 ranks P=16 1.02 ms (P=8
    // 1.47)); never more lanes than frames.
    int lpp = d->lanes_per_pixel;
    const bool auto_lpp = lpp == 0;
    if (lpp == 0) {
        // (a tile list: the pixels it covers -- a small window is a small launch, like a small rank share)
        const uint64_t pixels = sel ? sel->pixels : (uint64_t)desc->Width * local_rows;
        lpp = pixels >= (uint64_t)d->cu_count * 6144u ? 4 : pixels >= (uint64_t)d->cu_count * 3072u ? 8 : 16;
        while (lpp > 1 && (uint32_t)lpp / 2u >= desc->Frames) lpp /= 2;
    }
    // One lane per pixel, and one frame (the reference's OnRender unit): each lane
    // takes kPixelsPerLane pixels in turn (launch shape 0, rtk_shape.h Shape<0>),
    // so a wave stays full after its first pass and the launch has a quarter of
    // the waves.  Measured on the 1080p OnRender frame: see DESIGN.md §6a.
    const uint32_t pixels_per_lane =
        lpp == 1 && !(desc->Flags & RT_FLAG_SRGB_POW) &&
                (d->pixels_per_lane_env == 4 || (d->pixels_per_lane_env == 0 && auto_lpp && desc->Frames == 1))
            ? 4u : 1u;
    const uint32_t lanes = (uint32_t)lpp;  // lanes per pixel (the sample chains of a pixel)
    if (pixels_per_lane > 1) lpp = 0;      // the launch shape code of rtk_* (0: pixels per lane)
    // Tile scheduling.  Block tiles (2TW x 2TH pixels) are traced in the order
    // tile_order[0 .. n_live): with culling, the cull pass (once per camera /
    // scene / geometry) writes every wave tile's primary group mask and a
    // live-first order, and dead tiles (no candidate group anywhere, no sky)
    // never reach the trace kernel -- rtk_launch_empty folds their pixels.
    // With heaviest-first scheduling each launch also measures its tiles and
    // re-sorts them for the next launch (live tiles keep costs > 0, dead ones
    // 0, so the live prefix is preserved).
    if (d->want_wave_times) {  // one {start, end} per wave of this launch's tile shape
        const size_t waves = (size_t)rtk_tile_count(desc->Width, local_rows, lpp) * 4u;
        if (waves > d->wave_times_cap) {
            (void)hipFree(d->d_wave_times);
            d->d_wave_times = nullptr;
            if (hipMalloc(&d->d_wave_times, waves * 16u) != hipSuccess) return fail(RT_ENOMEM, "wave_times");
            d->wave_times_cap = waves;
        }
        a.wave_times = d->d_wave_times;
    }
    a.interleave = d->interleave_env && lpp >= 2 ? 1u : 0u;
    // The rsqrt and fold tables (10 KB) leave the LDS image at P = 16, whose 4-wave
    // ring (10 KB) would otherwise cap a CU at 6 blocks: measured on the 8-rank C2
    // share 0.900-0.903 against 0.914-0.922 ms; at P = 4 they stay (C2 -1.8 % without)
    const bool tables = !d->tables_global_env && lpp <= 8;
    a.lut_in_lds = rtk_lut_in_lds(a.n_groups) && tables ? 1u : 0u;
    a.fold_in_lds = rtk_fold_in_lds(a.n_groups) && tables ? 1u : 0u;
    a.scene_in_lds = a.n_groups <= kMaxLdsGroups && !d->scene_global_env ? 1u : 0u;
    if (d->solo_env && d->src == kSrcSmem) {  // one-wave workgroups keep no LDS image
        a.solo = 1u;
        a.lut_in_lds = a.fold_in_lds = a.scene_in_lds = 0u;
        // the walk-specialised kernel this launch asks for, or the run-time one (rt_kernel.h, the routing
        // rule: a.clusters is set only with n_cpairs >= 1, above, and Frames == 0 returned above)
        a.walk = rtk_walk_request(a, d->walk_any_env != 0);
        // The expanded table goes to the kernels that hold the expanded prefilter, and to no other (rt_kernel.h
        // kPrefilterExpanded): offered here, and taken back unless this launch's kernel is one of them.
        if (a.clusters && !a.pf_relative && d->clusters_x_ok[rs] && !d->walk_any_env) {
            const float4 *plain = a.clusters;
            a.clusters = d->d_clusters_x[rs];  // (the row {c0, 0}, then entry 0)
            a.prefilter = kPrefilterExpanded;
            a.walk = rtk_walk_request(a, false);
            if (!rtk_walk_expanded(a, d->cull != 0, lpp)) {
                // (a shape or a device without walk kernels: the request stands, as it always did for such a
                // launch, and rtk_walk_kernel gives it the run-time kernel, now for want of the expanded table too)
                a.clusters = plain;
                a.prefilter = kPrefilterOn;
            }
        }
    }
    const int src = a.scene_in_lds ? d->src : kSrcSmem;  // a scene in HBM is read through the scalar cache
    if (counts && !a.solo && !rtk_tile_counts_four_wave(a.scene_in_lds, src)) {
        // a four-wave launch whose kernel is not built with per-tile counts (SphereSourceLds, SceneInHbm,
        // a scene beyond the LDS image): the one-wave run-time kernel, reported as such (rt_trace_info)
        a.solo = 1u;
        a.lut_in_lds = a.fold_in_lds = a.scene_in_lds = 0u;
        a.walk = kWalkAny;
    }
    const uint32_t n_tiles = rtk_tile_count(desc->Width, local_rows, lpp);
    // Units of the heaviest-first order: waves for the one-wave kernels (each wave
    // its own workgroup, so each is placed by its own cost), block tiles otherwise
    a.unit_waves = a.solo && d->wave_order_env ? 1u : 0u;
    const uint32_t n_units = a.unit_waves ? 4u * n_tiles : n_tiles;
    const uint32_t n_words = rtk_mask_words(a.n_groups);
    const bool cull = d->cull != 0;
    const bool empty_capable = cull && !d->use_sky && desc->MaxBounce != 0;
    const bool sched = d->tile_sched != 0;
    a.tiles_x = rtk_tiles_x(desc->Width, lpp);
    std::vector<uint32_t> key = {desc->Width, desc->Height, local_rows, band_rows, band_count, desc->BandIndex,
                                 (uint32_t)lpp, (uint32_t)rs, (uint32_t)cull, (uint32_t)empty_capable, (uint32_t)sched,
                                 a.interleave, a.unit_waves,
                                 (uint32_t)d->scene_gen, (uint32_t)(d->scene_gen >> 32)};
    for (const float *f : {a.cam_pos, a.cam_x, a.cam_y, a.film_center}) {
        for (int i = 0; i < 3; ++i) {
            uint32_t u;
            memcpy(&u, f + i, 4);
            key.push_back(u);
        }
    }
    for (const float f : {a.film_w, a.film_h}) {
        uint32_t u;
        memcpy(&u, &f, 4);
        key.push_back(u);
    }
    // the selection is part of the key, word for word (never a hash: a collision would reuse another
    // list's masks and order); 64 words at 1080p, 131,072 at the 65536^2 limit
    key.push_back(sel ? 1u : 0u);
    if (sel) key.insert(key.end(), sel->bits, sel->bits + sel->n_words);
    // block tiles inside the listed tiles (every tile's without a list)
    const uint32_t n_selected = sel ? sel->block_tiles(lpp) : n_tiles;
    if (!d->tile_stream_set || s != d->tile_stream) {
        // order, masks and costs are written and read in stream order: on a new
        // stream, every launch issued on the previous one must have finished (the
        // previous stream may be gone, so the wait is for the device; switching
        // streams is rare -- every caller here keeps one per device)
        if (d->tile_stream_set) HIP_OK(hipDeviceSynchronize());
        d->tile_stream = s;
        d->tile_stream_set = true;
    }
    // (no allocation here once rt_device_reserve has sized the buffers for this geometry)
    if (const int rc = ensure_tile_buffers(d, n_tiles, s, false)) return rc;
    const size_t mask_words = (size_t)n_tiles * 4u * n_words;
    if (cull)
        if (const int rc = ensure_masks(d, mask_words, s, false)) return rc;
    // pixels dealt to waves by cost (options PixelSort): block tiles of at most 64 pixels
    const bool pixel_sort = d->pixel_sort_env && sched && lpp >= 4 && !a.interleave;
    if (pixel_sort)
        if (const int rc = ensure_pixel_sort(d, n_tiles, (size_t)desc->Width * local_rows, s, false)) return rc;
    if (sel)
        if (const int rc = ensure_sel(d, sel->n_tiles, s, false)) return rc;
    const bool new_key = key != d->tile_key;
    // the key's bitmap on the device (uploaded below when the key is new; the same list again finds it there)
    a.sel = sel ? d->d_sel : nullptr;
    a.sel_tiles_x = sel ? sel->tiles_x : 0u;
    // (the table is written by the key's cull pass: the key holds the camera and the scene)
    a.prim = cull ? d->d_prim[rs] : nullptr;
    uint32_t head_frames = 0;  // > 0: split this launch (first launch of a key, below): frames of the leading parts
    uint32_t split[8], n_split = 0;
    if (new_key) {
        // (first, so that a failed upload leaves no key behind that claims its bitmap is on the device)
        d->tile_key.clear();
        if (sel)
            if (const int rc = staged_upload(d->sel, d->d_sel, sel->bits, sel->n_words, s)) return rc;
        d->tile_key = key;
        d->n_sorts = 0;
        if (pixel_sort) HIP_OK(hipMemsetAsync(d->d_pix_perm, 0xFF, (size_t)n_tiles * 64u, s));  // identity
        if (cull) {
            a.masks = d->d_masks;
            d->mask_words = mask_words;
            if (rtk_launch_cull(&a, lpp, d->d_tile_live, d->d_tile_cost, d->d_cull_counters, empty_capable ? 1 : 0, s) !=
                    0 ||
                rtk_launch_tile_sort(d->d_tile_cost, d->d_tile_order, d->d_tile_scratch, n_units, s) != 0)
                return fail(RT_EIO, "rt_trace: cull pass launch failed: %s", hipGetErrorString(hipGetLastError()));
            // the totals follow asynchronously (resolve_counts); no host wait here
            HIP_OK(hipMemcpyAsync(d->h_counts, d->d_cull_counters + kCullTotals, 2 * sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, s));
            HIP_OK(hipEventRecord(d->ev_counts, s));
            d->counts_known = false;
            d->tile_order_valid = true;
            // The first launch of a key has no measured tile costs, and in the cull
            // pass's live-first order its heavy tiles start late and form the tail
            // (C2 cold 7.7 ms against 5.4 warm).  A long launch is therefore split:
            // its first head_samples samples per lane (1/8 of C2's work) run in that
            // order and measure the tile costs, and the remaining frames continue the
            // running mean heaviest-first.  Splitting a launch at a frame boundary
            // changes no bit: the owner lane folds frames in order either way, and
            // frame k's seed and weights depend on PreviousRayCount + k only.
            const uint32_t split_min = 4u * d->head_samples * lanes;
            // (not with per-tile counts: a split would need a head per tile)
            if (sched && d->split_env && !counts && desc->Frames >= split_min) {
                // leading parts of head_samples, x split_growth, ... samples per lane
                // while the rest keeps at least half the frames
                uint32_t f = d->head_samples * lanes, used = 0;
                // (f != 0: an extreme SplitGrowth wraps the product; no part of a launch is empty)
                for (uint32_t i = 0; i + 1 < d->split_parts && f != 0 && used + f <= desc->Frames / 2u; ++i) {
                    split[n_split++] = f;
                    used += f;
                    f *= d->split_growth;
                }
                head_frames = used;
            }
        } else {
            HIP_OK(hipMemsetAsync(d->d_tile_cost, 0, n_units * 4u, s));
            // no cull pass: every block tile is live, and the totals word the XCD grouping reads
            // (rtk_launch_xcd_group) says so (u64 little-endian: low word n_tiles, the rest 0)
            HIP_OK(hipMemsetAsync(d->d_cull_counters + kCullTotals, 0, 2 * sizeof(unsigned long long), s));
            HIP_OK(hipMemsetD32Async((hipDeviceptr_t)(d->d_cull_counters + kCullTotals), n_selected, 1, s));
            d->n_live = n_selected;
            d->dead_pixels = 0;
            d->counts_known = true;
            d->tile_order_valid = false;  // identity until a measured sort exists
            if (sel) {
                // a tile list: the identity order would trace unlisted tiles, so the selected
                // tiles (cost 2, the others 0) are sorted to the front and the grid is their count
                if (rtk_launch_select(&a, lpp, d->d_tile_live, d->d_tile_cost, s) != 0 ||
                    rtk_launch_tile_sort(d->d_tile_cost, d->d_tile_order, d->d_tile_scratch, n_units, s) != 0)
                    return fail(RT_EIO, "rt_trace_tiles: select pass launch failed: %s",
                                hipGetErrorString(hipGetLastError()));
                d->tile_order_valid = true;
            }
        }
    }
    // live-tile count: on the host once the cull totals have landed, else read
    // by the kernels from the device (grid over every tile, early exit)
    const bool known = resolve_counts(d, false);
    const uint32_t grid_tiles = known ? d->n_live : n_tiles;
    a.live_total = known ? nullptr : d->d_cull_counters + kCullTotals;
    const bool any_live = !known || d->n_live > 0;
    const bool any_dead = empty_capable && (!known || d->n_live < n_selected);
    a.masks = cull ? d->d_masks : nullptr;
    a.tile_order = d->tile_order_valid ? d->d_tile_order : nullptr;
    if (counts) {  // this call's table, whatever the key: the counts are no part of it
        a.tile_counts_at = rtk_sel_table_at(sel->n_tiles);
        if (const int rc = staged_upload(d->counts, d->d_sel + a.tile_counts_at, counts->table, counts->n_words, s)) return rc;
    }
    // (the identity order knows no selection: both paths above leave a sorted order for a tile list)
    if (sel && !a.tile_order) return fail(RT_EIO, "rt_trace_tiles: no tile order for the selection");
    a.tile_cost = sched ? d->d_tile_cost : nullptr;
    a.pix_perm = pixel_sort ? d->d_pix_perm : nullptr;
    a.pix_seg = d->pixel_seg;
    // (multi-frame launches only: a one-frame launch, OnRender's, keeps its store and one kernel fewer)
    // (the statistics need the old bytes: no kernel before the closing pass may store RGBA8, at any shape)
    a.skip_cur = (d->cur_pass && lpp >= 2) || d_delta ? 1u : 0u;
    d->last.PixelsSorted = pixel_sort && !new_key && d->n_sorts > 0 ? 1u : 0u;
    d->last_n_tiles = n_selected;  // (SegmentsFolded: the dead tiles among these)
    d->last.TilesSelected = n_selected;
    d->last_frames = desc->Frames;
    d->last_empty_capable = empty_capable;
    d->last.LanesPerPixel = lanes;
    d->last.PixelsPerLane = pixels_per_lane;
    d->last.TilesTotal = n_tiles;
    d->last.CullPassRan = cull && new_key ? 1u : 0u;
    d->last.OrderedLaunches = d->n_sorts;
    d->last.ClusteredWalk = a.clusters ? 1u : 0u;
    d->last.GroupsPerRuleSet = a.n_groups;
    d->last.OneWaveGroups = a.solo;
    d->last.Walk = a.walk;
    d->last_tile_counts = counts != nullptr;
    d->last_folded_on_device = false;
    // one launch, or the split of a key's first launch (above): the leading
    // parts, then the rest, each continuing the running mean heaviest-first
    split[n_split++] = desc->Frames - head_frames;
    uint32_t done_frames = 0;
    for (uint32_t part = 0; part < n_split; ++part) {
        if (part > 0) {
            a.prev_count = desc->PreviousRayCount + done_frames;
            a.flags &= ~kFlagAccumZero;
            a.tile_order = d->d_tile_order;
        }
        a.frames = split[part];
        done_frames += split[part];
        const bool resort = sched && any_live && (d->n_sorts < d->order_launches || part + 1 < n_split);
        a.pix_cost = pixel_sort && resort ? d->d_pix_cost : nullptr;
        // wave costs only for a launch whose costs are sorted: once the order is kept, the
        // per-wave 4-B cost stores (scattered partial lines, ~8 MB of HBM writes per 1080p
        // launch at P = 4) would feed nothing
        a.tile_cost = resort ? d->d_tile_cost : nullptr;
        if (rtk_launch_trace_grid(&a, desc->EnableSIMD ? 1 : 0, src, cull ? 1 : 0, lpp, grid_tiles, s) != 0)
            return fail(RT_EIO, "rt_trace: kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        if (any_dead && counts) {
            // each dead tile folds by its own pair, and the device sums the segments (they are no longer
            // dead pixels x frames); the sum follows to the host asynchronously, as the cull totals do
            unsigned long long *folded = d->d_cull_counters + kCullFolded;
            HIP_OK(hipMemsetAsync(folded, 0, sizeof(unsigned long long), s));
            if (rtk_launch_empty_counts(&a, lpp, d->d_tile_live, folded, s) != 0)
                return fail(RT_EIO, "rt_trace_tile_work: empty-tile launch failed: %s", hipGetErrorString(hipGetLastError()));
            HIP_OK(hipMemcpyAsync(d->h_folded, folded, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            HIP_OK(hipEventRecord(d->ev_folded, s));
            d->last_folded_on_device = true;
        } else if (any_dead && rtk_launch_empty(&a, lpp, d->d_tile_live, d->d_cull_counters + kCullTotals + 1, s) != 0)
            return fail(RT_EIO, "rt_trace: empty-tile launch failed: %s", hipGetErrorString(hipGetLastError()));
        // the learned order settles within a few launches (C2: 7.7, 6.3, 6.1, 5.9,
        // 5.8 ms); after order_launches re-sorts (RT_ORDER_LAUNCHES, default 4)
        // the order is kept and the three sort kernels (~14 us per launch, 1.5 %
        // of an 8-rank C2 share) are skipped
        if (resort) {
            d->n_sorts += 1;
            // one-wave kernels: sort, then group each block tile's waves onto one XCD
            const bool group = a.unit_waves && (d->xcd_group_env == 1 || (d->xcd_group_env < 0 && lpp <= 4));
            if (rtk_launch_tile_sort(d->d_tile_cost, group ? d->d_tile_order_sorted : d->d_tile_order,
                                     d->d_tile_scratch, n_units, s) != 0 ||
                (group && rtk_launch_xcd_group(d->d_tile_order_sorted, d->d_tile_order, n_units,
                                               d->d_cull_counters + kCullTotals, d->d_tile_scratch, d->d_tile_aux,
                                               s) != 0))
                return fail(RT_EIO, "rt_trace: tile sort launch failed: %s", hipGetErrorString(hipGetLastError()));
            if (pixel_sort && rtk_launch_pixel_sort(&a, lpp, d->d_pix_perm, s) != 0)
                return fail(RT_EIO, "rt_trace: pixel sort launch failed: %s", hipGetErrorString(hipGetLastError()));
            d->tile_order_valid = true;
        }
    }
    // options EncodePass: the RGBA8 band image from the running mean the kernels stored (main.cpp:490's
    // store on its own, the same bits), written by one coalesced pass
    // (a tile list: over the listed tiles' pixels only, so no other RGBA8 pixel is written)
    // (rt_trace_tile_work_delta: the same pass, one block per listed tile, with the tile's statistics)
    if (a.skip_cur && desc->Frames > 0 &&
        (d_delta ? rtk_launch_tile_delta_encode(&a, d_delta, s)
         : sel   ? rtk_launch_encode_selected(&a, s)
                 : rtk_launch_encode(a.prev, a.cur, (uint64_t)local_rows * desc->Width,
                                     (a.flags & kFlagSrgbPow) ? 1u : 0u, s)) != 0)
        return fail(RT_EIO, "rt_trace: RGBA8 encode launch failed: %s", hipGetErrorString(hipGetLastError()));
    d->last.SplitHeadFrames = head_frames;
    return RT_OK;
}

extern "C" int rt_trace(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, uint64_t *d_rays,
                        void *stream) {
    return trace_launch(d, cam, desc, nullptr, nullptr, d_rays, stream);
}

extern "C" int rt_trace_tiles(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, const uint32_t *tiles,
                              uint32_t n_tiles, uint64_t *d_rays, void *stream) {
    if (const int rc = check_trace_args(d, cam, desc, d_rays)) return rc;
    if (desc->BandCount > 1u || desc->BandIndex != 0u)
        return fail(RT_EINVAL, "rt_trace_tiles: tiles index the whole image (BandCount 0 or 1, BandIndex 0)");
    if (!tiles && n_tiles) return fail(RT_EINVAL, "rt_trace_tiles: tiles is NULL with n_tiles %u", n_tiles);
    // the list is consumed here: the bitmap lives in the device's own host vector, and a new key's
    // upload goes through the library's pinned slots, so the caller's array is free on return
    TileSelection sel;
    uint32_t bad = 0;
    const int v = build_selection(tiles, n_tiles, desc->Width, desc->Height, d->sel_bits, sel, &bad);
    if (v == -1)
        return fail(RT_EINVAL, "rt_trace_tiles: tiles[%u] = %u, the image has %u tiles", bad, tiles[bad],
                    rt_tile_count(desc->Width, desc->Height, nullptr));
    if (v == -2) return fail(RT_EINVAL, "rt_trace_tiles: tiles[%u] = %u is listed twice", bad, tiles[bad]);
    if (n_tiles == 0 || desc->Frames == 0) return RT_OK;
    return trace_launch(d, cam, desc, &sel, nullptr, d_rays, stream);
}

// rt_trace_tile_work and rt_trace_tile_work_delta (want_delta: d_delta is required and receives the listed
// tiles' change statistics from the closing RGBA8 pass).
static int trace_tile_work(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, const rt_tile_work *work,
                           uint32_t n_work, bool want_delta, rt_tile_delta *d_delta, uint64_t *d_rays, void *stream) {
    if (!desc) return fail(RT_EINVAL, "rt_trace: NULL argument");
    if (want_delta && (!d_delta || ((uintptr_t)d_delta & 15u)))
        return fail(RT_EINVAL, "rt_trace_tile_work_delta: d_delta is %s", d_delta ? "not 16-byte aligned" : "NULL");
    rt_trace_desc dd = *desc;  // (desc's own PreviousRayCount / Frames are not read: every entry has its pair)
    dd.PreviousRayCount = 0;
    dd.Frames = 0;
    if (const int rc = check_trace_args(d, cam, &dd, d_rays)) return rc;
    if (desc->BandCount > 1u || desc->BandIndex != 0u)
        return fail(RT_EINVAL, "rt_trace_tile_work: tiles index the whole image (BandCount 0 or 1, BandIndex 0)");
    if (!work && n_work) return fail(RT_EINVAL, "rt_trace_tile_work: work is NULL with n_work %u", n_work);
    // every entry's tile first, those of zero-frame entries included: a tile named twice is refused
    // before such entries are dropped.  The list is consumed here (the device's own host vectors; the
    // uploads go through the library's pinned slots), so the caller's array is free on return.
    TileSelection sel;
    uint32_t bad = 0;
    d->work_tiles.resize(n_work);
    for (uint32_t i = 0; i < n_work; ++i) d->work_tiles[i] = work[i].Tile;
    const int v = build_selection(d->work_tiles.data(), n_work, desc->Width, desc->Height, d->sel_bits, sel, &bad);
    if (v == -1)
        return fail(RT_EINVAL, "rt_trace_tile_work: work[%u].Tile = %u, the image has %u tiles", bad, work[bad].Tile,
                    rt_tile_count(desc->Width, desc->Height, nullptr));
    if (v == -2) return fail(RT_EINVAL, "rt_trace_tile_work: work[%u].Tile = %u is listed twice", bad, work[bad].Tile);
    for (uint32_t i = 0; i < n_work; ++i)
        if ((uint64_t)work[i].PreviousRayCount + work[i].Frames > 0xFFFFFFFFull)
            return fail(RT_EINVAL, "rt_trace_tile_work: work[%u]: PreviousRayCount + Frames exceeds the u32 frame count", i);
    // the kept entries (Frames > 0): their tiles, their table, whether they share one pair
    const uint32_t total = rt_tile_count(desc->Width, desc->Height, nullptr);
    d->counts_table.assign(2u * (size_t)total, 0u);
    uint32_t kept = 0, max_frames = 0;
    bool uniform = true;
    const rt_tile_work *first = nullptr;
    for (uint32_t i = 0; i < n_work; ++i) {
        const rt_tile_work &e = work[i];
        if (e.Frames == 0u) continue;
        if (!first) first = &e;
        uniform = uniform && e.PreviousRayCount == first->PreviousRayCount && e.Frames == first->Frames;
        max_frames = std::max(max_frames, e.Frames);
        d->counts_table[2u * (size_t)e.Tile] = e.PreviousRayCount;
        d->counts_table[2u * (size_t)e.Tile + 1u] = e.Frames;
        d->work_tiles[kept++] = e.Tile;
    }
    if (kept == 0) return RT_OK;
    (void)build_selection(d->work_tiles.data(), kept, desc->Width, desc->Height, d->sel_bits, sel, &bad);
    if (uniform) {  // one pair: rt_trace_tiles with it -- the same path, kernels and first-launch split
        dd.PreviousRayCount = first->PreviousRayCount;
        dd.Frames = first->Frames;
        return trace_launch(d, cam, &dd, &sel, nullptr, d_rays, stream, d_delta);
    }
    dd.Frames = max_frames;  // (the launch shape's frames; PreviousRayCount stays 0: every tile has its own)
    TileCounts counts;
    counts.table = d->counts_table.data();
    counts.n_words = d->counts_table.size();
    return trace_launch(d, cam, &dd, &sel, &counts, d_rays, stream, d_delta);
}

extern "C" int rt_trace_tile_work(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc,
                                  const rt_tile_work *work, uint32_t n_work, uint64_t *d_rays, void *stream) {
    return trace_tile_work(d, cam, desc, work, n_work, false, nullptr, d_rays, stream);
}

extern "C" int rt_trace_tile_work_delta(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc,
                                        const rt_tile_work *work, uint32_t n_work, rt_tile_delta *d_delta,
                                        uint64_t *d_rays, void *stream) {
    return trace_tile_work(d, cam, desc, work, n_work, true, d_delta, d_rays, stream);
}

extern "C" int rt_assemble_bands(const void *d_compact, uint64_t rank_stride_bytes, void *d_dst, uint32_t width,
                                 uint32_t height, uint32_t elem_bytes, uint32_t band_rows, uint32_t band_count,
                                 void *stream) {
    if (!d_compact || !d_dst || width == 0 || height == 0 || elem_bytes == 0 || band_rows == 0 || band_count == 0)
        return fail(RT_EINVAL, "rt_assemble_bands: bad argument");
    for (uint32_t r = 0; r < band_count; ++r)
        if ((uint64_t)rt_band_local_rows(height, band_rows, band_count, r) * width * elem_bytes > rank_stride_bytes)
            return fail(RT_EINVAL, "rt_assemble_bands: rank stride too small for rank %u", r);
    if (rtk_launch_assemble(d_compact, rank_stride_bytes, d_dst, width, height, elem_bytes, band_rows, band_count,
                            (hipStream_t)stream) != 0)
        return fail(RT_EIO, "rt_assemble_bands: launch failed");
    return RT_OK;
}

extern "C" int rt_encode_rgba8(const float *d_accum_v4, uint32_t *d_rgba8, uint64_t n_pixels, uint32_t flags,
                               void *stream) {
    if ((!d_accum_v4 || !d_rgba8) && n_pixels) return fail(RT_EINVAL, "rt_encode_rgba8: NULL buffer");
    if (flags & ~RT_FLAG_SRGB_POW) return fail(RT_EINVAL, "rt_encode_rgba8: unknown flags 0x%x", flags);
    if (rtk_launch_encode(d_accum_v4, d_rgba8, n_pixels, (flags & RT_FLAG_SRGB_POW) ? 1u : 0u, (hipStream_t)stream) != 0)
        return fail(RT_EIO, "rt_encode_rgba8: launch failed");
    return RT_OK;
}

extern "C" int rt_tile_delta_rgba8(const uint32_t *d_old, const uint32_t *d_new, uint32_t width, uint32_t height,
                                   rt_tile_delta *d_delta, void *stream) {
    if (!d_old || !d_new || !d_delta) return fail(RT_EINVAL, "rt_tile_delta_rgba8: NULL buffer");
    if ((uintptr_t)d_delta & 15u) return fail(RT_EINVAL, "rt_tile_delta_rgba8: d_delta is not 16-byte aligned");
    if (rt_tile_count(width, height, nullptr) == 0u)
        return fail(RT_EINVAL, "rt_tile_delta_rgba8: bad image size %ux%u", width, height);
    if (rtk_launch_tile_delta(d_old, d_new, width, height, d_delta, (hipStream_t)stream) != 0)
        return fail(RT_EIO, "rt_tile_delta_rgba8: launch failed");
    return RT_OK;
}

extern "C" int rt_trace_last_info(rt_device *d, rt_trace_info *out) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !out) return fail(RT_EINVAL, "rt_trace_last_info: NULL argument");
    // the live/dead totals of the last launch's key: waits for them if they
    // are still on their way from the device (the only blocking part)
    HIP_OK(hipSetDevice(d->ordinal));
    if (!resolve_counts(d, true)) return fail(RT_EIO, "rt_trace_last_info: cull totals: %s",
                                              hipGetErrorString(hipGetLastError()));
    d->last.TilesTraced = d->n_live;
    d->last.SegmentsFolded = d->last_empty_capable && d->n_live < d->last_n_tiles
                                 ? d->dead_pixels * d->last_frames : 0u;
    if (d->last_folded_on_device) {  // per-tile counts: the device's own sum (waits for it, as above)
        HIP_OK(hipEventSynchronize(d->ev_folded));
        d->last.SegmentsFolded = *d->h_folded;
    }
    *out = d->last;
    return RT_OK;
}

extern "C" int rt_trace_last_tile_counts(rt_device *d, uint32_t *out) {
    if (!d || !out) return fail(RT_EINVAL, "rt_trace_last_tile_counts: NULL argument");
    *out = d->last_tile_counts ? 1u : 0u;
    return RT_OK;
}

extern "C" int rt_device_synchronize(rt_device *d) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d) return fail(RT_EINVAL, "rt_device_synchronize: NULL device");
    HIP_OK(hipSetDevice(d->ordinal));
    return quiesce(d);
}

extern "C" int rt_debug_stats(rt_device *d, uint64_t out[32], int reset) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !out) return fail(RT_EINVAL, "rt_debug_stats: NULL argument");
    memset(out, 0, 32 * sizeof(uint64_t));
    if (!d->d_stats) return 0;
    HIP_OK(hipSetDevice(d->ordinal));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, d->d_stats, kStatSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) HIP_OK(hipMemset(d->d_stats, 0, kStatSlots * sizeof(unsigned long long)));
    return 1;
}

extern "C" int64_t rt_debug_masks(rt_device *d, uint64_t *out, uint64_t max_words) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !out) return fail(RT_EINVAL, "rt_debug_masks: NULL argument");
    if (!d->d_masks || d->tile_key.empty() || !d->mask_words) return 0;
    const uint64_t n = max_words < d->mask_words ? max_words : d->mask_words;
    HIP_OK(hipSetDevice(d->ordinal));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, d->d_masks, n * 8u, hipMemcpyDeviceToHost));
    return (int64_t)n;
}

extern "C" int64_t rt_debug_wave_times(rt_device *d, uint64_t *out, uint64_t max_waves) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !out) return fail(RT_EINVAL, "rt_debug_wave_times: NULL argument");
    if (!d->d_wave_times) return 0;
    const uint64_t n = max_waves < d->wave_times_cap ? max_waves : d->wave_times_cap;
    HIP_OK(hipSetDevice(d->ordinal));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, d->d_wave_times, n * 16u, hipMemcpyDeviceToHost));
    return (int64_t)n;
}
