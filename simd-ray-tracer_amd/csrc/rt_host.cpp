// rt_host.cpp — C-ABI host side: device context, scene upload, trace launch,
// band assembly.  Plain HIP runtime; no torch types cross this boundary.  What a launch decides
// without a device is rt_plan.cpp's; this file carries the plan out.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "rt_kernel.h"
#include "rt_pack.h"
#include "rt_plan.h"
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

// One rule set of the uploaded scene on the device (what the launch code knows of it: rt_plan.h SceneFacts).
struct SceneBuffers {
    float4 *groups = nullptr, *mats = nullptr;
    float4 *prim = nullptr;  // the primary rounds' camera-relative group rows (TraceArgs.prim), written by the cull pass
    size_t cap_groups = 0;
    float4 *clusters = nullptr;    // clustered prefilter table (rt_pack.cpp cluster_table)
    float4 *clusters_x = nullptr;  // the expanded table, {c0, 0} then the entries (rt_pack.cpp expand_table)
    size_t cap_clusters = 0, cap_clusters_x = 0;  // float4 capacities
};

// The launch buffers of the current geometry and the key they were filled for.
struct TileState {
    uint32_t *cost = nullptr, *order = nullptr, *scratch = nullptr, *live = nullptr;
    uint32_t *order_sorted = nullptr;  // the sort's output before XCD grouping (rtk_launch_xcd_group)
    uint32_t *aux = nullptr;           // XCD grouping: per block tile, first sorted position and group
    size_t cap = 0;                    // block tiles the six above are sized for
    unsigned long long *cull_counters = nullptr;  // kCullCounterWords: striped counters + device totals of the cull pass
    uint64_t *masks = nullptr;  // cull pass output: per wave tile primary group masks
    size_t mask_cap = 0;
    size_t mask_words = 0;      // words the last cull pass wrote (rt_debug_masks)
    uint8_t *pix_perm = nullptr;   // 64 B per block tile (TraceArgs.pix_perm)
    uint32_t *pix_cost = nullptr;  // per band pixel (TraceArgs.pix_cost)
    size_t pix_perm_cap = 0, pix_cost_cap = 0;
    // rt_device_reserve: the most block tiles (over every lanes-per-pixel shape), band pixels and
    // reference tiles of any geometry reserved so far (0: none)
    uint32_t reserve_tiles = 0, reserve_ref_tiles = 0;
    size_t reserve_pixels = 0;
    // the launch (camera, scene, geometry) the masks / live list / order were made for, and the
    // key of the launch being planned (plan_launch fills it: no vector is allocated per launch)
    std::vector<uint32_t> key, next_key;
    bool order_valid = false;
    uint32_t n_sorts = 0;  // re-sorts done for the current key
    // the last stream rt_trace ran on (a switch waits for the device: switch_stream)
    hipStream_t stream = nullptr;
    bool stream_set = false;
};

// rt_trace_tiles: the selection bitmap of the current tile key on the device (TraceArgs.sel; its
// words are part of the key, so keys compare by the lists' content).  A new key's bitmap is
// uploaded from one of two pinned slots (StagedWords).
// rt_trace_tile_work: the per-tile {PreviousRayCount, Frames} table of a launch with mixed counts
// (TraceArgs.tile_counts_at: two words per reference tile of the image) lies behind the bitmap in
// d_sel (rt_kernel.h rtk_sel_table_at) and is uploaded on EVERY such call -- the counts are no part
// of the key -- through two pinned slots of its own, by the same scheme
// rt_trace_tile_counts: that table is written by a pass on the launch's stream from the caller's device table (no
// staging), and behind it lies the bitmap of the listed tiles that fold a frame (rtk_sel_active_at), for the closing pass
struct SelectionStaging {
    uint32_t *d_sel = nullptr;
    StagedWords bits, counts;
    size_t cap = 0;                  // reference tiles d_sel and the pinned slots are sized for
    std::vector<uint32_t> tile_bits;  // rt_trace_tiles builds the call's bitmap here (no allocation per call)
    TileWorkList work;               // rt_trace_tile_work's list, bitmap and table (no allocation per call)
};

// rt_trace_first_hit: the bitmap of the call's tile list on the device and the two pinned slots it is
// uploaded from (StagedWords).  The pass's own: the key's selection buffer above, which a later
// rt_trace_tiles of the same list expects to find as it left it, is never touched.
struct FirstHitStaging {
    uint32_t *d_sel = nullptr;
    StagedWords bits;
    size_t cap = 0;                   // reference tiles d_sel and the pinned slots are sized for
    std::vector<uint32_t> tile_bits;  // the call's bitmap is built here (no allocation per call)
};

// The cull pass's totals travel to the host asynchronously (pinned h_counts,
// event ev_counts): a new key never blocks the host.  Until they have
// landed (known), launches size their grids for every tile and read
// the live count on the device (TraceArgs.live_total).
// A per-tile-counts launch's folded segments are summed on the device (cull_counters[kCullFolded]) and
// follow to the host the same way: pinned h_folded, event ev_folded
struct AsyncTotals {
    uint32_t n_live = 0;
    uint64_t dead_pixels = 0;
    bool known = true;
    unsigned long long *h_counts = nullptr;  // pinned {live tiles, dead pixels}
    hipEvent_t ev_counts = nullptr;
    unsigned long long *h_folded = nullptr;
    hipEvent_t ev_folded = nullptr;
};

// What the last rt_trace launched (rt_trace_last_info), and what that call resolves lazily (the
// folded segments need the totals).
struct LastLaunch {
    rt_trace_info info{};
    uint32_t n_tiles = 0, frames = 0;
    bool empty_capable = false;
    bool folded_on_device = false;  // SegmentsFolded is h_folded's
    bool tile_counts = false;       // the launch took per-tile counts (rt_trace_last_tile_counts)
    bool dir_table = false;         // its kernel is the direction walk's (rt_trace_last_direction_table)
};

struct rt_device {
    int ordinal = 0;
    hipStream_t stream = nullptr;
    uint32_t cu_count = 256;
    rt_device_options opt{};  // as created (rt_device_get_options)
    Switches sw;
    float *d_lut = nullptr;  // 2048 f32
    bool lut_set = false;
    float2 *d_weights = nullptr;  // TraceArgs.weights: kWeightsN running-mean weight pairs
    unsigned long long *d_stats = nullptr;       // RT_STATS=1: per-launch scheduling counters
    unsigned long long *d_wave_times = nullptr;  // RT_WAVETIMES=1: per-wave start/end of the last launch
    size_t wave_times_cap = 0;
    bool want_wave_times = false;
    // SIMD rule set (SIMDSpheres + Materials) and scalar rule set (ScalarSpheres)
    SceneBuffers scene[2];
    SceneFacts facts[2];
    bool scene_set = false;
    TileState tiles;
    SelectionStaging sel;
    FirstHitStaging first_hit;
    AsyncTotals totals;
    LastLaunch last;
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

// rt_pack.h, rt_plan.h: the error text other translation units (rt_pack.cpp, rt_plan.cpp, rt_multi.cpp) report
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

extern "C" int rt_device_get_options(rt_device *d, rt_device_options *out) {
    if (!d || !out) return fail(RT_EINVAL, "rt_device_get_options: NULL argument");
    *out = d->opt;
    return RT_OK;
}

// The stream, the tables and the pinned words of a new device.
static int create_device_state(rt_device *d) {
    AsyncTotals &t = d->totals;
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&d->d_lut, 2048 * sizeof(float)) != hipSuccess ||
        hipMalloc(&d->d_weights, kWeightsN * sizeof(float2)) != hipSuccess ||
        hipHostMalloc(&t.h_counts, 2 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&t.ev_counts, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(&t.h_folded, sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&t.ev_folded, hipEventDisableTiming) != hipSuccess)
        return fail(RT_ENOMEM, "rt_device_create: stream/LUT/event allocation failed");
    // IEEE f32 divisions (this file is built with -ffp-contract=off): the bits of the kernel's
    // rcp_rn / div_rn weights, which reproduce the reference's divisions (main.cpp:484-487)
    std::vector<float2> w(kWeightsN);
    for (uint32_t n = 0; n < kWeightsN; ++n) {
        const float d1 = (float)(n + 1u);
        w[n] = make_float2(1.0f / d1, (float)n / d1);
    }
    if (hipMemcpy(d->d_weights, w.data(), kWeightsN * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess)
        return fail(RT_EIO, "rt_device_create: weight table upload failed");
    return RT_OK;
}

extern "C" int rt_device_create_ex(int hip_device, const rt_device_options *options, rt_device **out) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!out) return fail(RT_EINVAL, "rt_device_create: out is NULL");
    // options are checked before anything touches a device
    if (const int rc = check_options(options)) return rc;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(RT_ENODEV, "rt_device_create: no HIP device visible");
    if (hip_device < 0 || hip_device >= count) return fail(RT_EINVAL, "rt_device_create: bad device %d", hip_device);
    HIP_OK(hipSetDevice(hip_device));
    rt_device *d = new rt_device();
    d->ordinal = hip_device;
    if (const int rc = create_device_state(d)) {
        rt_device_destroy(d);
        return rc;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) == hipSuccess && prop.multiProcessorCount > 0)
        d->cu_count = (uint32_t)prop.multiProcessorCount;
    if (options) {
        d->opt = *options;
        d->opt.Size = sizeof(rt_device_options);
        d->sw = from_options(*options);
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
    const TileState &t = d->tiles;
    for (const SceneBuffers &s : d->scene)
        for (void *p : {(void *)s.groups, (void *)s.prim, (void *)s.mats, (void *)s.clusters, (void *)s.clusters_x})
            (void)hipFree(p);
    for (void *p : {(void *)d->d_lut, (void *)d->d_weights, (void *)d->d_stats, (void *)d->d_wave_times, (void *)t.cost,
                    (void *)t.order, (void *)t.order_sorted, (void *)t.aux, (void *)t.scratch, (void *)t.live,
                    (void *)t.cull_counters, (void *)t.masks, (void *)t.pix_perm, (void *)t.pix_cost, (void *)d->sel.d_sel,
                    (void *)d->first_hit.d_sel})
        (void)hipFree(p);
    for (StagedWords *w : {&d->sel.bits, &d->sel.counts, &d->first_hit.bits}) {
        for (int i = 0; i < 2; ++i) {
            if (w->h[i]) (void)hipHostFree(w->h[i]);
            if (w->ev[i]) (void)hipEventDestroy(w->ev[i]);
        }
    }
    if (d->totals.h_folded) (void)hipHostFree(d->totals.h_folded);
    if (d->totals.ev_folded) (void)hipEventDestroy(d->totals.ev_folded);
    if (d->totals.h_counts) (void)hipHostFree(d->totals.h_counts);
    if (d->totals.ev_counts) (void)hipEventDestroy(d->totals.ev_counts);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
    return RT_OK;
}

// ---- Growing device buffers.  One idiom, written once: the buffers of a group share a capacity;
// growing frees them all and allocates them anew, and a failed growth leaves every pointer of the
// group null and the capacity 0, so the next call grows again.  The callers wait first for whatever
// may still read the old buffers, and count the growth and clear the tile key afterwards (grown).
struct Want {
    void **p;
    size_t bytes;
};
template <class T>
static Want want(T *&p, size_t bytes) {
    return {(void **)&p, bytes};
}

static void release(std::initializer_list<Want> bufs) {
    for (const Want &b : bufs) {
        (void)hipFree(*b.p);
        *b.p = nullptr;
    }
}

static int regrow(size_t &cap, size_t new_cap, std::initializer_list<Want> bufs, const char *what) {
    release(bufs);
    cap = 0;
    for (const Want &b : bufs)
        if (hipMalloc(b.p, b.bytes) != hipSuccess) {
            release(bufs);
            return fail(RT_ENOMEM, "%s", what);
        }
    cap = new_cap;
    return RT_OK;
}

// Growing a launch buffer frees one that earlier launches may still read, so `sync` (the caller's
// stream, or the whole device) is waited for first.
static int wait_for(hipStream_t sync, bool device_wide) {
    if (device_wide) HIP_OK(hipDeviceSynchronize());
    else HIP_OK(hipStreamSynchronize(sync));
    return RT_OK;
}

// After a launch buffer grew: what the tile key stood for is gone with the old buffers.
static int grown(rt_device *d) {
    d->last.info.BufferGrowths += 1;
    d->tiles.key.clear();
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
    AsyncTotals &t = d->totals;
    if (t.known) return true;
    if (wait) {
        if (hipEventSynchronize(t.ev_counts) != hipSuccess) return false;
    } else {
        const hipError_t q = hipEventQuery(t.ev_counts);
        if (q != hipSuccess) {
            (void)hipGetLastError();  // "not ready" must not reach a later launch check
            return false;
        }
    }
    t.n_live = (uint32_t)t.h_counts[0];
    t.dead_pixels = t.h_counts[1];
    t.known = true;
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
    SceneBuffers &b = d->scene[rs];
    if (n_groups > b.cap_groups) {
        // +2 padding groups: the kernel's loops prefetch up to group g+2 while testing g
        if (const int rc = regrow(b.cap_groups, n_groups,
                                  {want(b.groups, (size_t)(n_groups + 2) * kGroupF4 * 16),
                                   want(b.mats, (size_t)n_groups * 64u * kSphereF4),
                                   want(b.prim, (size_t)n_groups * kPrimF4 * 16)},
                                  "rt_scene_upload: device allocation failed"))
            return rc;
    }
    HIP_OK(hipMemsetAsync(b.groups + kGroupF4 * (size_t)n_groups, 0, 2 * kGroupF4 * 16, d->stream));
    HIP_OK(hipMemcpyAsync(b.groups, groups.data(), (size_t)n_groups * kGroupF4 * 16, hipMemcpyHostToDevice, d->stream));
    HIP_OK(hipMemcpyAsync(b.mats, mats.data(), (size_t)n_groups * 64u * kSphereF4, hipMemcpyHostToDevice, d->stream));
    d->facts[rs].n_groups = n_groups;
    return RT_OK;
}

// A cluster table's device buffer grown to hold `tab` (the stream's copies into the old one wait first),
// and the table, if there is one, copied into it on the device's stream.
static int upload_table(rt_device *d, float4 *&buf, size_t &cap, const std::vector<float> &tab) {
    const size_t nf4 = tab.size() / 4u;
    if (nf4 > cap) {
        HIP_OK(hipStreamSynchronize(d->stream));
        if (const int rc = regrow(cap, nf4, {want(buf, nf4 * 16u)}, "rt_scene_upload: device allocation failed")) return rc;
    }
    if (nf4) HIP_OK(hipMemcpyAsync(buf, tab.data(), nf4 * 16u, hipMemcpyHostToDevice, d->stream));
    return RT_OK;
}

extern "C" int rt_scene_upload(rt_device *d, const rt_scene *scene) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !scene) return fail(RT_EINVAL, "rt_scene_upload: NULL argument");
    PackedSet ps[2];
    for (int rs = 0; rs < 2; ++rs) {
        const int rc = pack_set(scene, rs, ps[rs], d->sw.pf_rel, d->sw.cluster_k, d->sw.sub_spheres, d->sw.dir_table != 0);
        if (rc) return rc;
    }
    HIP_OK(hipSetDevice(d->ordinal));
    if (const int rc = quiesce(d)) return rc;
    for (int rs = 0; rs < 2; ++rs) {
        SceneFacts &f = d->facts[rs];
        SceneBuffers &b = d->scene[rs];
        f.prefilter = d->sw.prefilter < 0 ? ((ps[rs].prefilter_pays || ps[rs].relative) ? 1u : 0u) : (uint32_t)d->sw.prefilter;
        f.pf_relative = ps[rs].relative ? 1u : 0u;
        f.fast_sqrt = ps[rs].fast_sqrt;
        const int rc = upload_set(d, rs, ps[rs].groups, ps[rs].mats, ps[rs].n_groups);
        if (rc) return rc;
        const ClusterTable &cl = ps[rs].cl;  // (without a table, tab and xtab are empty: rt_pack.h)
        f.n_cpairs = 0;
        if (const int rc2 = upload_table(d, b.clusters, b.cap_clusters, cl.tab)) return rc2;
        if (!cl.tab.empty()) {
            f.n_cpairs = cl.n_cpairs;
            f.cl_words = cl.words;
        }
        f.clusters_x_ok = f.dir_table = false;
        if (cl.dir.empty()) {
            if (const int rc2 = upload_table(d, b.clusters_x, b.cap_clusters_x, cl.xtab)) return rc2;
        } else {
            // the direction block behind the expanded table, its offset in float4 rows in word 3 of the row {c0, .}
            // (rt_layout.h): one buffer, so the kernel reaches the block from TraceArgs.clusters
            std::vector<float> both(cl.xtab);
            const uint32_t at = (uint32_t)(both.size() / 4u);
            memcpy(&both[3], &at, 4);
            both.insert(both.end(), cl.dir.begin(), cl.dir.end());
            if (const int rc2 = upload_table(d, b.clusters_x, b.cap_clusters_x, both)) return rc2;
            HIP_OK(hipStreamSynchronize(d->stream));  // (`both` is pageable and leaves scope here)
            f.dir_table = cl.x_ok;
        }
        f.clusters_x_ok = !cl.xtab.empty() && cl.x_ok;
    }
    HIP_OK(hipStreamSynchronize(d->stream));
    for (SceneFacts &f : d->facts) {
        f.n_spheres = scene->ScalarSpheres.Count;
        f.use_sky = scene->UseSkyColor;
        f.scene_gen += 1;
    }
    d->scene_set = true;
    // a reserved geometry keeps its promise for the new scene's mask words (the
    // device is quiescent here: the upload waited for every launch).  The scene
    // is committed by now, so a failure here does not fail the upload: the
    // reservation is dropped and later launches grow their buffers lazily.
    if (apply_reserve(d) != RT_OK) {
        (void)hipGetLastError();
        d->tiles.reserve_tiles = 0;
        d->tiles.reserve_pixels = 0;
    }
    return RT_OK;
}

// Launch buffers for n_tiles block tiles (cost, order, live flags, sort
// scratch, cull counters).
static int ensure_tile_buffers(rt_device *d, uint32_t n_tiles, hipStream_t sync, bool device_wide) {
    TileState &t = d->tiles;
    if (n_tiles <= t.cap && t.cull_counters) return RT_OK;
    if (const int rc = wait_for(sync, device_wide)) return rc;
    if (n_tiles > t.cap) {
        // cost / order / sort scratch per unit: up to 4 per block tile (wave units)
        if (const int rc = regrow(t.cap, n_tiles,
                                  {want(t.cost, 4u * n_tiles * 4u), want(t.order, 4u * n_tiles * 4u),
                                   want(t.order_sorted, 4u * n_tiles * 4u), want(t.aux, 2u * n_tiles * 4u),
                                   want(t.live, n_tiles * 4u), want(t.scratch, rtk_tile_sort_scratch(4u * n_tiles))},
                                  "rt_trace: tile order buffers"))
            return rc;
        d->last.info.BufferGrowths += 1;
    }
    if (!t.cull_counters && hipMalloc(&t.cull_counters, kCullCounterWords * 8u) != hipSuccess)
        return fail(RT_ENOMEM, "rt_trace: tile order buffers");
    t.key.clear();
    return RT_OK;
}

static int ensure_masks(rt_device *d, size_t mask_words, hipStream_t sync, bool device_wide) {
    TileState &t = d->tiles;
    if (mask_words <= t.mask_cap) return RT_OK;
    if (const int rc = wait_for(sync, device_wide)) return rc;
    if (const int rc = regrow(t.mask_cap, mask_words, {want(t.masks, mask_words * 8u)}, "rt_trace: cull masks")) return rc;
    return grown(d);
}

static int ensure_pixel_sort(rt_device *d, uint32_t n_tiles, size_t pixels, hipStream_t sync, bool device_wide) {
    TileState &t = d->tiles;
    const size_t perm = (size_t)n_tiles * 64u, cost = pixels * 4u;  // bytes
    if (perm <= t.pix_perm_cap && cost <= t.pix_cost_cap) return RT_OK;
    if (const int rc = wait_for(sync, device_wide)) return rc;
    if (perm > t.pix_perm_cap)
        if (const int rc = regrow(t.pix_perm_cap, perm, {want(t.pix_perm, perm)}, "rt_trace: pixel order")) return rc;
    if (cost > t.pix_cost_cap)
        if (const int rc = regrow(t.pix_cost_cap, cost, {want(t.pix_cost, cost)}, "rt_trace: pixel costs")) return rc;
    return grown(d);
}

// The selection buffer for images of up to `ref_tiles` reference tiles: the device copy of the
// bitmap and of rt_trace_tile_work's counts table behind it, and the two pinned slots each of them
// is uploaded from.  The wait covers the slots too (a copy out of a slot is work of that stream),
// so none is in flight afterwards.
static int ensure_sel(rt_device *d, uint32_t ref_tiles, hipStream_t sync, bool device_wide) {
    SelectionStaging &s = d->sel;
    if (ref_tiles <= s.cap) return RT_OK;
    if (const int rc = wait_for(sync, device_wide)) return rc;
    release({want(s.d_sel, 0)});
    s.cap = 0;
    const size_t slot_words[2] = {rtk_sel_table_at(ref_tiles), 2u * (size_t)ref_tiles};  // bitmap, table
    StagedWords *staged[2] = {&s.bits, &s.counts};
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
    if (const int rc = regrow(s.cap, ref_tiles, {want(s.d_sel, rtk_sel_buffer_words(ref_tiles) * 4u)},
                              "rt_trace_tiles: selection buffer"))
        return rc;
    return grown(d);
}

// rt_trace_first_hit's bitmap for images of up to `ref_tiles` reference tiles, and its two pinned slots
// (ensure_sel's scheme).  Nothing of the launch key depends on it: no key is cleared, no growth counted.
static int ensure_first_hit_sel(rt_device *d, uint32_t ref_tiles, hipStream_t sync, bool device_wide) {
    FirstHitStaging &s = d->first_hit;
    if (ref_tiles <= s.cap) return RT_OK;
    if (const int rc = wait_for(sync, device_wide)) return rc;
    release({want(s.d_sel, 0)});
    s.cap = 0;
    const size_t words = rtk_sel_table_at(ref_tiles);  // (the bitmap's words rounded up to a whole u64)
    for (int i = 0; i < 2; ++i) {
        StagedWords &w = s.bits;
        if (w.h[i]) (void)hipHostFree(w.h[i]);
        w.h[i] = nullptr;
        w.in_flight[i] = false;
        if (!w.ev[i] && hipEventCreateWithFlags(&w.ev[i], hipEventDisableTiming) != hipSuccess)
            return fail(RT_ENOMEM, "rt_trace_first_hit: upload event");
        if (hipHostMalloc(&w.h[i], words * 4u, hipHostMallocDefault) != hipSuccess)
            return fail(RT_ENOMEM, "rt_trace_first_hit: pinned staging");
    }
    return regrow(s.cap, ref_tiles, {want(s.d_sel, words * 4u)}, "rt_trace_first_hit: selection buffer");
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
    const TileState &t = d->tiles;
    if (!t.reserve_tiles) return RT_OK;
    const uint32_t n_tiles = t.reserve_tiles;
    uint32_t n_words = 1;
    if (d->scene_set)
        for (const SceneFacts &f : d->facts) n_words = std::max(n_words, rtk_mask_words(f.n_groups));
    if (const int rc = ensure_tile_buffers(d, n_tiles, nullptr, true)) return rc;
    if (const int rc = ensure_sel(d, t.reserve_ref_tiles, nullptr, true)) return rc;  // (rt_trace_tiles, rt_trace_tile_work)
    if (const int rc = ensure_first_hit_sel(d, t.reserve_ref_tiles, nullptr, true)) return rc;  // (rt_trace_first_hit)
    if (d->sw.pixel_sort)
        if (const int rc = ensure_pixel_sort(d, n_tiles, t.reserve_pixels, nullptr, true)) return rc;
    return ensure_masks(d, (size_t)n_tiles * 4u * n_words, nullptr, true);
}

extern "C" int rt_device_reserve(rt_device *d, uint32_t width, uint32_t local_rows) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || width == 0 || local_rows == 0 || width > 65536 || local_rows > 65536)
        return fail(RT_EINVAL, "rt_device_reserve: bad argument");
    HIP_OK(hipSetDevice(d->ordinal));
    TileState &t = d->tiles;
    uint32_t n_tiles = 0;
    for (const int p : {1, 2, 4, 8, 16, 32}) n_tiles = std::max(n_tiles, rtk_tile_count(width, local_rows, p));
    t.reserve_tiles = std::max(t.reserve_tiles, n_tiles);
    t.reserve_pixels = std::max(t.reserve_pixels, (size_t)width * local_rows);
    // (rt_trace_tiles' bitmap and rt_trace_tile_work's table: the reference tiles of a width x local_rows image)
    t.reserve_ref_tiles = std::max(t.reserve_ref_tiles, rt_tile_count(width, local_rows, nullptr));
    return apply_reserve(d);
}

// ---- The trace launch, in stages (trace_launch, below, is their sequence).

// A launch's per-tile counts, by where they come from: none; a host table (rt_trace_tile_work with mixed
// pairs: the table the kernels read, rt_plan.h TileWorkList.table, uploaded through the pinned slots); or
// the caller's device table (rt_trace_tile_counts), from which a pass on the launch's stream builds the
// kernels' table (rtk_launch_counts_table) -- the host never sees a count.
enum CountsSource { kCountsNone = 0, kCountsHost, kCountsDevice };
struct TileCounts {
    CountsSource source = kCountsNone;
    const uint32_t *table = nullptr;  // host: the table
    size_t n_words = 0;               //       2 x the image's reference tiles
    const rt_tile_counts *d_table = nullptr;  // device: the caller's table
    uint32_t max_frames = 0;                  //         the bound its Frames are clamped to
};

// What a launch covers beyond rt_trace's every tile of the band.
// sel (rt_trace_tiles): the listed reference tiles of the full image (one band, validated against
// desc's image and not empty).
// counts (rt_trace_tile_work with mixed pairs, rt_trace_tile_counts; needs sel): every listed tile folds
// its own frames from its own count.  desc then carries the LARGEST Frames of the list (a device table: the
// caller's bound of them), by which the launch shape is chosen (never more lanes than frames; 4 pixels per
// lane at one frame), and PreviousRayCount 0; the kernels take each tile's pair from the table.  Nothing of
// the counts enters the key.  With a device table a listed tile may fold no frame: it rests (no byte of it
// is written), and the closing pass takes the bitmap of the tiles that do not (rtk_sel_active_at).
// d_delta (rt_trace_tile_work_delta; needs sel): the RGBA8 image is left to the closing pass whatever the
// launch shape, and that pass also writes each listed tile's change statistics.  No part of the key either.
struct LaunchRequest {
    const TileSelection *sel = nullptr;
    TileCounts counts;
    rt_tile_delta *d_delta = nullptr;
    bool per_tile() const { return counts.source != kCountsNone; }
};

// The camera and the descriptor into TraceArgs, with the device's scene and table pointers.
static void fill_args(const rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, int rs,
                      uint32_t local_rows, uint64_t *d_rays, TraceArgs &a) {
    memset(&a, 0, sizeof(a));
    a.groups = d->scene[rs].groups;
    a.materials = d->scene[rs].mats;
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
    a.flags = ((desc->Flags & RT_FLAG_ACCUM_ZERO) ? kFlagAccumZero : 0u) |
              ((desc->Flags & RT_FLAG_SRGB_POW) ? kFlagSrgbPow : 0u);
    a.band_rows = desc->BandRows ? desc->BandRows : 32u;
    a.band_count = desc->BandCount ? desc->BandCount : 1u;
    a.band_index = desc->BandIndex;
    a.stats = d->d_stats;
}

// RT_WAVETIMES: one {start, end} per wave of this launch's tile shape
static int wave_times_buffer(rt_device *d, const LaunchPlan &p, TraceArgs &a) {
    const size_t waves = (size_t)rtk_tile_count(a.width, a.local_rows, p.lpp) * 4u;
    if (waves > d->wave_times_cap)
        if (const int rc = regrow(d->wave_times_cap, waves, {want(d->d_wave_times, waves * 16u)}, "wave_times")) return rc;
    a.wave_times = d->d_wave_times;
    return RT_OK;
}

// order, masks and costs are written and read in stream order: on a new
// stream, every launch issued on the previous one must have finished (the
// previous stream may be gone, so the wait is for the device; switching
// streams is rare -- every caller here keeps one per device)
static int switch_stream(rt_device *d, hipStream_t s) {
    TileState &t = d->tiles;
    if (t.stream_set && s == t.stream) return RT_OK;
    if (t.stream_set) HIP_OK(hipDeviceSynchronize());
    t.stream = s;
    t.stream_set = true;
    return RT_OK;
}

// (no allocation here once rt_device_reserve has sized the buffers for this geometry)
static int ensure_buffers(rt_device *d, const LaunchPlan &p, const TraceArgs &a, const TileSelection *sel, hipStream_t s) {
    if (const int rc = ensure_tile_buffers(d, p.n_tiles, s, false)) return rc;
    if (p.cull)
        if (const int rc = ensure_masks(d, p.mask_words, s, false)) return rc;
    if (p.pixel_sort)
        if (const int rc = ensure_pixel_sort(d, p.n_tiles, (size_t)a.width * a.local_rows, s, false)) return rc;
    if (sel)
        if (const int rc = ensure_sel(d, sel->n_tiles, s, false)) return rc;
    return RT_OK;
}

// A new key: its bitmap to the device, then the pass that makes its live list and first order --
// the cull pass, whose totals follow to the host asynchronously (resolve_counts; no host wait
// here), or without culling every tile live (a tile list: the select pass).
static int begin_key(rt_device *d, const LaunchRequest &rq, const LaunchPlan &p, const TraceArgs &a, hipStream_t s) {
    TileState &t = d->tiles;
    AsyncTotals &tot = d->totals;
    unsigned long long *totals = t.cull_counters + kCullTotals;
    // (first, so that a failed upload leaves no key behind that claims its bitmap is on the device)
    t.key.clear();
    if (rq.sel)
        if (const int rc = staged_upload(d->sel.bits, d->sel.d_sel, rq.sel->bits, rq.sel->n_words, s)) return rc;
    t.key = t.next_key;
    t.n_sorts = 0;
    if (p.pixel_sort) HIP_OK(hipMemsetAsync(t.pix_perm, 0xFF, (size_t)p.n_tiles * 64u, s));  // identity
    if (p.cull) {
        t.mask_words = p.mask_words;
        if (rtk_launch_cull(&a, p.lpp, t.live, t.cost, t.cull_counters, p.empty_capable ? 1 : 0, s) != 0 ||
            rtk_launch_tile_sort(t.cost, t.order, t.scratch, p.n_units, s) != 0)
            return fail(RT_EIO, "rt_trace: cull pass launch failed: %s", hipGetErrorString(hipGetLastError()));
        HIP_OK(hipMemcpyAsync(tot.h_counts, totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_OK(hipEventRecord(tot.ev_counts, s));
        tot.known = false;
        t.order_valid = true;
        return RT_OK;
    }
    HIP_OK(hipMemsetAsync(t.cost, 0, p.n_units * 4u, s));
    // no cull pass: every block tile is live, and the totals word the XCD grouping reads
    // (rtk_launch_xcd_group) says so (u64 little-endian: low word n_tiles, the rest 0)
    HIP_OK(hipMemsetAsync(totals, 0, 2 * sizeof(unsigned long long), s));
    HIP_OK(hipMemsetD32Async((hipDeviceptr_t)totals, p.n_selected, 1, s));
    tot.n_live = p.n_selected;
    tot.dead_pixels = 0;
    tot.known = true;
    t.order_valid = false;  // identity until a measured sort exists
    if (rq.sel) {
        // a tile list: the identity order would trace unlisted tiles, so the selected
        // tiles (cost 2, the others 0) are sorted to the front and the grid is their count
        if (rtk_launch_select(&a, p.lpp, t.live, t.cost, s) != 0 ||
            rtk_launch_tile_sort(t.cost, t.order, t.scratch, p.n_units, s) != 0)
            return fail(RT_EIO, "rt_trace_tiles: select pass launch failed: %s", hipGetErrorString(hipGetLastError()));
        t.order_valid = true;
    }
    return RT_OK;
}

// live-tile count: on the host once the cull totals have landed, else read
// by the kernels from the device (grid over every tile, early exit)
struct LiveCounts {
    uint32_t grid_tiles;
    bool any_live, any_dead;
};
static LiveCounts live_counts(rt_device *d, const LaunchPlan &p, TraceArgs &a) {
    const bool known = resolve_counts(d, false);
    const uint32_t n_live = d->totals.n_live;
    a.live_total = known ? nullptr : d->tiles.cull_counters + kCullTotals;
    return {known ? n_live : p.n_tiles, !known || n_live > 0, p.empty_capable && (!known || n_live < p.n_selected)};
}

// The key's order and this call's table into the arguments of the trace launches.
static int bind_launch(rt_device *d, const LaunchRequest &rq, const LaunchPlan &p, TraceArgs &a, hipStream_t s) {
    const TileState &t = d->tiles;
    a.tile_order = t.order_valid ? t.order : nullptr;
    if (rq.per_tile()) {  // this call's table, whatever the key: the counts are no part of it
        const uint32_t n_ref = rq.sel->n_tiles;
        a.tile_counts_at = rtk_sel_table_at(n_ref);
        uint32_t *table = d->sel.d_sel + a.tile_counts_at;
        if (rq.counts.source == kCountsHost) {
            if (const int rc = staged_upload(d->sel.counts, table, rq.counts.table, rq.counts.n_words, s)) return rc;
        } else if (rtk_launch_counts_table(rq.counts.d_table, d->sel.d_sel, n_ref, rq.counts.max_frames, table,
                                           d->sel.d_sel + rtk_sel_active_at(n_ref), s) != 0) {
            // (the key's bitmap is on the device by now: begin_key's upload, or an earlier call's)
            return fail(RT_EIO, "rt_trace_tile_counts: table pass launch failed: %s", hipGetErrorString(hipGetLastError()));
        }
    }
    // (the identity order knows no selection: both paths of begin_key leave a sorted order for a tile list)
    if (rq.sel && !a.tile_order) return fail(RT_EIO, "rt_trace_tiles: no tile order for the selection");
    a.tile_cost = p.sched ? t.cost : nullptr;
    a.pix_perm = p.pixel_sort ? t.pix_perm : nullptr;
    a.pix_seg = d->sw.pixel_seg;
    a.skip_cur = p.skip_cur;
    return RT_OK;
}

static void record_info(rt_device *d, const rt_trace_desc *desc, const LaunchRequest &rq, const LaunchPlan &p,
                        const TraceArgs &a, bool new_key) {
    LastLaunch &l = d->last;
    l.info.PixelsSorted = p.pixel_sort && !new_key && d->tiles.n_sorts > 0 ? 1u : 0u;
    l.n_tiles = p.n_selected;  // (SegmentsFolded: the dead tiles among these)
    l.info.TilesSelected = p.n_selected;
    l.frames = desc->Frames;
    l.empty_capable = p.empty_capable;
    l.info.LanesPerPixel = p.lanes;
    l.info.PixelsPerLane = p.pixels_per_lane;
    l.info.TilesTotal = p.n_tiles;
    l.info.CullPassRan = p.cull && new_key ? 1u : 0u;
    l.info.OrderedLaunches = d->tiles.n_sorts;
    l.info.ClusteredWalk = a.clusters ? 1u : 0u;
    l.info.GroupsPerRuleSet = a.n_groups;
    l.info.OneWaveGroups = a.solo;
    l.info.Walk = a.walk;
    l.tile_counts = rq.per_tile();
    l.dir_table = rtk_walk_direction(a, p.cull, p.lpp);
    l.folded_on_device = false;
}

// The pixels of dead tiles, folded without tracing.
static int fold_empty_tiles(rt_device *d, const LaunchRequest &rq, const LaunchPlan &p, const TraceArgs &a, hipStream_t s) {
    TileState &t = d->tiles;
    if (!rq.per_tile()) {
        if (rtk_launch_empty(&a, p.lpp, t.live, t.cull_counters + kCullTotals + 1, s) != 0)
            return fail(RT_EIO, "rt_trace: empty-tile launch failed: %s", hipGetErrorString(hipGetLastError()));
        return RT_OK;
    }
    // each dead tile folds by its own pair, and the device sums the segments (they are no longer
    // dead pixels x frames); the sum follows to the host asynchronously, as the cull totals do
    unsigned long long *folded = t.cull_counters + kCullFolded;
    HIP_OK(hipMemsetAsync(folded, 0, sizeof(unsigned long long), s));
    if (rtk_launch_empty_counts(&a, p.lpp, t.live, folded, s) != 0)
        return fail(RT_EIO, "rt_trace_tile_work: empty-tile launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_OK(hipMemcpyAsync(d->totals.h_folded, folded, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_OK(hipEventRecord(d->totals.ev_folded, s));
    d->last.folded_on_device = true;
    return RT_OK;
}

// The next launch's order from the costs this one measured.
// The learned order settles within a few launches (C2: 7.7, 6.3, 6.1, 5.9,
// 5.8 ms); after order_launches re-sorts (options OrderLaunches, default 4)
// the order is kept and the three sort kernels (~14 us per launch, 1.5 %
// of an 8-rank C2 share) are skipped
static int resort_tiles(rt_device *d, const LaunchPlan &p, const TraceArgs &a, hipStream_t s) {
    TileState &t = d->tiles;
    t.n_sorts += 1;
    const bool group = p.xcd_group;
    if (rtk_launch_tile_sort(t.cost, group ? t.order_sorted : t.order, t.scratch, p.n_units, s) != 0 ||
        (group && rtk_launch_xcd_group(t.order_sorted, t.order, p.n_units, t.cull_counters + kCullTotals, t.scratch,
                                       t.aux, s) != 0))
        return fail(RT_EIO, "rt_trace: tile sort launch failed: %s", hipGetErrorString(hipGetLastError()));
    if (p.pixel_sort && rtk_launch_pixel_sort(&a, p.lpp, t.pix_perm, s) != 0)
        return fail(RT_EIO, "rt_trace: pixel sort launch failed: %s", hipGetErrorString(hipGetLastError()));
    t.order_valid = true;
    return RT_OK;
}

// one launch, or the split of a key's first launch (split_schedule): the leading
// parts, then the rest, each continuing the running mean heaviest-first
static int run_parts(rt_device *d, const rt_trace_desc *desc, const LaunchRequest &rq, const LaunchPlan &p,
                     const SplitSchedule &split, const LiveCounts &live, TraceArgs &a, hipStream_t s) {
    const TileState &t = d->tiles;
    uint32_t done_frames = 0;
    for (uint32_t part = 0; part < split.n_parts; ++part) {
        if (part > 0) {
            a.prev_count = desc->PreviousRayCount + done_frames;
            a.flags &= ~kFlagAccumZero;
            a.tile_order = t.order;
        }
        a.frames = split.parts[part];
        done_frames += split.parts[part];
        const bool resort = p.sched && live.any_live && (t.n_sorts < d->sw.order_launches || part + 1 < split.n_parts);
        a.pix_cost = p.pixel_sort && resort ? t.pix_cost : nullptr;
        // wave costs only for a launch whose costs are sorted: once the order is kept, the
        // per-wave 4-B cost stores (scattered partial lines, ~8 MB of HBM writes per 1080p
        // launch at P = 4) would feed nothing
        a.tile_cost = resort ? t.cost : nullptr;
        if (rtk_launch_trace_grid(&a, desc->EnableSIMD ? 1 : 0, p.src, p.cull ? 1 : 0, p.lpp, live.grid_tiles, s) != 0)
            return fail(RT_EIO, "rt_trace: kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
        if (live.any_dead)
            if (const int rc = fold_empty_tiles(d, rq, p, a, s)) return rc;
        if (resort)
            if (const int rc = resort_tiles(d, p, a, s)) return rc;
    }
    return RT_OK;
}

// options EncodePass: the RGBA8 band image from the running mean the kernels stored (main.cpp:490's
// store on its own, the same bits), written by one coalesced pass
// (a tile list: over the listed tiles' pixels only, so no other RGBA8 pixel is written)
// (rt_trace_tile_work_delta: the same pass, one block per listed tile, with the tile's statistics)
// (rt_trace_tile_counts: over the listed tiles that folded a frame -- the table pass's bitmap in place of the key's)
static int closing_pass(const rt_device *d, const rt_trace_desc *desc, const LaunchRequest &rq, const TraceArgs &launched,
                        hipStream_t s) {
    if (!launched.skip_cur || desc->Frames == 0) return RT_OK;
    TraceArgs a = launched;
    if (rq.counts.source == kCountsDevice) a.sel = d->sel.d_sel + rtk_sel_active_at(rq.sel->n_tiles);
    if ((rq.d_delta ? rtk_launch_tile_delta_encode(&a, rq.d_delta, s)
         : rq.sel   ? rtk_launch_encode_selected(&a, s)
                    : rtk_launch_encode(a.prev, a.cur, (uint64_t)a.local_rows * desc->Width,
                                        (a.flags & kFlagSrgbPow) ? 1u : 0u, s)) != 0)
        return fail(RT_EIO, "rt_trace: RGBA8 encode launch failed: %s", hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

// rt_trace, rt_trace_tiles, rt_trace_tile_work, rt_trace_tile_work_delta and rt_trace_tile_counts behind their own checks.
static int trace_launch(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, const LaunchRequest &rq,
                        uint64_t *d_rays, void *stream) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (const int rc = check_trace_args(d != nullptr, d && d->lut_set, d && d->scene_set, cam, desc, d_rays)) return rc;
    const uint32_t local_rows = rt_band_local_rows(desc->Height, desc->BandRows ? desc->BandRows : 32u,
                                                   desc->BandCount ? desc->BandCount : 1u, desc->BandIndex);
    if (desc->Frames == 0 || local_rows == 0) return RT_OK;
    if (!cam->CurrentImage.Data || !cam->PreviousImage.Data)
        return fail(RT_EINVAL, "rt_trace: CurrentImage/PreviousImage device pointers missing");
    const int rs = desc->EnableSIMD ? 0 : 1;
    TileState &t = d->tiles;
    TraceArgs a;
    fill_args(d, cam, desc, rs, local_rows, d_rays, a);
    const LaunchPlan p = plan_launch(d->sw, d->facts[rs], rs, d->cu_count, *desc, local_rows, rq.sel, rq.per_tile(),
                                     rq.d_delta != nullptr, {d->scene[rs].clusters, d->scene[rs].clusters_x}, a, t.next_key);
    HIP_OK(hipSetDevice(d->ordinal));
    hipStream_t s = (hipStream_t)stream;  // NULL = the HIP null stream
    if (d->want_wave_times)
        if (const int rc = wave_times_buffer(d, p, a)) return rc;
    if (const int rc = switch_stream(d, s)) return rc;
    if (const int rc = ensure_buffers(d, p, a, rq.sel, s)) return rc;
    const bool new_key = t.next_key != t.key;
    // the key's bitmap on the device (uploaded by begin_key; the same list again finds it there)
    a.sel = rq.sel ? d->sel.d_sel : nullptr;
    a.sel_tiles_x = rq.sel ? rq.sel->tiles_x : 0u;
    // (the table is written by the key's cull pass: the key holds the camera and the scene)
    a.prim = p.cull ? d->scene[rs].prim : nullptr;
    a.masks = p.cull ? t.masks : nullptr;
    if (new_key)
        if (const int rc = begin_key(d, rq, p, a, s)) return rc;
    // (a culled new key's launch may split; not with per-tile counts: a split would need a head per tile)
    const SplitSchedule split = split_schedule(desc->Frames, p.lanes, d->sw.head_samples, d->sw.split_parts, d->sw.split_growth,
                                               new_key && p.cull && p.sched && d->sw.split && !rq.per_tile());
    const LiveCounts live = live_counts(d, p, a);
    if (const int rc = bind_launch(d, rq, p, a, s)) return rc;
    record_info(d, desc, rq, p, a, new_key);
    if (const int rc = run_parts(d, desc, rq, p, split, live, a, s)) return rc;
    if (const int rc = closing_pass(d, desc, rq, a, s)) return rc;
    d->last.info.SplitHeadFrames = split.head_frames;
    return RT_OK;
}

extern "C" int rt_trace(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, uint64_t *d_rays,
                        void *stream) {
    return trace_launch(d, cam, desc, LaunchRequest(), d_rays, stream);
}

extern "C" int rt_trace_tiles(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, const uint32_t *tiles,
                              uint32_t n_tiles, uint64_t *d_rays, void *stream) {
    if (const int rc = check_trace_args(d != nullptr, d && d->lut_set, d && d->scene_set, cam, desc, d_rays)) return rc;
    if (desc->BandCount > 1u || desc->BandIndex != 0u)
        return fail(RT_EINVAL, "rt_trace_tiles: tiles index the whole image (BandCount 0 or 1, BandIndex 0)");
    if (!tiles && n_tiles) return fail(RT_EINVAL, "rt_trace_tiles: tiles is NULL with n_tiles %u", n_tiles);
    // the list is consumed here: the bitmap lives in the device's own host vector, and a new key's
    // upload goes through the library's pinned slots, so the caller's array is free on return
    TileSelection sel;
    const ListName name = {"rt_trace_tiles", "tiles[", "]"};
    if (const int rc = select_tiles(name, tiles, n_tiles, desc->Width, desc->Height, d->sel.tile_bits, sel)) return rc;
    if (n_tiles == 0 || desc->Frames == 0) return RT_OK;
    LaunchRequest rq;
    rq.sel = &sel;
    return trace_launch(d, cam, desc, rq, d_rays, stream);
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
    if (const int rc = check_trace_args(d != nullptr, d && d->lut_set, d && d->scene_set, cam, &dd, d_rays)) return rc;
    if (desc->BandCount > 1u || desc->BandIndex != 0u)
        return fail(RT_EINVAL, "rt_trace_tile_work: tiles index the whole image (BandCount 0 or 1, BandIndex 0)");
    if (!work && n_work) return fail(RT_EINVAL, "rt_trace_tile_work: work is NULL with n_work %u", n_work);
    // The list is consumed here (the device's own host vectors; the uploads go through the library's
    // pinned slots), so the caller's array is free on return.
    TileWorkList &w = d->sel.work;
    if (const int rc = plan_tile_work(work, n_work, desc->Width, desc->Height, w)) return rc;
    if (w.kept == 0) return RT_OK;
    LaunchRequest rq;
    rq.sel = &w.sel;
    rq.d_delta = d_delta;
    if (w.uniform) {  // one pair: rt_trace_tiles with it -- the same path, kernels and first-launch split
        dd.PreviousRayCount = w.first.PreviousRayCount;
        dd.Frames = w.first.Frames;
        return trace_launch(d, cam, &dd, rq, d_rays, stream);
    }
    dd.Frames = w.max_frames;  // (the launch shape's frames; PreviousRayCount stays 0: every tile has its own)
    rq.counts.source = kCountsHost;
    rq.counts.table = w.table.data();
    rq.counts.n_words = w.table.size();
    return trace_launch(d, cam, &dd, rq, d_rays, stream);
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

extern "C" int rt_trace_tile_counts(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc,
                                    const uint32_t *tiles, uint32_t n_tiles, const rt_tile_counts *d_counts,
                                    uint32_t max_frames, rt_tile_delta *d_delta, uint64_t *d_rays, void *stream) {
    // the device-free plan of the call (rt_plan.cpp): its refusals, the list's selection, the launch's desc.
    // The list is consumed here (the bitmap lives in the device's own host vector), the table never read.
    if (!d) return fail(RT_EINVAL, "rt_trace: NULL argument");
    TileCountsCall call;
    if (const int rc = plan_tile_counts(true, d->lut_set, d->scene_set, cam, desc, tiles, n_tiles, d_counts, max_frames,
                                        d_delta, d_rays, d->sel.tile_bits, call))
        return rc;
    if (call.nothing) return RT_OK;
    LaunchRequest rq;
    rq.sel = &call.sel;
    rq.d_delta = d_delta;
    rq.counts.source = kCountsDevice;
    rq.counts.d_table = d_counts;
    rq.counts.max_frames = max_frames;
    return trace_launch(d, cam, &call.desc, rq, d_rays, stream);
}

extern "C" int rt_tile_counts_step(rt_tile_counts *d_counts, const rt_tile_delta *d_delta, uint32_t width, uint32_t height,
                                   const rt_tile_rule *rule, rt_tile_step_summary *d_summary, void *stream) {
    uint32_t n_tiles = 0;
    if (const int rc = check_tile_step(d_counts, d_delta, width, height, rule, &n_tiles)) return rc;
    if (rtk_launch_tile_counts_step(d_counts, d_delta, n_tiles, rule->MaxRoundFrames, rule->MaxTileFrames,
                                    rule->RestMaxDelta, rule->RestSumSquares, d_summary, (hipStream_t)stream) != 0)
        return fail(RT_EIO, "rt_tile_counts_step: launch failed");
    return RT_OK;
}

// The first segment of every pixel of the listed tiles as a pass of its own (rt_first_hit.hip).  Nothing of the
// launch state is read or written: no key, masks, order, costs or totals, and d->last stays what it was.
extern "C" int rt_trace_first_hit(rt_device *d, const rt_camera_info *cam, const rt_trace_desc *desc, const uint32_t *tiles,
                                  uint32_t n_tiles, uint32_t flags, const rt_first_hit_planes *out, void *stream) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d) return fail(RT_EINVAL, "rt_trace_first_hit: NULL argument");
    // the device-free plan of the call (rt_plan.cpp): its refusals and the list's selection.  The list is
    // consumed here (the bitmap lives in the device's own host vector), so the caller's array is free on return.
    FirstHitCall call;
    if (const int rc = plan_first_hit(true, d->scene_set, cam, desc, tiles, n_tiles, flags, out, d->first_hit.tile_bits, call))
        return rc;
    if (call.nothing) return RT_OK;
    const int rs = desc->EnableSIMD ? 0 : 1;
    TraceArgs a;
    fill_args(d, cam, desc, rs, desc->Height, nullptr, a);
    // (what the pass does not read stays out of its arguments: the images, Frames, MaxBounce and Flags)
    a.prev = nullptr;
    a.cur = nullptr;
    a.frames = a.max_bounce = a.flags = 0u;
    const SceneFacts &f = d->facts[rs];
    a.n_groups = f.n_groups;
    a.n_spheres = f.n_spheres;
    a.fast_sqrt = f.fast_sqrt;  // the scene fact the trace launches use
    a.tiles_x = rtk_tiles_x(desc->Width, 1);
    HIP_OK(hipSetDevice(d->ordinal));
    hipStream_t s = (hipStream_t)stream;  // NULL = the HIP null stream
    if (const int rc = switch_stream(d, s)) return rc;
    if (!call.all) {
        if (const int rc = ensure_first_hit_sel(d, call.sel.n_tiles, s, false)) return rc;
        if (const int rc = staged_upload(d->first_hit.bits, d->first_hit.d_sel, call.sel.bits, call.sel.n_words, s)) return rc;
        a.sel = d->first_hit.d_sel;
        a.sel_tiles_x = call.sel.tiles_x;
    }
    if (rtk_launch_first_hit(&a, desc->EnableSIMD ? 1 : 0, d->sw.cull, (flags & RT_HIT_PIXEL_CENTRE) ? 1 : 0, out->Hit,
                             out->Normal, out->Albedo, s) != 0)
        return fail(RT_EIO, "rt_trace_first_hit: launch failed: %s", hipGetErrorString(hipGetLastError()));
    return RT_OK;
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

// The a-trous filter over the first-hit planes (rt_denoise.hip): the plan's passes (rt_plan.cpp), one launch
// each.  No device handle, no state, no allocation, no wait.
extern "C" int rt_denoise(const rt_denoise_desc *desc, void *stream) {
    DenoisePlan plan;
    if (const int rc = plan_denoise(desc, plan)) return rc;
    const bool demodulate = (desc->Flags & RT_DENOISE_DEMODULATE) != 0u;
    for (uint32_t i = 0; i < plan.n_passes; ++i) {
        const bool last = i + 1u == plan.n_passes;
        DenoiseArgs a;
        a.src = plan.pass[i].src;
        a.dst = plan.pass[i].dst;
        a.hit = desc->Hit;
        a.normal = desc->Normal;
        a.albedo = desc->Albedo;
        a.rgba8 = last ? desc->Rgba8 : nullptr;
        a.width = desc->Width;
        a.height = desc->Height;
        a.step = plan.pass[i].step;
        a.normal_power = desc->NormalPower;
        a.sigma_depth = desc->SigmaDepth;
        a.ic = plan.pass[i].ic;
        a.demod_in = demodulate && i == 0u ? 1u : 0u;
        a.remod_out = demodulate && last ? 1u : 0u;
        a.srgb_pow = (desc->Flags & RT_DENOISE_SRGB_POW) ? 1u : 0u;
        if (rtk_launch_denoise_pass(&a, (hipStream_t)stream) != 0)
            return fail(RT_EIO, "rt_denoise: launch of pass %u failed: %s", i, hipGetErrorString(hipGetLastError()));
    }
    return RT_OK;
}

extern "C" int rt_denoise_defaults(rt_denoise_desc *out) {
    if (!out) return fail(RT_EINVAL, "rt_denoise_defaults: NULL argument");
    memset(out, 0, sizeof(*out));
    out->Size = (uint32_t)sizeof(*out);
    out->Iterations = 3u;
    out->NormalPower = 2u;
    out->SigmaDepth = 0.25f;
    out->SigmaColor = 0.5f;
    return RT_OK;
}

// The running mean across a camera move (rt_reproject.hip): the refusals and the launch's arguments are the
// plan's (rt_plan.cpp), the call is one launch.  No device handle, no state, no allocation, no wait.
extern "C" int rt_reproject(const rt_reproject_desc *desc, void *stream) {
    ReprojectArgs a;
    if (const int rc = plan_reproject(desc, a)) return rc;
    if (rtk_launch_reproject(&a, (hipStream_t)stream) != 0)
        return fail(RT_EIO, "rt_reproject: launch failed: %s", hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

extern "C" int rt_reproject_defaults(rt_reproject_desc *out) {
    if (!out) return fail(RT_EINVAL, "rt_reproject_defaults: NULL argument");
    memset(out, 0, sizeof(*out));
    out->Size = (uint32_t)sizeof(*out);
    out->Frames = 1u;
    out->MaxHistory = 8u;
    out->DepthTolerance = 0.1f;
    return RT_OK;
}

// rt_reproject with the history clamped to the fresh neighbourhood's band (rt_reproject.hip): plan_reproject_clip's
// refusals and arguments, one launch.  No device handle, no state, no allocation, no wait.
extern "C" int rt_reproject_clip(const rt_reproject_clip_desc *desc, void *stream) {
    ReprojectClipArgs c;
    if (const int rc = plan_reproject_clip(desc, c)) return rc;
    if (rtk_launch_reproject_clip(&c, (hipStream_t)stream) != 0)
        return fail(RT_EIO, "rt_reproject_clip: launch failed: %s", hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

extern "C" int rt_reproject_clip_defaults(rt_reproject_clip_desc *out) {
    if (!out) return fail(RT_EINVAL, "rt_reproject_clip_defaults: NULL argument");
    memset(out, 0, sizeof(*out));
    out->Size = (uint32_t)sizeof(*out);
    out->Radius = 1u;
    out->Gamma = 0.5f;
    return rt_reproject_defaults(&out->Reproject);
}

extern "C" int rt_trace_last_info(rt_device *d, rt_trace_info *out) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !out) return fail(RT_EINVAL, "rt_trace_last_info: NULL argument");
    // the live/dead totals of the last launch's key: waits for them if they
    // are still on their way from the device (the only blocking part)
    HIP_OK(hipSetDevice(d->ordinal));
    if (!resolve_counts(d, true)) return fail(RT_EIO, "rt_trace_last_info: cull totals: %s",
                                              hipGetErrorString(hipGetLastError()));
    LastLaunch &l = d->last;
    l.info.TilesTraced = d->totals.n_live;
    l.info.SegmentsFolded = l.empty_capable && d->totals.n_live < l.n_tiles ? d->totals.dead_pixels * l.frames : 0u;
    if (l.folded_on_device) {  // per-tile counts: the device's own sum (waits for it, as above)
        HIP_OK(hipEventSynchronize(d->totals.ev_folded));
        l.info.SegmentsFolded = *d->totals.h_folded;
    }
    *out = l.info;
    return RT_OK;
}

extern "C" int rt_trace_last_tile_counts(rt_device *d, uint32_t *out) {
    if (!d || !out) return fail(RT_EINVAL, "rt_trace_last_tile_counts: NULL argument");
    *out = d->last.tile_counts ? 1u : 0u;
    return RT_OK;
}

extern "C" int rt_trace_last_direction_table(rt_device *d, uint32_t *out) {
    if (!d || !out) return fail(RT_EINVAL, "rt_trace_last_direction_table: NULL argument");
    *out = d->last.dir_table ? 1u : 0u;
    return RT_OK;
}

extern "C" int rt_direction_union(rt_device *d, const uint32_t *words, uint32_t mask_bits, uint64_t lanes,
                                  const uint32_t *canary_in, uint32_t out_union[2], uint32_t *canary_out) {
    DeviceGuard device_guard;  // the caller's current device is restored on return
    if (!d || !words || !canary_in || !out_union || !canary_out)
        return fail(RT_EINVAL, "rt_direction_union: NULL argument");
    if (mask_bits != 32u && mask_bits != 64u) return fail(RT_EINVAL, "rt_direction_union: MaskBits %u is not 32 or 64", mask_bits);
    if (lanes == 0ull) return fail(RT_EINVAL, "rt_direction_union: no lane (a round has at least one)");
    HIP_OK(hipSetDevice(d->ordinal));
    const bool wide = mask_bits == 64u;
    uint32_t h_in[192] = {}, h_out[66] = {};
    for (uint32_t l = 0; l < 64u; ++l) {
        h_in[l] = wide ? words[2u * l] : words[l];
        h_in[64u + l] = wide ? words[2u * l + 1u] : 0u;
        h_in[128u + l] = canary_in[l];
    }
    uint32_t *d_buf = nullptr;
    if (hipMalloc(&d_buf, sizeof(h_in) + sizeof(h_out)) != hipSuccess) return fail(RT_ENOMEM, "rt_direction_union: device allocation");
    int rc = RT_OK;
    if (hipMemcpy(d_buf, h_in, sizeof(h_in), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_buf + 192, 0, sizeof(h_out)) != hipSuccess ||
        rtk_launch_direction_union(d_buf, lanes, wide ? 1u : 0u, d_buf + 192, nullptr) != 0 ||
        hipMemcpy(h_out, d_buf + 192, sizeof(h_out), hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(RT_EIO, "rt_direction_union: %s", hipGetErrorString(hipGetLastError()));
    (void)hipFree(d_buf);
    if (rc != RT_OK) return rc;
    out_union[0] = h_out[0], out_union[1] = h_out[1];
    memcpy(canary_out, h_out + 2, 64u * sizeof(uint32_t));
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
    const TileState &t = d->tiles;
    if (!t.masks || t.key.empty() || !t.mask_words) return 0;
    const uint64_t n = max_words < t.mask_words ? max_words : t.mask_words;
    HIP_OK(hipSetDevice(d->ordinal));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out, t.masks, n * 8u, hipMemcpyDeviceToHost));
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
