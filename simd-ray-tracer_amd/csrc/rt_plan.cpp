// rt_plan.cpp — the launch decisions (rt_plan.h).  Host arithmetic only: this unit calls nothing of
// the HIP runtime and links without it (tests/plan_check).
#include "rt_plan.h"

#include <string.h>

#include <algorithm>

#include "rtk_shape.h"

int check_options(const rt_device_options *o) {
    if (!o) return RT_OK;
    if (o->Size != 0 && o->Size != sizeof(rt_device_options))
        return rt_fail(RT_EINVAL, "rt_device_options: Size %u, this library's is %zu", o->Size, sizeof(rt_device_options));
    const int32_t tri[] = {o->Cull, o->Prefilter, o->PrefilterRelative, o->Clusters, o->OneWaveGroups,
                           o->SphereSourceLds, o->SceneInHbm, o->TablesInLds, o->WalkAny, o->Interleave,
                           o->MergeRounds, o->TileOrder, o->WaveOrder, o->PixelSort, o->XcdGroup,
                           o->SplitFirstLaunch, o->EncodePass, o->DirectionTable};
    for (const int32_t v : tri)
        if (v < -1 || v > 1) return rt_fail(RT_EINVAL, "rt_device_options: a switch is %d (RT_OPT_DEFAULT/ON/OFF)", v);
    const int32_t lpp = o->LanesPerPixel;
    if (!(lpp == 0 || lpp == 1 || lpp == 2 || lpp == 4 || lpp == 8 || lpp == 16 || lpp == 32))
        return rt_fail(RT_EINVAL, "rt_device_options: LanesPerPixel %d", lpp);
    if (!(o->PixelsPerLane == 0 || o->PixelsPerLane == 1 || o->PixelsPerLane == 4))
        return rt_fail(RT_EINVAL, "rt_device_options: PixelsPerLane %d", o->PixelsPerLane);
    if (!(o->PixelSegment == 0 || o->PixelSegment == 1 || o->PixelSegment == 2 || o->PixelSegment == 4))
        return rt_fail(RT_EINVAL, "rt_device_options: PixelSegment %d", o->PixelSegment);
    if (o->SplitParts < 0 || o->SplitParts > 8 || o->HeadSamples < 0 || o->SplitGrowth < 0 || o->OrderLaunches < -1 ||
        o->SecondaryThreshold < 0 || o->SecondaryThreshold > 64 || o->ClusterCount < 0 || o->ClusterCount == 1 ||
        o->SubClusterSpheres < 0)
        return rt_fail(RT_EINVAL, "rt_device_options: a count is out of range");
    return RT_OK;
}

Switches from_options(const rt_device_options &o) {
    auto on = [](int32_t v, bool dflt) { return v == RT_OPT_DEFAULT ? dflt : v == RT_OPT_ON; };
    auto tri = [](int32_t v) { return v == RT_OPT_DEFAULT ? -1 : v == RT_OPT_ON ? 1 : 0; };
    Switches s;
    s.cull = on(o.Cull, true) ? 1 : 0;
    s.prefilter = tri(o.Prefilter);
    s.pf_rel = tri(o.PrefilterRelative);
    s.clusters = o.Clusters == RT_OPT_DEFAULT ? 1 : o.Clusters == RT_OPT_ON ? 2 : 0;
    s.cluster_k = (uint32_t)o.ClusterCount;
    s.sub_spheres = (uint32_t)o.SubClusterSpheres;
    s.sec_threshold = (uint32_t)o.SecondaryThreshold;
    s.lanes_per_pixel = o.LanesPerPixel;
    s.pixels_per_lane = o.PixelsPerLane;
    s.solo = on(o.OneWaveGroups, true) ? 1 : 0;
    s.src = on(o.SphereSourceLds, false) ? kSrcLds : kSrcSmem;
    s.scene_global = on(o.SceneInHbm, false) ? 1 : 0;
    s.tables_global = on(o.TablesInLds, true) ? 0 : 1;
    s.walk_any = on(o.WalkAny, false) ? 1 : 0;
    s.interleave = on(o.Interleave, false) ? 1 : 0;
    s.merge = tri(o.MergeRounds);
    s.tile_sched = on(o.TileOrder, true) ? 1 : 0;
    s.wave_order = on(o.WaveOrder, true) ? 1 : 0;
    s.pixel_sort = on(o.PixelSort, true) ? 1 : 0;
    if (o.PixelSegment) s.pixel_seg = (uint32_t)o.PixelSegment;
    s.xcd_group = tri(o.XcdGroup);
    s.split = on(o.SplitFirstLaunch, true) ? 1 : 0;
    if (o.HeadSamples) s.head_samples = (uint32_t)o.HeadSamples;
    if (o.SplitParts) s.split_parts = (uint32_t)o.SplitParts;
    if (o.SplitGrowth) s.split_growth = (uint32_t)o.SplitGrowth;
    if (o.OrderLaunches) s.order_launches = o.OrderLaunches < 0 ? 0u : (uint32_t)o.OrderLaunches;
    s.cur_pass = on(o.EncodePass, true) ? 1u : 0u;
    s.dir_table = o.DirectionTable == RT_OPT_DEFAULT ? 1 : o.DirectionTable == RT_OPT_ON ? 2 : 0;
    return s;
}

extern "C" uint32_t rtk_tiles_x(uint32_t width, int lanes_per_pixel) {
    return rtk_tile_count(width, 1u, lanes_per_pixel);
}

extern "C" uint32_t rtk_tile_count(uint32_t width, uint32_t local_rows, int lanes_per_pixel) {
    uint32_t bw = 16u, bh = 16u;  // 2*TW x 2*TH of the launch's shape
    switch (lanes_per_pixel) {
        case 32: bw = 2u * rtk::Shape<32>::TW; bh = 2u * rtk::Shape<32>::TH; break;
        case 16: bw = 2u * rtk::Shape<16>::TW; bh = 2u * rtk::Shape<16>::TH; break;
        case 8: bw = 2u * rtk::Shape<8>::TW; bh = 2u * rtk::Shape<8>::TH; break;
        case 4: bw = 2u * rtk::Shape<4>::TW; bh = 2u * rtk::Shape<4>::TH; break;
        case 2: bw = 2u * rtk::Shape<2>::TW; bh = 2u * rtk::Shape<2>::TH; break;
        case 0: bw = 2u * rtk::Shape<0>::TW; bh = 2u * rtk::Shape<0>::TH; break;
        default: bw = 2u * rtk::Shape<1>::TW; bh = 2u * rtk::Shape<1>::TH; break;
    }
    return ((width + bw - 1u) / bw) * ((local_rows + bh - 1u) / bh);
}

extern "C" uint32_t rt_tile_count(uint32_t width, uint32_t height, uint32_t *out_tiles_x) {
    const bool ok = width != 0 && height != 0 && width <= 65536 && height <= 65536;
    const uint32_t tx = ok ? (width + RT_TILE_SIZE - 1u) / RT_TILE_SIZE : 0u;
    if (out_tiles_x) *out_tiles_x = tx;
    return ok ? tx * ((height + RT_TILE_SIZE - 1u) / RT_TILE_SIZE) : 0u;
}
static_assert(kRefTile == RT_TILE_SIZE, "the kernels' reference tile is the header's");

int build_selection(const uint32_t *tiles, uint32_t n_tiles, uint32_t width, uint32_t height,
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

int select_tiles(const ListName &name, const uint32_t *tiles, uint32_t n_tiles, uint32_t width, uint32_t height,
                 std::vector<uint32_t> &bits, TileSelection &sel) {
    uint32_t bad = 0;
    const int v = build_selection(tiles, n_tiles, width, height, bits, sel, &bad);
    if (v == -1)
        return rt_fail(RT_EINVAL, "%s: %s%u%s = %u, the image has %u tiles", name.api, name.open, bad, name.close,
                       tiles[bad], rt_tile_count(width, height, nullptr));
    if (v == -2)
        return rt_fail(RT_EINVAL, "%s: %s%u%s = %u is listed twice", name.api, name.open, bad, name.close, tiles[bad]);
    return RT_OK;
}

int check_trace_args(bool have_device, bool lut_set, bool scene_set, const rt_camera_info *cam,
                     const rt_trace_desc *desc, const uint64_t *d_rays) {
    if (!have_device || !cam || !desc || !d_rays) return rt_fail(RT_EINVAL, "rt_trace: NULL argument");
    if (!lut_set) return rt_fail(RT_EINVAL, "rt_trace: rsqrt table not set (rt_set_rsqrt_table)");
    if (!scene_set) return rt_fail(RT_EINVAL, "rt_trace: no scene uploaded (rt_scene_upload)");
    if (desc->SeedMode != RT_SEED_PIXEL) return rt_fail(RT_EINVAL, "rt_trace: only RT_SEED_PIXEL runs on the GPU");
    if (desc->Flags & ~(RT_FLAG_ACCUM_ZERO | RT_FLAG_SRGB_POW))
        return rt_fail(RT_EINVAL, "rt_trace: unknown Flags 0x%x", desc->Flags);
    if (desc->Width == 0 || desc->Height == 0 || desc->Width > 65536 || desc->Height > 65536)
        return rt_fail(RT_EINVAL, "rt_trace: bad image size %ux%u", desc->Width, desc->Height);
    const uint32_t band_rows = desc->BandRows ? desc->BandRows : 32u;
    const uint32_t band_count = desc->BandCount ? desc->BandCount : 1u;
    if (desc->BandIndex >= band_count) return rt_fail(RT_EINVAL, "rt_trace: BandIndex >= BandCount");
    if (band_rows % 8u) return rt_fail(RT_EINVAL, "rt_trace: BandRows must be a multiple of 8");
    if ((uint64_t)desc->PreviousRayCount + desc->Frames > 0xFFFFFFFFull)
        return rt_fail(RT_EINVAL, "rt_trace: PreviousRayCount + Frames exceeds the u32 frame count");
    return RT_OK;
}

int plan_tile_work(const rt_tile_work *work, uint32_t n_work, uint32_t width, uint32_t height, TileWorkList &out) {
    // every entry's tile first, those of zero-frame entries included: a tile named twice is refused
    // before such entries are dropped
    out.tiles.resize(n_work);
    for (uint32_t i = 0; i < n_work; ++i) out.tiles[i] = work[i].Tile;
    const ListName name = {"rt_trace_tile_work", "work[", "].Tile"};
    if (const int rc = select_tiles(name, out.tiles.data(), n_work, width, height, out.bits, out.sel)) return rc;
    for (uint32_t i = 0; i < n_work; ++i)
        if ((uint64_t)work[i].PreviousRayCount + work[i].Frames > 0xFFFFFFFFull)
            return rt_fail(RT_EINVAL, "rt_trace_tile_work: work[%u]: PreviousRayCount + Frames exceeds the u32 frame count", i);
    // the kept entries (Frames > 0): their tiles, their table, whether they share one pair
    out.table.assign(2u * (size_t)out.sel.n_tiles, 0u);
    out.kept = out.max_frames = 0;
    out.uniform = true;
    for (uint32_t i = 0; i < n_work; ++i) {
        const rt_tile_work &e = work[i];
        if (e.Frames == 0u) continue;
        if (!out.kept) out.first = e;
        out.uniform = out.uniform && e.PreviousRayCount == out.first.PreviousRayCount && e.Frames == out.first.Frames;
        out.max_frames = std::max(out.max_frames, e.Frames);
        out.table[2u * (size_t)e.Tile] = e.PreviousRayCount;
        out.table[2u * (size_t)e.Tile + 1u] = e.Frames;
        out.tiles[out.kept++] = e.Tile;
    }
    uint32_t bad = 0;
    if (out.kept) (void)build_selection(out.tiles.data(), out.kept, width, height, out.bits, out.sel, &bad);
    return RT_OK;
}

int plan_tile_counts(bool have_device, bool lut_set, bool scene_set, const rt_camera_info *cam, const rt_trace_desc *desc,
                     const uint32_t *tiles, uint32_t n_tiles, const void *d_counts, uint32_t max_frames,
                     const void *d_delta, const uint64_t *d_rays, std::vector<uint32_t> &bits, TileCountsCall &out) {
    if (!desc) return rt_fail(RT_EINVAL, "rt_trace: NULL argument");
    if (!d_counts) return rt_fail(RT_EINVAL, "rt_trace_tile_counts: d_counts is NULL");
    if (max_frames == 0u) return rt_fail(RT_EINVAL, "rt_trace_tile_counts: max_frames is 0");
    if ((uintptr_t)d_delta & 15u) return rt_fail(RT_EINVAL, "rt_trace_tile_counts: d_delta is not 16-byte aligned");
    out = TileCountsCall();
    out.desc = *desc;  // (desc's own PreviousRayCount / Frames are not read: every tile has its entry)
    out.desc.PreviousRayCount = 0;
    out.desc.Frames = max_frames;
    if (const int rc = check_trace_args(have_device, lut_set, scene_set, cam, &out.desc, d_rays)) return rc;
    if (desc->BandCount > 1u || desc->BandIndex != 0u)
        return rt_fail(RT_EINVAL, "rt_trace_tile_counts: tiles index the whole image (BandCount 0 or 1, BandIndex 0)");
    if (!tiles && n_tiles) return rt_fail(RT_EINVAL, "rt_trace_tile_counts: tiles is NULL with n_tiles %u", n_tiles);
    const ListName name = {"rt_trace_tile_counts", "tiles[", "]"};
    if (const int rc = select_tiles(name, tiles, n_tiles, desc->Width, desc->Height, bits, out.sel)) return rc;
    out.nothing = n_tiles == 0u;
    return RT_OK;
}

int check_tile_step(const void *d_counts, const void *d_delta, uint32_t width, uint32_t height, const rt_tile_rule *rule,
                    uint32_t *n_tiles) {
    if (!d_counts || !d_delta || !rule) return rt_fail(RT_EINVAL, "rt_tile_counts_step: NULL argument");
    if (rule->Size != sizeof(rt_tile_rule))
        return rt_fail(RT_EINVAL, "rt_tile_rule: Size %u, this library's is %zu", rule->Size, sizeof(rt_tile_rule));
    if (rule->MaxRoundFrames == 0u || rule->MaxTileFrames == 0u)
        return rt_fail(RT_EINVAL, "rt_tile_rule: MaxRoundFrames %u, MaxTileFrames %u (both >= 1)", rule->MaxRoundFrames,
                       rule->MaxTileFrames);
    if ((uintptr_t)d_delta & 15u) return rt_fail(RT_EINVAL, "rt_tile_counts_step: d_delta is not 16-byte aligned");
    *n_tiles = rt_tile_count(width, height, nullptr);
    if (*n_tiles == 0u) return rt_fail(RT_EINVAL, "rt_tile_counts_step: bad image size %ux%u", width, height);
    return RT_OK;
}

int plan_first_hit(bool have_device, bool scene_set, const rt_camera_info *cam, const rt_trace_desc *desc,
                   const uint32_t *tiles, uint32_t n_tiles, uint32_t flags, const rt_first_hit_planes *out,
                   std::vector<uint32_t> &bits, FirstHitCall &call) {
    if (!have_device || !cam || !desc || !out) return rt_fail(RT_EINVAL, "rt_trace_first_hit: NULL argument");
    if (out->Size != sizeof(rt_first_hit_planes))
        return rt_fail(RT_EINVAL, "rt_first_hit_planes: Size %u, this library's is %zu", out->Size, sizeof(rt_first_hit_planes));
    if (!out->Hit && !out->Normal && !out->Albedo) return rt_fail(RT_EINVAL, "rt_trace_first_hit: every plane is NULL");
    if ((uintptr_t)out->Hit & 7u) return rt_fail(RT_EINVAL, "rt_trace_first_hit: Hit is not 8-byte aligned");
    if ((uintptr_t)out->Normal & 15u) return rt_fail(RT_EINVAL, "rt_trace_first_hit: Normal is not 16-byte aligned");
    if ((uintptr_t)out->Albedo & 15u) return rt_fail(RT_EINVAL, "rt_trace_first_hit: Albedo is not 16-byte aligned");
    if (flags & ~RT_HIT_PIXEL_CENTRE) return rt_fail(RT_EINVAL, "rt_trace_first_hit: unknown flags 0x%x", flags);
    if (desc->SeedMode != RT_SEED_PIXEL) return rt_fail(RT_EINVAL, "rt_trace_first_hit: only RT_SEED_PIXEL runs on the GPU");
    if (desc->BandCount > 1u || desc->BandIndex != 0u)
        return rt_fail(RT_EINVAL, "rt_trace_first_hit: the planes are whole images (BandCount 0 or 1, BandIndex 0)");
    if (rt_tile_count(desc->Width, desc->Height, nullptr) == 0u)
        return rt_fail(RT_EINVAL, "rt_trace_first_hit: bad image size %ux%u", desc->Width, desc->Height);
    if (!scene_set) return rt_fail(RT_EINVAL, "rt_trace_first_hit: no scene uploaded (rt_scene_upload)");
    if (!tiles && n_tiles) return rt_fail(RT_EINVAL, "rt_trace_first_hit: tiles is NULL with n_tiles %u", n_tiles);
    call = FirstHitCall();
    const ListName name = {"rt_trace_first_hit", "tiles[", "]"};
    // (a refused list has been written into `bits` up to the index refused: scratch of this pass alone, rebuilt by
    // every call before anything reads it, so nothing a later call or the launch key sees has changed)
    if (const int rc = select_tiles(name, tiles, n_tiles, desc->Width, desc->Height, bits, call.sel)) return rc;
    call.all = tiles == nullptr;
    call.nothing = !call.all && n_tiles == 0u;
    return RT_OK;
}

int plan_denoise(const rt_denoise_desc *d, DenoisePlan &plan) {
    if (!d) return rt_fail(RT_EINVAL, "rt_denoise: NULL argument");
    if (d->Size != sizeof(rt_denoise_desc))
        return rt_fail(RT_EINVAL, "rt_denoise_desc: Size %u, this library's is %zu", d->Size, sizeof(rt_denoise_desc));
    if (rt_tile_count(d->Width, d->Height, nullptr) == 0u)
        return rt_fail(RT_EINVAL, "rt_denoise: bad image size %ux%u", d->Width, d->Height);
    if (d->Iterations < 1u || d->Iterations > RT_DENOISE_MAX_ITERATIONS)
        return rt_fail(RT_EINVAL, "rt_denoise: Iterations %u (1..%u)", d->Iterations, RT_DENOISE_MAX_ITERATIONS);
    if (d->Flags & ~(RT_DENOISE_DEMODULATE | RT_DENOISE_SRGB_POW))
        return rt_fail(RT_EINVAL, "rt_denoise: unknown flags 0x%x", d->Flags);
    if (d->NormalPower > 8u) return rt_fail(RT_EINVAL, "rt_denoise: NormalPower %u (0..8)", d->NormalPower);
    // (a NaN fails the first comparison, an infinity the second)
    if (!(d->SigmaDepth >= 0.0f && d->SigmaDepth <= 3.402823466e+38f))
        return rt_fail(RT_EINVAL, "rt_denoise: SigmaDepth is negative, NaN or infinite");
    if (!(d->SigmaColor >= 0.0f && d->SigmaColor <= 3.402823466e+38f))
        return rt_fail(RT_EINVAL, "rt_denoise: SigmaColor is negative, NaN or infinite");
    if (!d->Mean) return rt_fail(RT_EINVAL, "rt_denoise: Mean is NULL");
    if (!d->Hit) return rt_fail(RT_EINVAL, "rt_denoise: Hit is NULL");
    if (!d->Out) return rt_fail(RT_EINVAL, "rt_denoise: Out is NULL");
    if (!d->Normal && d->NormalPower != 0u)
        return rt_fail(RT_EINVAL, "rt_denoise: Normal is NULL with NormalPower %u", d->NormalPower);
    if (!d->Albedo && (d->Flags & RT_DENOISE_DEMODULATE))
        return rt_fail(RT_EINVAL, "rt_denoise: Albedo is NULL with RT_DENOISE_DEMODULATE");
    if (!d->Scratch && d->Iterations >= 2u)
        return rt_fail(RT_EINVAL, "rt_denoise: Scratch is NULL with Iterations %u", d->Iterations);
    const struct {
        const void *p;
        uintptr_t mask;
        const char *name;
    } planes[] = {{d->Mean, 15u, "Mean"}, {d->Hit, 7u, "Hit"},          {d->Normal, 15u, "Normal"}, {d->Albedo, 15u, "Albedo"},
                  {d->Out, 15u, "Out"},   {d->Scratch, 15u, "Scratch"}, {d->Rgba8, 3u, "Rgba8"}};
    for (const auto &pl : planes)
        if ((uintptr_t)pl.p & pl.mask)
            return rt_fail(RT_EINVAL, "rt_denoise: %s is not %u-byte aligned", pl.name, (unsigned)pl.mask + 1u);
    if ((const float *)d->Out == d->Mean)
        return rt_fail(RT_EINVAL, "rt_denoise: Out is Mean (the filter does not run in place)");
    // (a Scratch the call never touches is compared all the same: one rule for every Iterations)
    if (d->Scratch && (const float *)d->Scratch == d->Mean) return rt_fail(RT_EINVAL, "rt_denoise: Scratch is Mean");
    if (d->Scratch && d->Scratch == d->Out) return rt_fail(RT_EINVAL, "rt_denoise: Scratch is Out");
    plan = DenoisePlan();
    plan.n_passes = d->Iterations;
    plan.ic0 = d->SigmaColor > 0.0f ? 1.0f / d->SigmaColor : 0.0f;
    const float *src = d->Mean;
    for (uint32_t i = 0; i < plan.n_passes; ++i) {
        DenoisePass &p = plan.pass[i];
        p.src = src;
        p.dst = ((plan.n_passes - 1u - i) & 1u) ? d->Scratch : d->Out;  // the last pass writes Out
        p.step = 1u << i;
        p.ic = plan.ic0 * (float)p.step;
        src = p.dst;
    }
    return RT_OK;
}

int plan_reproject(const rt_reproject_desc *d, ReprojectArgs &args) {
    if (!d) return rt_fail(RT_EINVAL, "rt_reproject: NULL argument");
    if (d->Size != sizeof(rt_reproject_desc))
        return rt_fail(RT_EINVAL, "rt_reproject_desc: Size %u, this library's is %zu", d->Size, sizeof(rt_reproject_desc));
    if (rt_tile_count(d->Width, d->Height, nullptr) == 0u)
        return rt_fail(RT_EINVAL, "rt_reproject: bad image size %ux%u", d->Width, d->Height);
    if (d->Frames == 0u) return rt_fail(RT_EINVAL, "rt_reproject: Frames is 0");
    if (d->MaxHistory < d->Frames)
        return rt_fail(RT_EINVAL, "rt_reproject: MaxHistory %u is below Frames %u", d->MaxHistory, d->Frames);
    if (d->Flags & ~RT_REPROJECT_SRGB_POW) return rt_fail(RT_EINVAL, "rt_reproject: unknown flags 0x%x", d->Flags);
    // (a NaN fails the first comparison, an infinity the second)
    if (!(d->DepthTolerance >= 0.0f && d->DepthTolerance <= 3.402823466e+38f))
        return rt_fail(RT_EINVAL, "rt_reproject: DepthTolerance is negative, NaN or infinite");
    const struct {
        const void *p;
        uintptr_t mask;
        const char *name;
        bool required;
    } planes[] = {{d->Camera, 0u, "Camera", true},
                  {d->PreviousCamera, 0u, "PreviousCamera", true},
                  {d->Mean, 15u, "Mean", true},
                  {d->Hit, 7u, "Hit", true},
                  {d->Out, 15u, "Out", true},
                  {d->OutCount, 3u, "OutCount", true},
                  {d->History, 15u, "History", false},
                  {d->HistoryHit, 7u, "HistoryHit", false},
                  {d->HistoryCount, 3u, "HistoryCount", false},
                  {d->Rgba8, 3u, "Rgba8", false}};
    for (const auto &pl : planes)
        if (pl.required && !pl.p) return rt_fail(RT_EINVAL, "rt_reproject: %s is NULL", pl.name);
    if ((d->History != nullptr) != (d->HistoryHit != nullptr) || (d->History != nullptr) != (d->HistoryCount != nullptr))
        return rt_fail(RT_EINVAL, "rt_reproject: History, HistoryHit and HistoryCount must be all NULL or all given");
    for (const auto &pl : planes)
        if ((uintptr_t)pl.p & pl.mask)
            return rt_fail(RT_EINVAL, "rt_reproject: %s is not %u-byte aligned", pl.name, (unsigned)pl.mask + 1u);
    if ((const float *)d->Out == d->Mean)
        return rt_fail(RT_EINVAL, "rt_reproject: Out is Mean (the pass does not run in place)");
    if ((const float *)d->Out == d->History)
        return rt_fail(RT_EINVAL, "rt_reproject: Out is History (the pass does not run in place)");
    if ((const uint32_t *)d->OutCount == d->HistoryCount)
        return rt_fail(RT_EINVAL, "rt_reproject: OutCount is HistoryCount (the pass does not run in place)");
    ReprojectArgs a;
    memset(&a, 0, sizeof(a));
    a.mean = d->Mean;
    a.hit = d->Hit;
    a.history = d->History;
    a.history_hit = d->HistoryHit;
    a.history_count = d->HistoryCount;
    a.out = d->Out;
    a.out_count = d->OutCount;
    a.rgba8 = d->Rgba8;
    a.width = d->Width;
    a.height = d->Height;
    a.frames = d->Frames;
    a.max_history = d->MaxHistory;
    a.depth_tolerance = d->DepthTolerance > 0.0f ? d->DepthTolerance : 0.0f;  // (-0.0f is off, like +0.0f)
    a.srgb_pow = (d->Flags & RT_REPROJECT_SRGB_POW) ? 1u : 0u;
    const rt_camera_info &c = *d->Camera, &p = *d->PreviousCamera;
    const float cur[4][3] = {{c.CameraPosition.x, c.CameraPosition.y, c.CameraPosition.z},
                             {c.CameraX.x, c.CameraX.y, c.CameraX.z},
                             {c.CameraY.x, c.CameraY.y, c.CameraY.z},
                             {c.FilmCenter.x, c.FilmCenter.y, c.FilmCenter.z}};
    const float prev[4][3] = {{p.CameraPosition.x, p.CameraPosition.y, p.CameraPosition.z},
                              {p.CameraX.x, p.CameraX.y, p.CameraX.z},
                              {p.CameraY.x, p.CameraY.y, p.CameraY.z},
                              {p.FilmCenter.x, p.FilmCenter.y, p.FilmCenter.z}};
    for (int i = 0; i < 3; ++i) {
        a.cam_pos[i] = cur[0][i];
        a.cam_x[i] = cur[1][i];
        a.cam_y[i] = cur[2][i];
        a.film_center[i] = cur[3][i];
        a.prev_pos[i] = prev[0][i];
        a.prev_x[i] = prev[1][i];
        a.prev_y[i] = prev[2][i];
        a.fv[i] = prev[3][i] - prev[0][i];
    }
    a.film_w = c.FilmW;
    a.film_h = c.FilmH;
    a.prev_film_w = p.FilmW;
    a.prev_film_h = p.FilmH;
    // dot3: each product and each sum rounds on its own (this unit is built with -ffp-contract=off)
    const float fx2 = a.fv[0] * a.fv[0], fy2 = a.fv[1] * a.fv[1], fz2 = a.fv[2] * a.fv[2];
    a.ff = (fx2 + fy2) + fz2;
    a.wf = (float)d->Width;
    a.hf = (float)d->Height;
    a.hw = a.wf * 0.5f;
    a.hh = a.hf * 0.5f;
    args = a;
    return RT_OK;
}

int plan_reproject_clip(const rt_reproject_clip_desc *d, ReprojectClipArgs &args) {
    if (!d) return rt_fail(RT_EINVAL, "rt_reproject_clip: NULL argument");
    if (d->Size != sizeof(rt_reproject_clip_desc))
        return rt_fail(RT_EINVAL, "rt_reproject_clip_desc: Size %u, this library's is %zu", d->Size,
                       sizeof(rt_reproject_clip_desc));
    if (d->Radius < 1u || d->Radius > 3u) return rt_fail(RT_EINVAL, "rt_reproject_clip: Radius %u is not in 1..3", d->Radius);
    // (a NaN fails the first comparison, an infinity the second)
    if (!(d->Gamma > 0.0f && d->Gamma <= 3.402823466e+38f))
        return rt_fail(RT_EINVAL, "rt_reproject_clip: Gamma is not a finite number above 0");
    ReprojectClipArgs c;
    memset(&c, 0, sizeof(c));
    if (const int rc = plan_reproject(&d->Reproject, c.rp)) return rc;
    c.radius = d->Radius;
    c.gamma = d->Gamma;
    args = c;
    return RT_OK;
}

// The key: every word the cull masks, the live list and the learned order depend on.
static void launch_key(const LaunchPlan &p, const SceneFacts &sf, int rs, const rt_trace_desc &desc,
                       const TileSelection *sel, const TraceArgs &a, std::vector<uint32_t> &key) {
    key.clear();
    for (const uint32_t w : {desc.Width, desc.Height, a.local_rows, a.band_rows, a.band_count, desc.BandIndex,
                             (uint32_t)p.lpp, (uint32_t)rs, (uint32_t)p.cull, (uint32_t)p.empty_capable,
                             (uint32_t)p.sched, p.interleave, p.unit_waves, (uint32_t)sf.scene_gen,
                             (uint32_t)(sf.scene_gen >> 32)})
        key.push_back(w);
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
}

// The LDS image and the kernel: which tables and whether the scene go into the image, one wave or
// four per workgroup, the walk and the table it reads.
static void route_kernel(const Switches &sw, const SceneFacts &sf, int lpp, bool counts, const TablePointers &tables,
                         TraceArgs &a, LaunchPlan &p) {
    // The rsqrt and fold tables (10 KB) leave the LDS image at P = 16, whose 4-wave
    // ring (10 KB) would otherwise cap a CU at 6 blocks: measured on the 8-rank C2
    // share 0.900-0.903 against 0.914-0.922 ms; at P = 4 they stay (C2 -1.8 % without)
    const bool in_lds = !sw.tables_global && lpp <= 8;
    a.lut_in_lds = rtk_lut_in_lds(a.n_groups) && in_lds ? 1u : 0u;
    a.fold_in_lds = rtk_fold_in_lds(a.n_groups) && in_lds ? 1u : 0u;
    a.scene_in_lds = a.n_groups <= kMaxLdsGroups && !sw.scene_global ? 1u : 0u;
    if (sw.solo && sw.src == kSrcSmem) {  // one-wave workgroups keep no LDS image
        a.solo = 1u;
        a.lut_in_lds = a.fold_in_lds = a.scene_in_lds = 0u;
        // the walk-specialised kernel this launch asks for, or the run-time one (rt_kernel.h, the routing
        // rule: a.clusters is set only with n_cpairs >= 1, and rt_trace returns before the plan at Frames == 0)
        a.walk = rtk_walk_request(a, sw.walk_any != 0);
        // The expanded table goes to the kernels that hold the expanded prefilter, and to no other (rt_kernel.h
        // kPrefilterExpanded): offered here, and taken back unless this launch's kernel is one of them.
        if (a.clusters && !a.pf_relative && sf.clusters_x_ok && !sw.walk_any) {
            a.clusters = tables.expanded;  // (the row {c0, 0}, then entry 0)
            // (with the direction block behind it where the upload built one: rtk_walk_kernel decides the rest)
            const bool dir = sf.dir_table && (sw.dir_table == 2 || rtk_direction_default(lpp));
            a.prefilter = dir ? kPrefilterDirection : kPrefilterExpanded;
            p.table = kTableExpanded;
            a.walk = rtk_walk_request(a, false);
            if (!rtk_walk_expanded(a, sw.cull != 0, lpp)) {
                // (a shape or a device without walk kernels: the request stands, as it always did for such a
                // launch, and rtk_walk_kernel gives it the run-time kernel, now for want of the expanded table too)
                a.clusters = tables.plain;
                a.prefilter = kPrefilterOn;
                p.table = kTablePlain;
            }
        }
    }
    p.src = a.scene_in_lds ? sw.src : kSrcSmem;  // a scene in HBM is read through the scalar cache
    if (counts && !a.solo && !rtk_tile_counts_four_wave(a.scene_in_lds, p.src)) {
        // a four-wave launch whose kernel is not built with per-tile counts (SphereSourceLds, SceneInHbm,
        // a scene beyond the LDS image): the one-wave run-time kernel, reported as such (rt_trace_info)
        a.solo = 1u;
        a.lut_in_lds = a.fold_in_lds = a.scene_in_lds = 0u;
        a.walk = kWalkAny;
    }
}

LaunchPlan plan_launch(const Switches &sw, const SceneFacts &sf, int rs, uint32_t cu_count, const rt_trace_desc &desc,
                       uint32_t local_rows, const TileSelection *sel, bool counts, bool delta,
                       const TablePointers &tables, TraceArgs &a, std::vector<uint32_t> &key) {
    LaunchPlan p;
    a.n_groups = sf.n_groups;
    a.n_spheres = sf.n_spheres;
    a.use_sky = sf.use_sky ? 1u : 0u;
    a.prefilter = sf.prefilter;
    a.pf_relative = sf.pf_relative;
    a.fast_sqrt = sf.fast_sqrt;
    a.clusters = nullptr;
    a.n_cpairs = a.cl_words = 0u;
    if (a.prefilter && sf.n_cpairs && (sw.clusters == 2 || (sw.clusters == 1 && sf.n_groups <= kClAutoGroups))) {
        a.clusters = tables.plain;
        a.n_cpairs = sf.n_cpairs;
        a.cl_words = sf.cl_words;
        p.table = kTablePlain;
    }
    // Lanes that must wait before a secondary round runs: the dearer a wave's
    // secondary round (cluster pairs, or groups without clusters), the more it
    // pays to fill it first.  Measured (same box, Mrays/s, threshold 16/32/40/48):
    // RTWeekend (20 cluster pairs) 18.6k/19.4k/19.5k/19.5k, C5 at 512 spp (16)
    // 44.7k/46.3k/46.4k/46.4k, C2 (5) 153.8k/151.2k/150.4k/149.9k.  Round 4 (in-pixel
    // sample hand-out, 40/44/48/52): RTWeekend (per-lane thresholds) 25.61k/25.73k/25.74k/
    // 25.71k, C5 (scene-wide) 52.74k/52.44k/52.58k/52.38k: 48 for per-lane walks.
    a.merge_rounds = sw.merge == 1 || (sw.merge == -1 && sf.n_groups <= kMergeGroups) ? 1u : 0u;
    // Round 5 (primary table, steady state): 24 for the small walks, against 16 / 32: C2 +1.2 %, C3 +1.0 %, the
    // 4-rank share -2.7 %, the 8-rank share -0.8 % (profiles/r05r_sec_threshold_ab.txt).
    // (never 0 in the kernel, whose round decision compares the count of secondary lanes against it: round_select)
    a.sec_threshold = sw.sec_threshold;
    if (a.sec_threshold == 0)
        a.sec_threshold = (a.clusters ? a.n_cpairs : a.n_groups) >= 12u ? (a.pf_relative ? 48u : 40u) : 24u;
    // Lanes per pixel (measured on MI355X at 1/2/4/8-way band splits of C2,
    // bench.py --sim-ranks, heaviest-first order at every P): 4 while the band
    // has >= 6k pixels per CU, 8 down to 3k, else 16 (round 4, with the in-pixel
    // sample hand-out: the 4-rank share 1.19-1.23 ms at P = 16 against 1.25-1.28
    // at P = 8; the 2-rank share 2.26-2.27 at P = 8, 2.29 at P = 16; more lanes per pixel
    // shorten the per-lane sample chains that form the launch tail; C2 rank
    // shares: 1 GPU P=4 6.21 ms (P=8 6.29, P=16 6.62); 2 ranks P=8 3.26 ms
    // (P=4 3.35); 4 ranks P=8 = P=16 1.81 ms; 8 ranks P=16 1.02 ms (P=8
    // 1.47)); never more lanes than frames.
    int lpp = sw.lanes_per_pixel;
    const bool auto_lpp = lpp == 0;
    if (lpp == 0) {
        // (a tile list: the pixels it covers -- a small window is a small launch, like a small rank share)
        const uint64_t pixels = sel ? sel->pixels : (uint64_t)desc.Width * local_rows;
        lpp = pixels >= (uint64_t)cu_count * 6144u ? 4 : pixels >= (uint64_t)cu_count * 3072u ? 8 : 16;
        while (lpp > 1 && (uint32_t)lpp / 2u >= desc.Frames) lpp /= 2;
    }
    // One lane per pixel, and one frame (the reference's OnRender unit): each lane
    // takes kPixelsPerLane pixels in turn (launch shape 0, rtk_shape.h Shape<0>),
    // so a wave stays full after its first pass and the launch has a quarter of
    // the waves.  Measured on the 1080p OnRender frame: see DESIGN.md §6a.
    p.pixels_per_lane = lpp == 1 && !(desc.Flags & RT_FLAG_SRGB_POW) &&
                                (sw.pixels_per_lane == 4 || (sw.pixels_per_lane == 0 && auto_lpp && desc.Frames == 1))
                            ? 4u : 1u;
    p.lanes = (uint32_t)lpp;
    if (p.pixels_per_lane > 1) lpp = 0;
    p.lpp = lpp;
    a.interleave = sw.interleave && lpp >= 2 ? 1u : 0u;
    route_kernel(sw, sf, lpp, counts, tables, a, p);
    // Tile scheduling.  Block tiles (2TW x 2TH pixels) are traced in the order
    // tile_order[0 .. n_live): with culling, the cull pass (once per camera /
    // scene / geometry) writes every wave tile's primary group mask and a
    // live-first order, and dead tiles (no candidate group anywhere, no sky)
    // never reach the trace kernel -- rtk_launch_empty folds their pixels.
    // With heaviest-first scheduling each launch also measures its tiles and
    // re-sorts them for the next launch (live tiles keep costs > 0, dead ones
    // 0, so the live prefix is preserved).
    p.n_tiles = rtk_tile_count(desc.Width, local_rows, lpp);
    // Units of the heaviest-first order: waves for the one-wave kernels (each wave
    // its own workgroup, so each is placed by its own cost), block tiles otherwise
    a.unit_waves = a.solo && sw.wave_order ? 1u : 0u;
    p.n_units = a.unit_waves ? 4u * p.n_tiles : p.n_tiles;
    p.n_words = rtk_mask_words(a.n_groups);
    p.mask_words = (size_t)p.n_tiles * 4u * p.n_words;
    p.cull = sw.cull != 0;
    p.empty_capable = p.cull && !sf.use_sky && desc.MaxBounce != 0;
    p.sched = sw.tile_sched != 0;
    a.tiles_x = rtk_tiles_x(desc.Width, lpp);
    p.n_selected = sel ? sel->block_tiles(lpp) : p.n_tiles;
    // pixels dealt to waves by cost (options PixelSort): block tiles of at most 64 pixels
    p.pixel_sort = sw.pixel_sort && p.sched && lpp >= 4 && !a.interleave;
    // one-wave kernels: sort, then group each block tile's waves onto one XCD
    p.xcd_group = a.unit_waves && (sw.xcd_group == 1 || (sw.xcd_group < 0 && lpp <= 4));
    // (multi-frame launches only: a one-frame launch, OnRender's, keeps its store and one kernel fewer)
    // (the statistics need the old bytes: no kernel before the closing pass may store RGBA8, at any shape)
    // (for the trace launches and what follows them: a new key's cull or select pass runs before it is set)
    p.skip_cur = (sw.cur_pass && lpp >= 2) || delta ? 1u : 0u;
    p.interleave = a.interleave;
    p.lut_in_lds = a.lut_in_lds;
    p.fold_in_lds = a.fold_in_lds;
    p.scene_in_lds = a.scene_in_lds;
    p.solo = a.solo;
    p.walk = a.walk;
    p.prefilter = a.prefilter;
    p.merge_rounds = a.merge_rounds;
    p.sec_threshold = a.sec_threshold;
    p.unit_waves = a.unit_waves;
    p.tiles_x = a.tiles_x;
    launch_key(p, sf, rs, desc, sel, a, key);
    return p;
}

SplitSchedule split_schedule(uint32_t frames, uint32_t lanes, uint32_t head_samples, uint32_t split_parts,
                             uint32_t split_growth, bool may_split) {
    // The first launch of a key has no measured tile costs, and in the cull
    // pass's live-first order its heavy tiles start late and form the tail
    // (C2 cold 7.7 ms against 5.4 warm).  A long launch is therefore split:
    // its first head_samples samples per lane (1/8 of C2's work) run in that
    // order and measure the tile costs, and the remaining frames continue the
    // running mean heaviest-first.  Splitting a launch at a frame boundary
    // changes no bit: the owner lane folds frames in order either way, and
    // frame k's seed and weights depend on PreviousRayCount + k only.
    SplitSchedule s;
    const uint32_t split_min = 4u * head_samples * lanes;
    if (may_split && frames >= split_min) {
        // leading parts of head_samples, x split_growth, ... samples per lane
        // while the rest keeps at least half the frames
        uint32_t f = head_samples * lanes;
        // (f != 0: an extreme SplitGrowth wraps the product; no part of a launch is empty)
        for (uint32_t i = 0; i + 1 < split_parts && f != 0 && s.head_frames + f <= frames / 2u; ++i) {
            s.parts[s.n_parts++] = f;
            s.head_frames += f;
            f *= split_growth;
        }
    }
    s.parts[s.n_parts++] = frames - s.head_frames;
    return s;
}
