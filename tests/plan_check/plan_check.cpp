// plan_check.cpp — the launch decisions (csrc/rt_plan.cpp) as a plain host program: no HIP library, no device.
// Links csrc/rt_plan.cpp only.  Every case is one rule of the plan at the smallest input where it can
// go wrong; the program prints one line per case, "section/case : value", and compares the value with
// the literal the case states (exit status 1 and a line on stderr where they differ).  Built with a host
// sanitizer (tests/test_plan_standalone.py) the run also checks every index the selection code forms.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "rt_plan.h"
#include "rtk_shape.h"

static char g_err[512];
// the library's is in rt_host.cpp, beside the error text it sets
int rt_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace {

int g_bad = 0;

void expect(const std::string &name, long long got, long long want) {
    printf("%s : %lld\n", name.c_str(), got);
    if (got != want) {
        fprintf(stderr, "plan_check: %s: got %lld, expected %lld\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

void expect_text(const std::string &name, const char *got, const char *want) {
    printf("%s : %s\n", name.c_str(), got);
    if (strcmp(got, want)) {
        fprintf(stderr, "plan_check: %s: got \"%s\", expected \"%s\"\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

std::string list_of(const uint32_t *v, uint32_t n) {
    std::string s;
    for (uint32_t i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

const float4 kPlain[1] = {}, kExpanded[1] = {};  // stand-ins for the two device tables: only their identity matters

// One launch's inputs.  The defaults: a one-CU device at its default options, a 16-group scene with a
// scene-wide one-word cluster table whose expanded table is in use, a 64 x 48 image, 256 frames, 8 bounces.
struct In {
    Switches sw;
    SceneFacts sf;
    int rs = 0;
    uint32_t cu = 1;
    rt_trace_desc desc;
    uint32_t local_rows = 48;
    const TileSelection *sel = nullptr;
    bool counts = false, delta = false;
    float cam[14];
    In() {
        sf.n_groups = 16;
        sf.prefilter = 1;
        sf.fast_sqrt = 1;
        sf.n_cpairs = 5;
        sf.cl_words = 1;
        sf.clusters_x_ok = true;
        sf.n_spheres = 64;
        sf.scene_gen = 1;
        memset(&desc, 0, sizeof(desc));
        desc.Width = 64;
        desc.Height = 48;
        desc.Frames = 256;
        desc.MaxBounce = 8;
        desc.EnableSIMD = 1;
        desc.SeedMode = RT_SEED_PIXEL;
        for (int i = 0; i < 14; ++i) cam[i] = 1.0f + (float)i;
    }
    void size(uint32_t w, uint32_t h) {
        desc.Width = w;
        desc.Height = local_rows = h;
    }
};

struct Out {
    LaunchPlan p;
    TraceArgs a;
    std::vector<uint32_t> key;
};

// (what rt_host.cpp fill_args hands to the plan: the descriptor and the camera)
Out plan(const In &in) {
    Out o;
    TraceArgs &a = o.a;
    memset(&a, 0, sizeof(a));
    float *dst[4] = {a.cam_pos, a.cam_x, a.cam_y, a.film_center};
    for (int i = 0; i < 12; ++i) dst[i / 3][i % 3] = in.cam[i];
    a.film_w = in.cam[12];
    a.film_h = in.cam[13];
    a.width = in.desc.Width;
    a.height = in.desc.Height;
    a.local_rows = in.local_rows;
    a.prev_count = in.desc.PreviousRayCount;
    a.frames = in.desc.Frames;
    a.max_bounce = in.desc.MaxBounce;
    a.band_rows = in.desc.BandRows ? in.desc.BandRows : 32u;
    a.band_count = in.desc.BandCount ? in.desc.BandCount : 1u;
    a.band_index = in.desc.BandIndex;
    o.key.assign(3, 0xDEADu);  // (the plan clears what the vector held)
    o.p = plan_launch(in.sw, in.sf, in.rs, in.cu, in.desc, in.local_rows, in.sel, in.counts, in.delta,
                      TablePointers{kPlain, kExpanded}, a, o.key);
    return o;
}

const int kShapes[7] = {0, 1, 2, 4, 8, 16, 32};

template <int P>
void shape_case() {
    const uint32_t bw = 2u * rtk::Shape<P>::TW, bh = 2u * rtk::Shape<P>::TH;
    const std::string n = "shape/p" + std::to_string(P);
    expect(n + "_one_tile", rtk_tile_count(bw, bh, P), 1);
    expect(n + "_ragged", rtk_tile_count(bw + 1u, bh + 1u, P), 4);
    expect(n + "_tiles_x", rtk_tiles_x(3u * bw, P), 3);
}

void lanes_cases() {
    const struct {
        uint32_t w, h, lanes;
    } by_pixels[] = {{96, 64, 4}, {6143, 1, 8}, {64, 48, 8}, {3071, 1, 16}};
    for (const auto &c : by_pixels) {
        In in;
        in.size(c.w, c.h);
        expect("lanes/pixels" + std::to_string(c.w * c.h), plan(in).p.lanes, c.lanes);
    }
    const uint32_t by_frames[][2] = {{1, 1}, {2, 2}, {3, 4}, {4, 4}, {5, 8}, {9, 16}};
    for (const auto &c : by_frames) {
        In in;
        in.size(3071, 1);
        in.desc.Frames = c[0];
        in.sw.pixels_per_lane = 1;
        expect("lanes/frames" + std::to_string(c[0]), plan(in).p.lanes, c[1]);
    }
    // a tile list: the list's clipped pixels (one 32 x 32 tile), not the image's 6144
    In in;
    in.size(96, 64);
    std::vector<uint32_t> bits;
    TileSelection sel;
    uint32_t bad = 0, tile = 0;
    expect("lanes/list_valid", build_selection(&tile, 1, 96, 64, bits, sel, &bad), 0);
    in.sel = &sel;
    expect("lanes/list_pixels1024", plan(in).p.lanes, 16);
    in.sw.lanes_per_pixel = 2;
    expect("lanes/forced2", plan(in).p.lanes, 2);
}

void pixels_per_lane_cases() {
    In in;
    in.desc.Frames = 1;
    Out o = plan(in);
    expect("ppl/auto_one_frame", o.p.pixels_per_lane, 4);
    expect("ppl/auto_one_frame_shape_code", o.p.lpp, 0);
    expect("ppl/auto_one_frame_lanes", o.p.lanes, 1);
    in.desc.Flags = RT_FLAG_SRGB_POW;
    expect("ppl/srgb_pow", plan(in).p.pixels_per_lane, 1);
    in.desc.Flags = 0;
    in.sw.pixels_per_lane = 1;
    o = plan(in);
    expect("ppl/option1", o.p.pixels_per_lane, 1);
    expect("ppl/option1_shape_code", o.p.lpp, 1);
    in.sw.pixels_per_lane = 0;
    in.sw.lanes_per_pixel = 1;
    expect("ppl/forced_lanes1_option0", plan(in).p.pixels_per_lane, 1);
    in.sw.pixels_per_lane = 4;
    in.desc.Frames = 256;
    o = plan(in);
    expect("ppl/option4_forced_lanes1", o.p.pixels_per_lane, 4);
    expect("ppl/option4_shape_code", o.p.lpp, 0);
    in.sw.lanes_per_pixel = 2;
    expect("ppl/option4_lanes2", plan(in).p.pixels_per_lane, 1);
    in.sw.lanes_per_pixel = 0;
    in.sw.pixels_per_lane = 0;
    in.desc.Frames = 2;
    expect("ppl/auto_two_frames", plan(in).p.pixels_per_lane, 1);
}

void threshold_cases() {
    In in;
    in.sf.n_cpairs = 11;
    expect("sec/cpairs11", plan(in).a.sec_threshold, 24);
    in.sf.n_cpairs = 12;
    expect("sec/cpairs12", plan(in).a.sec_threshold, 40);
    in.sf.pf_relative = 1;
    expect("sec/cpairs12_per_lane", plan(in).a.sec_threshold, 48);
    in.sf.pf_relative = 0;
    in.sw.clusters = 0;  // no clustered table: the units are groups
    in.sf.n_groups = 11;
    expect("sec/groups11", plan(in).a.sec_threshold, 24);
    in.sf.n_groups = 12;
    expect("sec/groups12", plan(in).a.sec_threshold, 40);
    in.sw.sec_threshold = 16;
    expect("sec/option16", plan(in).a.sec_threshold, 16);
    in.sf.n_groups = 0;
    in.sw.sec_threshold = 0;
    const Out o = plan(in);
    expect("sec/never_zero", o.a.sec_threshold, 24);
    expect("sec/plan_holds_it", o.p.sec_threshold, 24);
}

void merge_cases() {
    In in;
    in.sf.n_groups = 2;
    expect("merge/auto_groups2", plan(in).a.merge_rounds, 1);
    in.sw.merge = 0;
    expect("merge/off_groups2", plan(in).a.merge_rounds, 0);
    in.sf.n_groups = 3;
    in.sw.merge = -1;
    expect("merge/auto_groups3", plan(in).a.merge_rounds, 0);
    in.sw.merge = 1;
    expect("merge/on_groups3", plan(in).a.merge_rounds, 1);
}

void table_cases() {
    In in;
    in.sf.clusters_x_ok = false;
    expect("table/default", plan(in).p.table, kTablePlain);
    in.sf.prefilter = 0;
    expect("table/prefilter_off", plan(in).p.table, kTableNone);
    in.sf.prefilter = 1;
    in.sf.n_cpairs = 0;
    const Out none = plan(in);
    expect("table/no_cpairs", none.p.table, kTableNone);
    expect("table/no_cpairs_pointer", none.a.clusters == nullptr, 1);
    in.sf.n_cpairs = 1;
    const Out one = plan(in);
    expect("table/one_cpair", one.p.table, kTablePlain);
    expect("table/one_cpair_pointer", one.a.clusters == kPlain, 1);
    in.sw.clusters = 0;
    expect("table/clusters_off", plan(in).p.table, kTableNone);
    in.sw.clusters = 1;
    in.sf.n_groups = kClAutoGroups;
    expect("table/auto_at_limit", plan(in).p.table, kTablePlain);
    in.sf.n_groups = kClAutoGroups + 1u;
    expect("table/auto_past_limit", plan(in).p.table, kTableNone);
    in.sw.clusters = 2;
    expect("table/on_past_limit", plan(in).p.table, kTablePlain);
}

void lds_cases() {
    In in;
    in.sw.lanes_per_pixel = 8;
    Out o = plan(in);
    expect("lds/one_wave_no_image", o.a.lut_in_lds + o.a.fold_in_lds + o.a.scene_in_lds, 0);
    in.sw.solo = 0;
    in.sf.n_groups = 32;
    o = plan(in);
    expect("lds/groups32_lanes8_lut", o.a.lut_in_lds, 1);
    expect("lds/groups32_lanes8_fold", o.a.fold_in_lds, 1);
    expect("lds/groups32_four_waves", o.a.solo, 0);
    in.sf.n_groups = 33;
    o = plan(in);
    expect("lds/groups33_lut", o.a.lut_in_lds, 0);
    expect("lds/groups33_fold", o.a.fold_in_lds, 0);
    expect("lds/groups33_scene", o.a.scene_in_lds, 1);
    in.sf.n_groups = 32;
    in.sw.lanes_per_pixel = 16;
    o = plan(in);
    expect("lds/lanes16_lut", o.a.lut_in_lds, 0);
    expect("lds/lanes16_fold", o.a.fold_in_lds, 0);
    in.sw.lanes_per_pixel = 8;
    in.sw.tables_global = 1;
    expect("lds/tables_off_lut", plan(in).a.lut_in_lds, 0);
    in.sw.tables_global = 0;
    in.sw.clusters = 2;
    in.sf.n_groups = kMaxLdsGroups;
    expect("lds/scene_at_limit", plan(in).a.scene_in_lds, 1);
    in.sf.n_groups = kMaxLdsGroups + 1u;
    expect("lds/scene_past_limit", plan(in).a.scene_in_lds, 0);
    in.sf.n_groups = 32;
    in.sw.scene_global = 1;
    o = plan(in);
    expect("lds/scene_in_hbm", o.a.scene_in_lds, 0);
    in.sw.src = kSrcLds;
    expect("lds/scene_in_hbm_source", plan(in).p.src, kSrcSmem);
    in.sw.scene_global = 0;
    expect("lds/lds_source", plan(in).p.src, kSrcLds);
}

// one case per row of the routing comment in rt_kernel.h
void routing_cases() {
    In in;
    in.sw.lanes_per_pixel = 4;
    in.desc.MaxBounce = 0;
    expect("route/max_bounce0", plan(in).a.walk, kWalkAny);
    in.desc.MaxBounce = 8;
    in.sf.fast_sqrt = 0;
    expect("route/no_fast_sqrt", plan(in).a.walk, kWalkAny);
    in.sf.fast_sqrt = 1;
    in.sw.walk_any = 1;
    Out o = plan(in);
    expect("route/walk_any", o.a.walk, kWalkAny);
    expect("route/walk_any_table", o.p.table, kTablePlain);
    in.sw.walk_any = 0;
    in.sf.n_cpairs = 0;
    expect("route/no_table", plan(in).a.walk, kWalkGroups);
    in.sf.n_cpairs = 5;
    const uint32_t words[3] = {1, 2, 4};
    for (uint32_t i = 0; i < 3; ++i) {
        in.sf.cl_words = words[i];
        in.sf.pf_relative = 0;
        o = plan(in);
        const std::string n = "route/words" + std::to_string(words[i]);
        expect(n + "_scene_wide", o.a.walk, kWalkCl1 + i);
        expect(n + "_scene_wide_table", o.p.table, kTableExpanded);
        expect(n + "_scene_wide_pointer", o.a.clusters == kExpanded, 1);
        expect(n + "_scene_wide_prefilter", o.a.prefilter, kPrefilterExpanded);
        in.sf.pf_relative = 1;
        o = plan(in);
        expect(n + "_per_lane", o.a.walk, kWalkCl1Rel + i);
        expect(n + "_per_lane_table", o.p.table, kTablePlain);
        expect(n + "_per_lane_prefilter", o.a.prefilter, kPrefilterOn);
    }
    in.sf.cl_words = 1;
    in.sf.pf_relative = 0;
    in.sf.clusters_x_ok = false;
    o = plan(in);
    expect("route/scene_wide_unproven", o.a.walk, kWalkAny);
    expect("route/scene_wide_unproven_table", o.p.table, kTablePlain);
    in.sf.clusters_x_ok = true;
    // a shape without walk kernels, or no culling: the request stands and the expanded table is taken back
    for (const int lanes : {1, 2, 32}) {
        in.sw.lanes_per_pixel = lanes;
        in.sw.pixels_per_lane = 1;
        o = plan(in);
        const std::string n = "route/lanes" + std::to_string(lanes);
        expect(n + "_request", o.a.walk, kWalkCl1);
        expect(n + "_table", o.p.table, kTablePlain);
        expect(n + "_pointer", o.a.clusters == kPlain, 1);
        expect(n + "_prefilter", o.a.prefilter, kPrefilterOn);
    }
    in.sw.lanes_per_pixel = 4;
    in.sw.cull = 0;
    o = plan(in);
    expect("route/cull_off_request", o.a.walk, kWalkCl1);
    expect("route/cull_off_table", o.p.table, kTablePlain);
    expect("route/cull_off_prefilter", o.a.prefilter, kPrefilterOn);
    in.sw.cull = 1;
    // per-tile counts on a four-wave device: the default one keeps its kernels, any other runs the one-wave run-time kernel
    in.counts = true;
    in.sw.solo = 0;
    o = plan(in);
    expect("route/counts_default_four_wave", o.a.solo, 0);
    in.sw.src = kSrcLds;
    o = plan(in);
    expect("route/counts_lds_source_solo", o.a.solo, 1);
    expect("route/counts_lds_source_walk", o.a.walk, kWalkAny);
    expect("route/counts_lds_source_image", o.a.lut_in_lds + o.a.fold_in_lds + o.a.scene_in_lds, 0);
    in.sw.src = kSrcSmem;
    in.sw.scene_global = 1;
    o = plan(in);
    expect("route/counts_scene_in_hbm_solo", o.a.solo, 1);
    expect("route/counts_scene_in_hbm_walk", o.a.walk, kWalkAny);
    in.sw.scene_global = 0;
    in.sw.clusters = 2;
    in.sf.n_groups = kMaxLdsGroups + 1u;
    o = plan(in);
    expect("route/counts_large_scene_solo", o.a.solo, 1);
    expect("route/counts_large_scene_walk", o.a.walk, kWalkAny);
    in.counts = false;
    expect("route/large_scene_four_wave", plan(in).a.solo, 0);
}

void geometry_cases() {
    In in;  // 64 x 48 at 8 lanes: 8 x 4 block tiles
    Out o = plan(in);
    expect("geometry/n_tiles", o.p.n_tiles, 8 * 12);
    expect("geometry/n_units", o.p.n_units, 4 * 8 * 12);
    expect("geometry/n_selected", o.p.n_selected, 8 * 12);
    expect("geometry/tiles_x", o.a.tiles_x, 8);
    expect("geometry/mask_words", (long long)o.p.mask_words, 8 * 12 * 4);
    expect("geometry/empty_capable", o.p.empty_capable, 1);
    expect("geometry/pixel_sort", o.p.pixel_sort, 1);
    expect("geometry/xcd_group_lanes8", o.p.xcd_group, 0);
    expect("geometry/skip_cur", o.p.skip_cur, 1);
    in.sf.use_sky = true;
    expect("geometry/sky_not_empty_capable", plan(in).p.empty_capable, 0);
    in.sf.use_sky = false;
    in.sw.lanes_per_pixel = 4;
    expect("geometry/xcd_group_lanes4", plan(in).p.xcd_group, 1);
    in.sw.wave_order = 0;
    o = plan(in);
    expect("geometry/block_units", o.p.n_units, o.p.n_tiles);
    expect("geometry/block_units_no_group", o.p.xcd_group, 0);
    in.sw.wave_order = 1;
    in.sw.lanes_per_pixel = 1;
    in.sw.pixels_per_lane = 1;
    o = plan(in);
    expect("geometry/lanes1_store_in_kernel", o.p.skip_cur, 0);
    expect("geometry/lanes1_no_pixel_sort", o.p.pixel_sort, 0);
    in.delta = true;
    expect("geometry/delta_leaves_rgba8", plan(in).p.skip_cur, 1);
}

void split_cases() {
    const struct {
        uint32_t frames, parts;
        const char *want;
        uint32_t head;
    } rows[] = {{127, 2, "127", 0}, {128, 2, "32,96", 32}, {256, 2, "32,224", 32}, {256, 8, "32,96,128", 128},
                {256, 1, "256", 0}, {4096, 1, "4096", 0}};
    for (const auto &r : rows) {
        const SplitSchedule s = split_schedule(r.frames, 4, 8, r.parts, 3, true);
        const std::string n = "split/frames" + std::to_string(r.frames) + "_parts" + std::to_string(r.parts);
        expect_text(n, list_of(s.parts, s.n_parts).c_str(), r.want);
        expect(n + "_head", s.head_frames, r.head);
    }
    // SplitGrowth 2^31: 32 x 2^31 wraps to 0, the schedule stops there and no part is empty
    const SplitSchedule w = split_schedule(256, 4, 8, 8, 0x80000000u, true);
    expect_text("split/growth_wraps", list_of(w.parts, w.n_parts).c_str(), "32,224");
    // per-tile counts, a key seen before, no culling or no order: the launch may not split
    const SplitSchedule n = split_schedule(256, 4, 8, 8, 3, false);
    expect_text("split/may_not", list_of(n.parts, n.n_parts).c_str(), "256");
    expect("split/may_not_head", n.head_frames, 0);
}

void selection_cases() {
    // 33 x 33: 2 x 2 reference tiles, the last column 1 pixel wide and the last row 1 pixel high
    const uint32_t W = 33, H = 33;
    const uint32_t size[4][2] = {{32, 32}, {1, 32}, {32, 1}, {1, 1}};
    std::vector<uint32_t> bits;
    TileSelection sel;
    uint32_t bad = 0;
    for (uint32_t t = 0; t < 4; ++t) {
        const std::string n = "selection/tile" + std::to_string(t);
        expect(n + "_valid", build_selection(&t, 1, W, H, bits, sel, &bad), 0);
        expect(n + "_class", sel.n_class[t], 1);
        expect(n + "_listed", sel.n_class[0] + sel.n_class[1] + sel.n_class[2] + sel.n_class[3], 1);
        expect(n + "_pixels", (long long)sel.pixels, size[t][0] * size[t][1]);
        expect(n + "_bits", sel.bits[0], 1u << t);
        for (const int p : kShapes)
            expect(n + "_block_tiles_p" + std::to_string(p), sel.block_tiles(p), rtk_tile_count(size[t][0], size[t][1], p));
    }
    const uint32_t all[4] = {3, 0, 2, 1};
    expect("selection/all_valid", build_selection(all, 4, W, H, bits, sel, &bad), 0);
    expect("selection/all_pixels", (long long)sel.pixels, 1089);
    expect("selection/all_words", sel.n_words, 1);
    expect("selection/all_tiles_x", sel.tiles_x, 2);
    expect("selection/clip", sel.clip_w * 100 + sel.clip_h, 101);
    for (const int p : kShapes) {
        uint32_t sum = 0;
        for (uint32_t t = 0; t < 4; ++t) sum += rtk_tile_count(size[t][0], size[t][1], p);
        expect("selection/all_block_tiles_p" + std::to_string(p), sel.block_tiles(p), sum);
    }
    const uint32_t past[3] = {0, 1, 4};
    expect("selection/past_image", build_selection(past, 3, W, H, bits, sel, &bad), -1);
    expect("selection/past_image_at", bad, 2);
    const uint32_t twice[4] = {2, 0, 1, 0};
    expect("selection/twice", build_selection(twice, 4, W, H, bits, sel, &bad), -2);
    expect("selection/twice_at", bad, 3);
    // the two refusals as each entry point words them
    const ListName tiles_name = {"rt_trace_tiles", "tiles[", "]"};
    expect("selection/text_past_rc", select_tiles(tiles_name, past, 3, W, H, bits, sel), RT_EINVAL);
    expect_text("selection/text_past", g_err, "rt_trace_tiles: tiles[2] = 4, the image has 4 tiles");
    expect("selection/text_twice_rc", select_tiles(tiles_name, twice, 4, W, H, bits, sel), RT_EINVAL);
    expect_text("selection/text_twice", g_err, "rt_trace_tiles: tiles[3] = 0 is listed twice");
    TileWorkList work;
    const rt_tile_work w_past[2] = {{1, 0, 4}, {7, 0, 4}};
    expect("work/past_rc", plan_tile_work(w_past, 2, W, H, work), RT_EINVAL);
    expect_text("work/past_text", g_err, "rt_trace_tile_work: work[1].Tile = 7, the image has 4 tiles");
    // a zero-frame entry is still checked for a duplicate before it is dropped
    const rt_tile_work w_twice[3] = {{1, 0, 4}, {2, 8, 2}, {1, 0, 0}};
    expect("work/twice_rc", plan_tile_work(w_twice, 3, W, H, work), RT_EINVAL);
    expect_text("work/twice_text", g_err, "rt_trace_tile_work: work[2].Tile = 1 is listed twice");
    const rt_tile_work w_wrap[1] = {{0, 0xFFFFFFFFu, 1}};
    expect("work/wrap_rc", plan_tile_work(w_wrap, 1, W, H, work), RT_EINVAL);
    expect_text("work/wrap_text", g_err, "rt_trace_tile_work: work[0]: PreviousRayCount + Frames exceeds the u32 frame count");
    const rt_tile_work mixed[4] = {{3, 5, 2}, {0, 0, 0}, {1, 0, 7}, {2, 0, 0}};
    expect("work/mixed_rc", plan_tile_work(mixed, 4, W, H, work), RT_OK);
    expect("work/mixed_kept", work.kept, 2);
    expect("work/mixed_uniform", work.uniform, 0);
    expect("work/mixed_max_frames", work.max_frames, 7);
    expect("work/mixed_bits", work.sel.bits[0], 0xA);
    expect("work/mixed_pixels", (long long)work.sel.pixels, 33);
    expect_text("work/mixed_table", list_of(work.table.data(), (uint32_t)work.table.size()).c_str(), "0,0,0,7,0,0,5,2");
    const rt_tile_work same[3] = {{3, 5, 2}, {0, 5, 2}, {1, 9, 0}};
    expect("work/uniform_rc", plan_tile_work(same, 3, W, H, work), RT_OK);
    expect("work/uniform", work.uniform, 1);
    expect("work/uniform_first", work.first.PreviousRayCount * 100 + work.first.Frames, 502);
    expect("work/uniform_bits", work.sel.bits[0], 0x9);
    const rt_tile_work none[1] = {{3, 5, 0}};
    expect("work/none_rc", plan_tile_work(none, 1, W, H, work), RT_OK);
    expect("work/none_kept", work.kept, 0);
}

void key_cases() {
    const In base;
    const std::vector<uint32_t> k0 = plan(base).key;
    expect("key/equal_inputs", plan(base).key == k0, 1);
    expect("key/words", (long long)k0.size(), 15 + 14 + 1);
    auto differs = [&](const std::string &name, const In &in) { expect("key/" + name, plan(in).key != k0, 1); };
    auto same = [&](const std::string &name, const In &in) { expect("key/" + name, plan(in).key == k0, 1); };
    In in = base;
    in.desc.Width = 65;
    differs("width", in);
    in = base;
    in.desc.Height = 49;
    differs("height", in);
    in = base;
    in.local_rows = 47;
    differs("local_rows", in);
    in = base;
    in.desc.BandRows = 8;
    differs("band_rows", in);
    in = base;
    in.desc.BandCount = 2;
    differs("band_count", in);
    in = base;
    in.desc.BandCount = 2;
    const std::vector<uint32_t> k_band = plan(in).key;
    in.desc.BandIndex = 1;
    expect("key/band_index", plan(in).key != k_band, 1);
    in = base;
    in.sw.lanes_per_pixel = 4;
    differs("shape_code", in);
    in = base;
    in.rs = 1;
    differs("rule_set", in);
    in = base;
    in.sw.cull = 0;
    differs("cull", in);
    in = base;
    in.sf.use_sky = true;
    differs("empty_capable", in);
    in = base;
    in.sw.tile_sched = 0;
    differs("sched", in);
    in = base;
    in.sw.interleave = 1;
    differs("interleave", in);
    in = base;
    in.sw.wave_order = 0;
    differs("unit_waves", in);
    in = base;
    in.sf.scene_gen = 2;
    differs("scene_gen_low", in);
    in = base;
    in.sf.scene_gen = 1ull | (1ull << 32);
    differs("scene_gen_high", in);
    for (int i = 0; i < 14; ++i) {
        in = base;
        in.cam[i] += 0.5f;
        differs("camera_float" + std::to_string(i), in);
    }
    std::vector<uint32_t> bits, bits2;
    TileSelection sel, sel2;
    uint32_t bad = 0;
    const uint32_t all[4] = {0, 1, 2, 3}, but_one[3] = {0, 1, 3};  // (64 x 48: 2 x 2 reference tiles)
    expect("key/selection_all_valid", build_selection(all, 4, 64, 48, bits, sel, &bad), 0);
    expect("key/selection_but_one_valid", build_selection(but_one, 3, 64, 48, bits2, sel2, &bad), 0);
    in = base;
    in.sw.lanes_per_pixel = 8;  // (the shape a list must not change by its pixel count here)
    const std::vector<uint32_t> k_all = plan(in).key;
    in.sel = &sel;
    const std::vector<uint32_t> k_sel = plan(in).key;
    expect("key/selection_present", k_sel != k_all, 1);
    expect("key/selection_words", (long long)k_sel.size(), 15 + 14 + 1 + 1);
    in.sel = &sel2;
    expect("key/selection_one_bit", plan(in).key != k_sel, 1);
    in.sel = &sel;
    in.counts = true;
    expect("key/counts_not_in_key", plan(in).key == k_sel, 1);
    in.counts = false;
    in.delta = true;
    expect("key/delta_not_in_key", plan(in).key == k_sel, 1);
    in = base;
    in.desc.Frames = 255;
    in.desc.PreviousRayCount = 3;
    in.desc.MaxBounce = 7;
    same("frames_and_counts_not_in_key", in);
}

void option_cases() {
    rt_device_options o;
    memset(&o, 0, sizeof(o));
    expect("options/null", check_options(nullptr), RT_OK);
    expect("options/zero", check_options(&o), RT_OK);
    Switches s = from_options(o);
    expect("options/defaults", s.cull * 1000 + s.clusters * 100 + (int)s.head_samples * 10 + (int)s.split_parts, 1182);
    expect("options/default_tristates", s.prefilter + s.pf_rel + s.xcd_group + s.merge, -4);
    o.Clusters = RT_OPT_ON;
    o.TablesInLds = RT_OPT_OFF;
    o.SphereSourceLds = RT_OPT_ON;
    o.OrderLaunches = -1;
    o.PixelSegment = 4;
    s = from_options(o);
    expect("options/clusters_on", s.clusters, 2);
    expect("options/tables_off", s.tables_global, 1);
    expect("options/lds_source", s.src, kSrcLds);
    expect("options/order_launches_none", s.order_launches, 0);
    expect("options/pixel_segment", s.pixel_seg, 4);
    o.LanesPerPixel = 3;
    expect("options/lanes3_rc", check_options(&o), RT_EINVAL);
    expect_text("options/lanes3_text", g_err, "rt_device_options: LanesPerPixel 3");
    o.LanesPerPixel = 0;
    o.Cull = 2;
    expect("options/switch2_rc", check_options(&o), RT_EINVAL);
    expect_text("options/switch2_text", g_err, "rt_device_options: a switch is 2 (RT_OPT_DEFAULT/ON/OFF)");
    o.Cull = 0;
    o.SplitParts = 9;
    expect("options/parts9_rc", check_options(&o), RT_EINVAL);
    o.SplitParts = 8;
    expect("options/parts8_rc", check_options(&o), RT_OK);
}

}  // namespace

int main() {
    shape_case<0>();
    shape_case<1>();
    shape_case<2>();
    shape_case<4>();
    shape_case<8>();
    shape_case<16>();
    shape_case<32>();
    lanes_cases();
    pixels_per_lane_cases();
    threshold_cases();
    merge_cases();
    table_cases();
    lds_cases();
    routing_cases();
    geometry_cases();
    split_cases();
    selection_cases();
    key_cases();
    option_cases();
    return g_bad;
}
