// tile_counts_check.cpp — the device-free part of rt_trace_tile_counts and rt_tile_counts_step (csrc/rt_plan.cpp
// plan_tile_counts, check_tile_step; rt_kernel.h rtk_effective_frames) as a plain host program: no HIP library,
// no device.  Links csrc/rt_plan.cpp only, beside tests/plan_check and in its manner: one printed line per
// case, "section/case : value", compared with the literal the case states (exit status 1 and a line on stderr
// where they differ).  The pointers a call names as device memory are compared, never followed: the stand-ins
// here are host addresses with the alignment a case needs.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "rt_plan.h"

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
        fprintf(stderr, "tile_counts_check: %s: got %lld, expected %lld\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

void expect_text(const std::string &name, const char *got, const char *want) {
    printf("%s : %s\n", name.c_str(), got);
    if (strcmp(got, want)) {
        fprintf(stderr, "tile_counts_check: %s: got \"%s\", expected \"%s\"\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

alignas(16) unsigned char g_mem[64];  // stand-ins for device memory

struct Call {
    rt_camera_info cam;
    rt_trace_desc desc;
    std::vector<uint32_t> tiles = {0, 1, 3};
    const void *counts = g_mem + 32, *delta = g_mem;
    uint32_t max_frames = 16;
    uint64_t rays = 0;
    std::vector<uint32_t> bits;
    TileCountsCall out;
    Call() {
        memset(&cam, 0, sizeof(cam));
        memset(&desc, 0, sizeof(desc));
        desc.Width = 64;  // 2 x 2 tiles
        desc.Height = 48;
        desc.PreviousRayCount = 0xFFFFFFFFu;  // (not read: values rt_trace itself refuses)
        desc.Frames = 0xFFFFFFFFu;
        desc.MaxBounce = 8;
        desc.EnableSIMD = 1;
        desc.SeedMode = RT_SEED_PIXEL;
    }
    int run(const rt_trace_desc *d) {
        g_err[0] = 0;
        return plan_tile_counts(true, true, true, &cam, d, tiles.empty() ? nullptr : tiles.data(), (uint32_t)tiles.size(),
                                counts, max_frames, delta, &rays, bits, out);
    }
    int run() { return run(&desc); }
};

// The key of a launch planned over `sel` with or without per-tile counts (the defaults of tests/plan_check).
std::vector<uint32_t> key_of(const rt_trace_desc &desc, const TileSelection *sel, bool counts, bool delta) {
    Switches sw;
    SceneFacts sf;
    sf.n_groups = 16;
    sf.prefilter = 1;
    sf.fast_sqrt = 1;
    sf.n_spheres = 64;
    sf.scene_gen = 1;
    TraceArgs a;
    memset(&a, 0, sizeof(a));
    a.width = desc.Width;
    a.height = a.local_rows = desc.Height;
    a.frames = desc.Frames;
    a.max_bounce = desc.MaxBounce;
    a.band_rows = 32u;
    a.band_count = 1u;
    std::vector<uint32_t> key;
    (void)plan_launch(sw, sf, 0, 1, desc, desc.Height, sel, counts, delta, TablePointers{}, a, key);
    return key;
}

void effective_frames() {
    expect("clamp/below_bound", rtk_effective_frames(3, 5, 12), 5);
    expect("clamp/at_bound", rtk_effective_frames(3, 12, 12), 12);
    expect("clamp/above_bound", rtk_effective_frames(3, 100, 12), 12);
    expect("clamp/zero_frames", rtk_effective_frames(3, 0, 12), 0);
    expect("clamp/fits_exactly", rtk_effective_frames(0xFFFFFFF0u, 0x0F, 0x20), 0x0F);
    expect("clamp/overflow", rtk_effective_frames(0xFFFFFFF0u, 0x20, 0x20), 0);
    expect("clamp/overflow_after_clamp_fits", rtk_effective_frames(0xFFFFFFF0u, 0x20, 0x0F), 0x0F);
    expect("clamp/overflow_by_one", rtk_effective_frames(0xFFFFFFFFu, 1, 1), 0);
    expect("clamp/last_frame", rtk_effective_frames(0xFFFFFFFEu, 1, 1), 1);
}

void refusals() {
    Call c;
    expect("refuse/good", c.run(), RT_OK);
    expect("refuse/good_nothing", c.out.nothing, 0);
    expect("refuse/desc_frames", c.out.desc.Frames, 16);
    expect("refuse/desc_prev", c.out.desc.PreviousRayCount, 0);
    expect("refuse/desc_kept", c.out.desc.Width == 64 && c.out.desc.MaxBounce == 8, 1);
    expect("refuse/sel_tiles", c.out.sel.n_tiles, 4);
    expect("refuse/sel_bits", c.out.sel.bits[0], 0xB);
    expect("refuse/null_desc", c.run(nullptr), RT_EINVAL);
    {
        Call k;
        k.counts = nullptr;
        expect("refuse/null_counts", k.run(), RT_EINVAL);
        expect_text("refuse/null_counts_text", g_err, "rt_trace_tile_counts: d_counts is NULL");
    }
    {
        Call k;
        k.max_frames = 0;
        expect("refuse/max_frames_0", k.run(), RT_EINVAL);
        expect_text("refuse/max_frames_text", g_err, "rt_trace_tile_counts: max_frames is 0");
    }
    {
        Call k;
        k.delta = g_mem + 8;
        expect("refuse/delta_misaligned", k.run(), RT_EINVAL);
        k.delta = nullptr;
        expect("refuse/delta_null_is_fine", k.run(), RT_OK);
    }
    {
        Call k;
        k.desc.BandCount = 2;
        expect("refuse/bands", k.run(), RT_EINVAL);
        k.desc.BandCount = 1;
        k.desc.Flags = 4;
        expect("refuse/flags", k.run(), RT_EINVAL);
    }
    {
        Call k;
        k.tiles = {0, 4};
        expect("refuse/past", k.run(), RT_EINVAL);
        expect_text("refuse/text_past", g_err, "rt_trace_tile_counts: tiles[1] = 4, the image has 4 tiles");
        k.tiles = {1, 0, 1};
        expect("refuse/twice", k.run(), RT_EINVAL);
        expect_text("refuse/text_twice", g_err, "rt_trace_tile_counts: tiles[2] = 1 is listed twice");
    }
    {
        Call k;
        expect("refuse/null_list", plan_tile_counts(true, true, true, &k.cam, &k.desc, nullptr, 2, k.counts, 16, k.delta,
                                                    &k.rays, k.bits, k.out), RT_EINVAL);
        expect("refuse/no_device", plan_tile_counts(false, true, true, &k.cam, &k.desc, k.tiles.data(), 3, k.counts, 16,
                                                    k.delta, &k.rays, k.bits, k.out), RT_EINVAL);
        expect("refuse/no_scene", plan_tile_counts(true, true, false, &k.cam, &k.desc, k.tiles.data(), 3, k.counts, 16,
                                                   k.delta, &k.rays, k.bits, k.out), RT_EINVAL);
        k.tiles.clear();
        expect("refuse/empty_list_ok", k.run(), RT_OK);
        expect("refuse/empty_list_nothing", k.out.nothing, 1);
    }
}

void keys() {
    Call c;
    (void)c.run();
    // rt_trace_tiles over the same tiles at Frames = max_frames: the same selection, the same key
    std::vector<uint32_t> bits;
    TileSelection sel;
    const ListName name = {"rt_trace_tiles", "tiles[", "]"};
    (void)select_tiles(name, c.tiles.data(), 3, 64, 48, bits, sel);
    rt_trace_desc d = c.out.desc;
    const std::vector<uint32_t> k_tiles = key_of(d, &sel, false, false);
    const std::vector<uint32_t> k_counts = key_of(c.out.desc, &c.out.sel, true, true);
    expect("key/same_as_rt_trace_tiles", k_tiles == k_counts, 1);
    expect("key/counts_launch_same_key", key_of(c.out.desc, &c.out.sel, true, false) == k_counts, 1);
    // another list is another key; another bound that keeps the shape is not
    Call o;
    o.tiles = {0, 1, 2};
    (void)o.run();
    expect("key/other_list", key_of(o.out.desc, &o.out.sel, true, true) == k_counts, 0);
    Call m;
    m.max_frames = 40;
    (void)m.run();
    expect("key/other_bound_same_shape", key_of(m.out.desc, &m.out.sel, true, true) == k_counts, 1);
}

void step_rule() {
    rt_tile_rule r = {sizeof(rt_tile_rule), 16, 32, 1, 0xFFFFFFFFu};
    uint32_t n = 0;
    expect("step/good", check_tile_step(g_mem + 32, g_mem, 136, 104, &r, &n), RT_OK);
    expect("step/tiles", n, 20);
    expect("step/null_counts", check_tile_step(nullptr, g_mem, 136, 104, &r, &n), RT_EINVAL);
    expect("step/null_delta", check_tile_step(g_mem + 32, nullptr, 136, 104, &r, &n), RT_EINVAL);
    expect("step/null_rule", check_tile_step(g_mem + 32, g_mem, 136, 104, nullptr, &n), RT_EINVAL);
    expect("step/delta_misaligned", check_tile_step(g_mem + 32, g_mem + 4, 136, 104, &r, &n), RT_EINVAL);
    expect("step/empty_image", check_tile_step(g_mem + 32, g_mem, 0, 104, &r, &n), RT_EINVAL);
    r.Size = 16;
    expect("step/size", check_tile_step(g_mem + 32, g_mem, 136, 104, &r, &n), RT_EINVAL);
    r.Size = sizeof(rt_tile_rule);
    r.MaxRoundFrames = 0;
    expect("step/round_0", check_tile_step(g_mem + 32, g_mem, 136, 104, &r, &n), RT_EINVAL);
    r.MaxRoundFrames = 16;
    r.MaxTileFrames = 0;
    expect("step/tile_0", check_tile_step(g_mem + 32, g_mem, 136, 104, &r, &n), RT_EINVAL);
}

}  // namespace

int main() {
    effective_frames();
    refusals();
    keys();
    step_rule();
    if (!g_bad) printf("tile_counts_check : ok\n");
    return g_bad;
}
