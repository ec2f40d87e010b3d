// first_hit_check.cpp — the device-free part of rt_trace_first_hit (csrc/rt_plan.cpp plan_first_hit) as a plain
// host program: no HIP library, no device.  Links csrc/rt_plan.cpp only, beside tests/plan_check and in its
// manner: one printed line per case, "section/case : value", compared with the literal the case states (exit
// status 1 and a line on stderr where they differ).  The planes a call names as device memory are compared,
// never followed: the stand-ins here are host addresses with the alignment a case needs.
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
        fprintf(stderr, "first_hit_check: %s: got %lld, expected %lld\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

void expect_text(const std::string &name, const char *got, const char *want) {
    printf("%s : %s\n", name.c_str(), got);
    if (strcmp(got, want)) {
        fprintf(stderr, "first_hit_check: %s: got \"%s\", expected \"%s\"\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

alignas(16) unsigned char g_mem[96];  // stand-ins for device memory

struct Call {
    rt_camera_info cam;
    rt_trace_desc desc;
    rt_first_hit_planes planes;
    std::vector<uint32_t> tiles = {0, 1, 3};
    bool null_list = false;  // tiles == NULL (n_tiles stays tiles.size())
    uint32_t flags = 0;
    bool have_device = true, scene_set = true;
    std::vector<uint32_t> bits;
    FirstHitCall out;
    Call() {
        memset(&cam, 0, sizeof(cam));
        memset(&desc, 0, sizeof(desc));
        desc.Width = 64;  // 2 x 2 tiles
        desc.Height = 48;
        desc.PreviousRayCount = 0xFFFFFFFFu;  // a frame index like any other
        desc.Frames = 0xFFFFFFFFu;            // (not read: with that PreviousRayCount rt_trace itself refuses it)
        desc.MaxBounce = 0;                   // (not read)
        desc.Flags = 0xFFFFFFFFu;             // (not read: rt_trace refuses unknown bits)
        desc.EnableSIMD = 1;
        desc.SeedMode = RT_SEED_PIXEL;
        planes.Size = sizeof(rt_first_hit_planes);
        planes.Hit = (rt_first_hit *)(g_mem + 8);  // 8-byte aligned, not 16
        planes.Normal = (float *)(g_mem + 16);
        planes.Albedo = (float *)(g_mem + 48);
    }
    int run(const rt_camera_info *c, const rt_trace_desc *d, const rt_first_hit_planes *p) {
        g_err[0] = 0;
        return plan_first_hit(have_device, scene_set, c, d, null_list ? nullptr : tiles.data(), (uint32_t)tiles.size(),
                              flags, p, bits, out);
    }
    int run() { return run(&cam, &desc, &planes); }
};

void refusals() {
    {
        Call c;
        expect("accept/list", c.run(), RT_OK);
        expect("accept/list_all", c.out.all ? 1 : 0, 0);
        expect("accept/list_nothing", c.out.nothing ? 1 : 0, 0);
        expect_text("accept/no_text", g_err, "");
    }
    {
        Call c;
        c.have_device = false;
        expect("refuse/no_device", c.run(), RT_EINVAL);
        expect_text("refuse/null_text", g_err, "rt_trace_first_hit: NULL argument");
    }
    {
        Call c;
        expect("refuse/no_cam", c.run(nullptr, &c.desc, &c.planes), RT_EINVAL);
        expect("refuse/no_desc", c.run(&c.cam, nullptr, &c.planes), RT_EINVAL);
        expect("refuse/no_out", c.run(&c.cam, &c.desc, nullptr), RT_EINVAL);
    }
    for (const uint32_t size : {0u, 24u, 40u}) {
        Call c;
        c.planes.Size = size;
        expect("refuse/size" + std::to_string(size), c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.planes.Size = 31;
        (void)c.run();
        expect_text("refuse/size_text", g_err, "rt_first_hit_planes: Size 31, this library's is 32");
    }
    {
        Call c;
        c.planes.Hit = nullptr;
        c.planes.Normal = nullptr;
        c.planes.Albedo = nullptr;
        expect("refuse/no_plane", c.run(), RT_EINVAL);
        expect_text("refuse/no_plane_text", g_err, "rt_trace_first_hit: every plane is NULL");
    }
    // each plane alone is enough
    for (int k = 0; k < 3; ++k) {
        Call c;
        if (k != 0) c.planes.Hit = nullptr;
        if (k != 1) c.planes.Normal = nullptr;
        if (k != 2) c.planes.Albedo = nullptr;
        expect("accept/plane" + std::to_string(k) + "_alone", c.run(), RT_OK);
    }
    {
        Call c;
        c.planes.Hit = (rt_first_hit *)(g_mem + 4);
        expect("refuse/hit_misaligned", c.run(), RT_EINVAL);
        expect_text("refuse/hit_misaligned_text", g_err, "rt_trace_first_hit: Hit is not 8-byte aligned");
    }
    {
        Call c;
        c.planes.Normal = (float *)(g_mem + 24);
        expect("refuse/normal_misaligned", c.run(), RT_EINVAL);
        expect_text("refuse/normal_misaligned_text", g_err, "rt_trace_first_hit: Normal is not 16-byte aligned");
    }
    {
        Call c;
        c.planes.Albedo = (float *)(g_mem + 56);
        expect("refuse/albedo_misaligned", c.run(), RT_EINVAL);
        expect_text("refuse/albedo_misaligned_text", g_err, "rt_trace_first_hit: Albedo is not 16-byte aligned");
    }
    for (const uint32_t f : {2u, 3u, 0x80000000u}) {
        Call c;
        c.flags = f;
        expect("refuse/flags" + std::to_string(f), c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.flags = RT_HIT_PIXEL_CENTRE;
        expect("accept/centre", c.run(), RT_OK);
    }
    {
        Call c;
        c.desc.SeedMode = RT_SEED_PIXEL + 1u;
        expect("refuse/seed_mode", c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.desc.BandCount = 2;
        expect("refuse/band_count2", c.run(), RT_EINVAL);
        c.desc.BandCount = 1;
        expect("accept/band_count1", c.run(), RT_OK);
        c.desc.BandIndex = 1;
        expect("refuse/band_index1", c.run(), RT_EINVAL);
    }
    for (int k = 0; k < 4; ++k) {
        Call c;
        c.desc.Width = k == 0 ? 0u : k == 2 ? 65537u : 64u;
        c.desc.Height = k == 1 ? 0u : k == 3 ? 65537u : 48u;
        expect("refuse/image" + std::to_string(k), c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.scene_set = false;
        expect("refuse/no_scene", c.run(), RT_EINVAL);
        expect_text("refuse/no_scene_text", g_err, "rt_trace_first_hit: no scene uploaded (rt_scene_upload)");
    }
    {
        Call c;
        c.null_list = true;
        expect("refuse/null_list_with_count", c.run(), RT_EINVAL);
        expect_text("refuse/null_list_text", g_err, "rt_trace_first_hit: tiles is NULL with n_tiles 3");
    }
    {
        Call c;
        c.tiles = {0, 4};
        expect("refuse/past", c.run(), RT_EINVAL);
        expect_text("refuse/past_text", g_err, "rt_trace_first_hit: tiles[1] = 4, the image has 4 tiles");
    }
    {
        Call c;
        c.tiles = {0, 1, 1};
        expect("refuse/twice", c.run(), RT_EINVAL);
        expect_text("refuse/twice_text", g_err, "rt_trace_first_hit: tiles[2] = 1 is listed twice");
    }
}

void nothing_to_do() {
    {
        Call c;  // every tile: tiles == NULL with n_tiles == 0
        c.tiles.clear();
        c.null_list = true;
        expect("all/rc", c.run(), RT_OK);
        expect("all/all", c.out.all ? 1 : 0, 1);
        expect("all/nothing", c.out.nothing ? 1 : 0, 0);
        expect("all/tiles_x", c.out.sel.tiles_x, 2);
        expect("all/n_tiles", c.out.sel.n_tiles, 4);
    }
    {
        Call c;  // a list of no tiles: nothing to launch
        c.tiles.clear();
        c.tiles.reserve(1);  // (data() of an empty vector with capacity: a non-NULL pointer)
        expect("empty/rc", c.run(), RT_OK);
        expect("empty/all", c.out.all ? 1 : 0, 0);
        expect("empty/nothing", c.out.nothing ? 1 : 0, 1);
    }
}

// The bitmap of a list is build_selection's, word for word, with its clipping.
void bitmap() {
    struct Case {
        const char *name;
        uint32_t w, h;
        std::vector<uint32_t> tiles;
    };
    const Case cases[] = {
        {"ragged", 136, 104, {7, 19, 4, 9, 14}},
        {"descending", 136, 104, {19, 18, 17, 3, 2, 1, 0}},
        {"one", 64, 48, {3}},
        {"wide", 32 * 70, 32, {0, 31, 32, 33, 63, 64, 69}},
    };
    for (const Case &k : cases) {
        Call c;
        c.desc.Width = k.w;
        c.desc.Height = k.h;
        c.tiles = k.tiles;
        const std::string n = std::string("bitmap/") + k.name;
        expect(n + "_rc", c.run(), RT_OK);
        std::vector<uint32_t> bits;
        TileSelection sel;
        uint32_t bad = 0;
        expect(n + "_build", build_selection(k.tiles.data(), (uint32_t)k.tiles.size(), k.w, k.h, bits, sel, &bad), 0);
        expect(n + "_words", c.out.sel.n_words == sel.n_words && c.bits == bits ? 1 : 0, 1);
        expect(n + "_bits_are_the_vector", c.out.sel.bits == c.bits.data() ? 1 : 0, 1);
        expect(n + "_pixels", (long long)c.out.sel.pixels, (long long)sel.pixels);
        uint32_t set = 0;
        for (const uint32_t w : c.bits) set += (uint32_t)__builtin_popcount(w);
        expect(n + "_set_bits", set, (long long)k.tiles.size());
    }
    {
        Call c;  // ragged 136 x 104: tile 19 is the 8 x 8 corner, tile 4 an 8 x 32 right-column tile
        c.desc.Width = 136;
        c.desc.Height = 104;
        c.tiles = {19, 4, 0};
        (void)c.run();
        expect("bitmap/clip_pixels", (long long)c.out.sel.pixels, 8 * 8 + 8 * 32 + 32 * 32);
        expect("bitmap/clip_w", c.out.sel.clip_w, 8);
        expect("bitmap/clip_h", c.out.sel.clip_h, 8);
    }
}

}  // namespace

int main() {
    refusals();
    nothing_to_do();
    bitmap();
    printf("first_hit_check : %s\n", g_bad ? "FAILED" : "ok");
    return g_bad;
}
