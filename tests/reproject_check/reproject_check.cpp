// reproject_check.cpp — the device-free part of rt_reproject (csrc/rt_plan.cpp plan_reproject) as a plain host
// program: no HIP library, no device.  Links csrc/rt_plan.cpp only, beside tests/denoise_check and in its manner:
// one printed line per case, "section/case : value", compared with the literal the case states (exit status 1 and
// a line on stderr where they differ).  The planes a call names as device memory are compared, never followed: the
// stand-ins here are host addresses with the alignment a case needs.  The two cameras are host structs and are read.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>

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
        fprintf(stderr, "reproject_check: %s: got %lld, expected %lld\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

void expect_text(const std::string &name, const char *got, const char *want) {
    printf("%s : %s\n", name.c_str(), got);
    if (strcmp(got, want)) {
        fprintf(stderr, "reproject_check: %s: got \"%s\", expected \"%s\"\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// the same bits: 1
void expect_bits(const std::string &name, float got, float want) { expect(name, bits(got) == bits(want) ? 1 : 0, 1); }

alignas(16) unsigned char g_mem[8 * 64];  // stand-ins for device memory: one 64-byte slot per plane

rt_camera_info camera(float px, float py, float pz, float fx, float fy, float fz, float fw, float fh) {
    rt_camera_info c;
    memset(&c, 0, sizeof(c));
    c.CameraPosition = {px, py, pz, 0.0f};
    c.CameraX = {0.6f, 0.0f, -0.8f, 0.0f};
    c.CameraY = {0.0f, 1.0f, 0.0f, 0.0f};
    c.FilmCenter = {fx, fy, fz, 0.0f};
    c.FilmW = fw;
    c.FilmH = fh;
    return c;
}

struct Call {
    rt_reproject_desc d;
    rt_camera_info cam, prev;
    ReprojectArgs args;
    Call() {
        cam = camera(1.0f, 2.0f, 3.0f, 1.5f, 2.25f, 3.75f, 1.0f, 0.75f);
        prev = camera(0.1f, 0.2f, 0.3f, 0.7f, -0.1f, 1.9f, 1.25f, 0.3f);
        memset(&d, 0, sizeof(d));
        memset(&args, 0xEE, sizeof(args));
        d.Size = sizeof(rt_reproject_desc);
        d.Width = 136;
        d.Height = 104;
        d.Frames = 2;
        d.MaxHistory = 32;
        d.Flags = RT_REPROJECT_SRGB_POW;
        d.DepthTolerance = 0.02f;
        d.Camera = &cam;
        d.PreviousCamera = &prev;
        d.Mean = (const float *)(g_mem + 0 * 64);
        d.Hit = (const rt_first_hit *)(g_mem + 1 * 64 + 8);  // 8-byte aligned, not 16
        d.History = (const float *)(g_mem + 2 * 64);
        d.HistoryHit = (const rt_first_hit *)(g_mem + 3 * 64 + 8);
        d.HistoryCount = (const uint32_t *)(g_mem + 4 * 64 + 4);  // 4-byte aligned, no more
        d.Out = (float *)(g_mem + 5 * 64);
        d.OutCount = (uint32_t *)(g_mem + 6 * 64 + 4);
        d.Rgba8 = (uint32_t *)(g_mem + 7 * 64 + 4);
    }
    void no_history() { d.History = nullptr, d.HistoryHit = nullptr, d.HistoryCount = nullptr; }
    int run() {
        g_err[0] = 0;
        return plan_reproject(&d, args);
    }
};

void refuse(const std::string &name, Call &c, const char *text) {
    expect("refuse/" + name, c.run(), RT_EINVAL);
    expect_text("refuse/" + name + "_text", g_err, text);
}

void refusals() {
    {
        g_err[0] = 0;
        ReprojectArgs a;
        expect("refuse/null_desc", plan_reproject(nullptr, a), RT_EINVAL);
        expect_text("refuse/null_desc_text", g_err, "rt_reproject: NULL argument");
    }
    for (const uint32_t size : {0u, 104u, 120u}) {
        Call c;
        c.d.Size = size;
        expect("refuse/size" + std::to_string(size), c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.d.Size = 111;
        refuse("size111", c, "rt_reproject_desc: Size 111, this library's is 112");
    }
    for (int k = 0; k < 4; ++k) {
        Call c;
        c.d.Width = k == 0 ? 0u : k == 2 ? 65537u : 64u;
        c.d.Height = k == 1 ? 0u : k == 3 ? 65537u : 48u;
        expect("refuse/image" + std::to_string(k), c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.d.Width = 0;
        refuse("image", c, "rt_reproject: bad image size 0x104");
    }
    {
        Call c;
        c.d.Frames = 0;
        refuse("frames0", c, "rt_reproject: Frames is 0");
        c.d.Frames = 33;
        refuse("max_history_below_frames", c, "rt_reproject: MaxHistory 32 is below Frames 33");
        c.d.Frames = 1;
        c.d.MaxHistory = 0;
        refuse("max_history0", c, "rt_reproject: MaxHistory 0 is below Frames 1");
    }
    for (const uint32_t f : {1u, 4u, 0x80000000u}) {
        Call c;
        c.d.Flags = f;
        expect("refuse/flags" + std::to_string(f), c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.d.Flags = 4u | RT_REPROJECT_SRGB_POW;
        refuse("flags", c, "rt_reproject: unknown flags 0x6");
    }
    const float bad[] = {-1.0f, -0.0f - 1e-30f, NAN, INFINITY, -INFINITY};
    for (int k = 0; k < 5; ++k) {
        Call c;
        c.d.DepthTolerance = bad[k];
        refuse("depth_tolerance" + std::to_string(k), c, "rt_reproject: DepthTolerance is negative, NaN or infinite");
    }
    {
        Call c;
        c.d.Camera = nullptr;
        refuse("no_camera", c, "rt_reproject: Camera is NULL");
    }
    {
        Call c;
        c.d.PreviousCamera = nullptr;
        refuse("no_previous_camera", c, "rt_reproject: PreviousCamera is NULL");
    }
    {
        Call c;
        c.d.Mean = nullptr;
        refuse("no_mean", c, "rt_reproject: Mean is NULL");
    }
    {
        Call c;
        c.d.Hit = nullptr;
        refuse("no_hit", c, "rt_reproject: Hit is NULL");
    }
    {
        Call c;
        c.d.Out = nullptr;
        refuse("no_out", c, "rt_reproject: Out is NULL");
    }
    {
        Call c;
        c.d.OutCount = nullptr;
        refuse("no_out_count", c, "rt_reproject: OutCount is NULL");
    }
    // the three history planes: every way of giving one or two of them
    for (int mask = 1; mask < 7; ++mask) {
        Call c;
        if (!(mask & 1)) c.d.History = nullptr;
        if (!(mask & 2)) c.d.HistoryHit = nullptr;
        if (!(mask & 4)) c.d.HistoryCount = nullptr;
        refuse("history_partial" + std::to_string(mask), c,
               "rt_reproject: History, HistoryHit and HistoryCount must be all NULL or all given");
    }
    {
        Call c;
        c.d.Mean = (const float *)(g_mem + 8);
        refuse("mean_misaligned", c, "rt_reproject: Mean is not 16-byte aligned");
    }
    {
        Call c;
        c.d.Hit = (const rt_first_hit *)(g_mem + 64 + 4);
        refuse("hit_misaligned", c, "rt_reproject: Hit is not 8-byte aligned");
    }
    {
        Call c;
        c.d.History = (const float *)(g_mem + 2 * 64 + 8);
        refuse("history_misaligned", c, "rt_reproject: History is not 16-byte aligned");
    }
    {
        Call c;
        c.d.HistoryHit = (const rt_first_hit *)(g_mem + 3 * 64 + 4);
        refuse("history_hit_misaligned", c, "rt_reproject: HistoryHit is not 8-byte aligned");
    }
    {
        Call c;
        c.d.HistoryCount = (const uint32_t *)(g_mem + 4 * 64 + 2);
        refuse("history_count_misaligned", c, "rt_reproject: HistoryCount is not 4-byte aligned");
    }
    {
        Call c;
        c.d.Out = (float *)(g_mem + 5 * 64 + 8);
        refuse("out_misaligned", c, "rt_reproject: Out is not 16-byte aligned");
    }
    {
        Call c;
        c.d.OutCount = (uint32_t *)(g_mem + 6 * 64 + 1);
        refuse("out_count_misaligned", c, "rt_reproject: OutCount is not 4-byte aligned");
    }
    {
        Call c;
        c.d.Rgba8 = (uint32_t *)(g_mem + 7 * 64 + 2);
        refuse("rgba8_misaligned", c, "rt_reproject: Rgba8 is not 4-byte aligned");
    }
    {
        Call c;
        c.d.Out = (float *)c.d.Mean;
        refuse("out_is_mean", c, "rt_reproject: Out is Mean (the pass does not run in place)");
    }
    {
        Call c;
        c.d.Out = (float *)c.d.History;
        refuse("out_is_history", c, "rt_reproject: Out is History (the pass does not run in place)");
    }
    {
        Call c;
        c.d.OutCount = (uint32_t *)c.d.HistoryCount;
        refuse("out_count_is_history_count", c, "rt_reproject: OutCount is HistoryCount (the pass does not run in place)");
    }
    {
        Call c;  // a refused call leaves the caller's arguments as they were
        c.d.Frames = 0;
        (void)c.run();
        unsigned char same[sizeof(ReprojectArgs)];
        memset(same, 0xEE, sizeof(same));
        expect("refuse/args_untouched", memcmp(&c.args, same, sizeof(same)) == 0 ? 1 : 0, 1);
    }
}

void accepted() {
    {
        Call c;
        expect("accept/full", c.run(), RT_OK);
        expect_text("accept/no_text", g_err, "");
    }
    {
        Call c;  // a loop's first frame: no history, no Rgba8, no flag, no depth test
        c.no_history();
        c.d.Rgba8 = nullptr;
        c.d.Flags = 0;
        c.d.DepthTolerance = 0.0f;
        c.d.Frames = 1;
        c.d.MaxHistory = 1;
        expect("accept/minimal", c.run(), RT_OK);
        expect("accept/minimal_history_null", c.args.history == nullptr && c.args.history_hit == nullptr &&
                                                      c.args.history_count == nullptr && c.args.rgba8 == nullptr
                                                  ? 1
                                                  : 0,
               1);
        expect("accept/minimal_srgb_pow", c.args.srgb_pow, 0);
    }
    {
        Call c;
        c.d.Width = 1;
        c.d.Height = 1;
        expect("accept/1x1", c.run(), RT_OK);
        c.d.Width = 65536;
        c.d.Height = 65536;
        expect("accept/largest_image", c.run(), RT_OK);
        expect_bits("accept/largest_image_hw", c.args.hw, 32768.0f);
    }
    {
        Call c;
        c.d.Frames = 0xFFFFFFFFu;
        c.d.MaxHistory = 0xFFFFFFFFu;
        expect("accept/largest_counts", c.run(), RT_OK);
        expect("accept/largest_counts_frames", c.args.frames, 0xFFFFFFFFu);
    }
    {
        Call c;  // -0.0f is zero: the depth test is off
        c.d.DepthTolerance = -0.0f;
        expect("accept/minus_zero_tolerance", c.run(), RT_OK);
        expect_bits("accept/minus_zero_tolerance_is_plus_zero", c.args.depth_tolerance, 0.0f);
    }
    {
        Call c;  // the same camera twice, and Mean as History (only Out may not alias an input)
        c.d.PreviousCamera = c.d.Camera;
        c.d.History = c.d.Mean;
        expect("accept/same_camera_mean_as_history", c.run(), RT_OK);
    }
}

// What the launch receives: the planes and counts as given, both cameras' fields, and the host's constants, each the
// one f32 operation the header lists (volatile operands: the expected value is formed at run time, unfused).
void arguments() {
    Call c;
    expect("args/rc", c.run(), RT_OK);
    const ReprojectArgs &a = c.args;
    expect("args/planes",
           a.mean == c.d.Mean && a.hit == c.d.Hit && a.history == c.d.History && a.history_hit == c.d.HistoryHit &&
                   a.history_count == c.d.HistoryCount && a.out == c.d.Out && a.out_count == c.d.OutCount && a.rgba8 == c.d.Rgba8
               ? 1
               : 0,
           1);
    expect("args/width", a.width, 136);
    expect("args/height", a.height, 104);
    expect("args/frames", a.frames, 2);
    expect("args/max_history", a.max_history, 32);
    expect("args/srgb_pow", a.srgb_pow, 1);
    expect_bits("args/depth_tolerance", a.depth_tolerance, 0.02f);
    const rt_v3 *cur[4] = {&c.cam.CameraPosition, &c.cam.CameraX, &c.cam.CameraY, &c.cam.FilmCenter};
    const float *got_cur[4] = {a.cam_pos, a.cam_x, a.cam_y, a.film_center};
    int same = 1;
    for (int k = 0; k < 4; ++k)
        same &= bits(got_cur[k][0]) == bits(cur[k]->x) && bits(got_cur[k][1]) == bits(cur[k]->y) &&
                bits(got_cur[k][2]) == bits(cur[k]->z);
    expect("args/camera_fields", same, 1);
    expect_bits("args/film_w", a.film_w, 1.0f);
    expect_bits("args/film_h", a.film_h, 0.75f);
    const rt_v3 *prv[3] = {&c.prev.CameraPosition, &c.prev.CameraX, &c.prev.CameraY};
    const float *got_prv[3] = {a.prev_pos, a.prev_x, a.prev_y};
    same = 1;
    for (int k = 0; k < 3; ++k)
        same &= bits(got_prv[k][0]) == bits(prv[k]->x) && bits(got_prv[k][1]) == bits(prv[k]->y) &&
                bits(got_prv[k][2]) == bits(prv[k]->z);
    expect("args/previous_camera_fields", same, 1);
    expect_bits("args/prev_film_w", a.prev_film_w, 1.25f);
    expect_bits("args/prev_film_h", a.prev_film_h, 0.3f);
    const volatile float fcx = 0.7f, fcy = -0.1f, fcz = 1.9f, px = 0.1f, py = 0.2f, pz = 0.3f;
    const volatile float fvx = fcx - px, fvy = fcy - py, fvz = fcz - pz;
    expect_bits("args/fv_x", a.fv[0], fvx);
    expect_bits("args/fv_y", a.fv[1], fvy);
    expect_bits("args/fv_z", a.fv[2], fvz);
    const volatile float sx = fvx * fvx, sy = fvy * fvy, sz = fvz * fvz;
    const volatile float sxy = sx + sy;
    const volatile float ff = sxy + sz;
    expect_bits("args/ff", a.ff, ff);
    expect_bits("args/wf", a.wf, 136.0f);
    expect_bits("args/hf", a.hf, 104.0f);
    expect_bits("args/hw", a.hw, 68.0f);
    expect_bits("args/hh", a.hh, 52.0f);
    {
        Call o;  // odd sizes: the halves are exact
        o.d.Width = 75;
        o.d.Height = 41;
        expect("args/odd_rc", o.run(), RT_OK);
        expect_bits("args/odd_hw", o.args.hw, 37.5f);
        expect_bits("args/odd_hh", o.args.hh, 20.5f);
    }
    {
        Call k;  // an accepted call after a refused one overwrites the arguments
        k.d.Frames = 0;
        (void)k.run();
        k.d.Frames = 3;
        expect("args/after_refusal_rc", k.run(), RT_OK);
        expect("args/after_refusal_frames", k.args.frames, 3);
    }
}

}  // namespace

int main() {
    refusals();
    accepted();
    arguments();
    printf("reproject_check : %s\n", g_bad ? "FAILED" : "ok");
    return g_bad;
}
