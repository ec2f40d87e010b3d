// reproject_clip_check.cpp — the device-free part of rt_reproject_clip (csrc/rt_plan.cpp plan_reproject_clip) as a
// plain host program: no HIP library, no device.  Links csrc/rt_plan.cpp only, beside tests/reproject_check and in
// its manner: one printed line per case, "section/case : value", compared with the literal the case states (exit
// status 1 and a line on stderr where they differ).  plan_reproject's own refusals and arguments are
// tests/reproject_check's; here they are reached through the outer desc: a sample of them with their texts, and the
// launch's arguments against plan_reproject's of the same inner desc, byte for byte.
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
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
        fprintf(stderr, "reproject_clip_check: %s: got %lld, expected %lld\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

void expect_text(const std::string &name, const char *got, const char *want) {
    printf("%s : %s\n", name.c_str(), got);
    if (strcmp(got, want)) {
        fprintf(stderr, "reproject_clip_check: %s: got \"%s\", expected \"%s\"\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

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
    rt_reproject_clip_desc d;
    rt_camera_info cam, prev;
    ReprojectClipArgs args;
    Call() {
        cam = camera(1.0f, 2.0f, 3.0f, 1.5f, 2.25f, 3.75f, 1.0f, 0.75f);
        prev = camera(0.1f, 0.2f, 0.3f, 0.7f, -0.1f, 1.9f, 1.25f, 0.3f);
        memset(&d, 0, sizeof(d));
        memset(&args, 0xEE, sizeof(args));
        d.Size = sizeof(rt_reproject_clip_desc);
        d.Radius = 3;
        d.Gamma = 0.75f;
        rt_reproject_desc &r = d.Reproject;
        r.Size = sizeof(rt_reproject_desc);
        r.Width = 136;
        r.Height = 104;
        r.Frames = 2;
        r.MaxHistory = 32;
        r.Flags = RT_REPROJECT_SRGB_POW;
        r.DepthTolerance = 0.02f;
        r.Camera = &cam;
        r.PreviousCamera = &prev;
        r.Mean = (const float *)(g_mem + 0 * 64);
        r.Hit = (const rt_first_hit *)(g_mem + 1 * 64 + 8);  // 8-byte aligned, not 16
        r.History = (const float *)(g_mem + 2 * 64);
        r.HistoryHit = (const rt_first_hit *)(g_mem + 3 * 64 + 8);
        r.HistoryCount = (const uint32_t *)(g_mem + 4 * 64 + 4);  // 4-byte aligned, no more
        r.Out = (float *)(g_mem + 5 * 64);
        r.OutCount = (uint32_t *)(g_mem + 6 * 64 + 4);
        r.Rgba8 = (uint32_t *)(g_mem + 7 * 64 + 4);
    }
    void no_history() { d.Reproject.History = nullptr, d.Reproject.HistoryHit = nullptr, d.Reproject.HistoryCount = nullptr; }
    int run() {
        g_err[0] = 0;
        return plan_reproject_clip(&d, args);
    }
};

void refuse(const std::string &name, Call &c, const char *text) {
    expect("refuse/" + name, c.run(), RT_EINVAL);
    expect_text("refuse/" + name + "_text", g_err, text);
    // a refused call leaves the arguments as they were
    bool untouched = true;
    for (size_t i = 0; i < sizeof(c.args); ++i) untouched = untouched && ((const unsigned char *)&c.args)[i] == 0xEE;
    expect("refuse/" + name + "_args_untouched", untouched ? 1 : 0, 1);
}

void refusals() {
    {
        g_err[0] = 0;
        ReprojectClipArgs a;
        expect("refuse/null_desc", plan_reproject_clip(nullptr, a), RT_EINVAL);
        expect_text("refuse/null_desc_text", g_err, "rt_reproject_clip: NULL argument");
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    {
        Call c;
        c.d.Size = 112;  // the inner desc's size is not the outer's
        refuse("size112", c, "rt_reproject_clip_desc: Size 112, this library's is 128");
    }
    {
        Call c;
        c.d.Size = 0;
        refuse("size0", c, "rt_reproject_clip_desc: Size 0, this library's is 128");
    }
    {
        Call c;
        c.d.Reproject.Size = 128;  // ... nor the outer's the inner's
        refuse("inner_size128", c, "rt_reproject_desc: Size 128, this library's is 112");
    }
    {
        Call c;
        c.d.Radius = 0;
        refuse("radius0", c, "rt_reproject_clip: Radius 0 is not in 1..3");
    }
    {
        Call c;
        c.d.Radius = 4;
        refuse("radius4", c, "rt_reproject_clip: Radius 4 is not in 1..3");
    }
    {
        Call c;
        c.d.Radius = 0xFFFFFFFFu;
        refuse("radius_max", c, "rt_reproject_clip: Radius 4294967295 is not in 1..3");
    }
    const struct {
        const char *name;
        float v;
    } gammas[] = {{"gamma_zero", 0.0f}, {"gamma_minus_zero", -0.0f}, {"gamma_negative", -1.0f}, {"gamma_nan", nan},
                  {"gamma_inf", inf},   {"gamma_minus_inf", -inf}};
    for (const auto &g : gammas) {
        Call c;
        c.d.Gamma = g.v;
        refuse(g.name, c, "rt_reproject_clip: Gamma is not a finite number above 0");
    }
    {  // the outer desc is judged first
        Call c;
        c.d.Radius = 7;
        c.d.Reproject.Width = 0;
        refuse("radius_before_inner", c, "rt_reproject_clip: Radius 7 is not in 1..3");
    }
    // what rt_reproject refuses for the inner desc, with its texts
    {
        Call c;
        c.d.Reproject.Width = 0;
        refuse("inner_image", c, "rt_reproject: bad image size 0x104");
    }
    {
        Call c;
        c.d.Reproject.Frames = 33;
        refuse("inner_max_history_below_frames", c, "rt_reproject: MaxHistory 32 is below Frames 33");
    }
    {
        Call c;
        c.d.Reproject.Flags = 1;
        refuse("inner_flags", c, "rt_reproject: unknown flags 0x1");
    }
    {
        Call c;
        c.d.Reproject.DepthTolerance = nan;
        refuse("inner_depth_tolerance", c, "rt_reproject: DepthTolerance is negative, NaN or infinite");
    }
    {
        Call c;
        c.d.Reproject.Camera = nullptr;
        refuse("inner_no_camera", c, "rt_reproject: Camera is NULL");
    }
    {
        Call c;
        c.d.Reproject.Mean = nullptr;
        refuse("inner_no_mean", c, "rt_reproject: Mean is NULL");
    }
    {
        Call c;
        c.d.Reproject.HistoryHit = nullptr;
        refuse("inner_history_partial", c, "rt_reproject: History, HistoryHit and HistoryCount must be all NULL or all given");
    }
    {
        Call c;
        c.d.Reproject.Out = (float *)(g_mem + 5 * 64 + 8);
        refuse("inner_out_misaligned", c, "rt_reproject: Out is not 16-byte aligned");
    }
    {
        Call c;
        c.d.Reproject.Out = (float *)c.d.Reproject.History;
        refuse("inner_out_is_history", c, "rt_reproject: Out is History (the pass does not run in place)");
    }
}

// An accepted call: RT_OK, rp equal to plan_reproject's arguments of the inner desc byte for byte, the desc's radius
// and gamma.
void accept(const std::string &name, Call &c) {
    expect("accept/" + name, c.run(), RT_OK);
    ReprojectArgs want;
    memset(&want, 0x11, sizeof(want));
    expect("accept/" + name + "_inner", plan_reproject(&c.d.Reproject, want), RT_OK);
    // (up to the last member: a struct assignment need not copy the padding behind it)
    expect("accept/" + name + "_rp", memcmp(&c.args.rp, &want, offsetof(ReprojectArgs, hh) + sizeof(float)) == 0 ? 1 : 0, 1);
    expect("accept/" + name + "_radius", c.args.radius, c.d.Radius);
    expect("accept/" + name + "_gamma", memcmp(&c.args.gamma, &c.d.Gamma, 4) == 0 ? 1 : 0, 1);
}

void accepted() {
    {
        Call c;
        accept("full", c);
    }
    {
        Call c;
        c.no_history();
        c.d.Reproject.Rgba8 = nullptr;
        accept("minimal", c);
    }
    for (const uint32_t r : {1u, 2u, 3u}) {
        Call c;
        c.d.Radius = r;
        accept("radius" + std::to_string(r), c);
    }
    {
        Call c;
        c.d.Gamma = 1e-45f;  // the smallest denormal is above 0
        accept("gamma_denormal", c);
    }
    {
        Call c;
        c.d.Gamma = 3.402823466e+38f;
        accept("gamma_largest", c);
    }
    {
        Call c;
        c.d.Reproject.Width = c.d.Reproject.Height = 1;
        accept("1x1", c);
    }
}

}  // namespace

int main() {
    static_assert(sizeof(rt_reproject_clip_desc) == 128, "rt_reproject_clip_desc is 128 bytes");
    static_assert(offsetof(rt_reproject_clip_desc, Reproject) == 16, "the inner desc starts at byte 16");
    refusals();
    accepted();
    printf("reproject_clip_check : %s\n", g_bad ? "FAILED" : "ok");
    return g_bad;
}
