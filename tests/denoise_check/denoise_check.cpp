// denoise_check.cpp — the device-free part of rt_denoise (csrc/rt_plan.cpp plan_denoise) as a plain host
// program: no HIP library, no device.  Links csrc/rt_plan.cpp only, beside tests/first_hit_check and in its
// manner: one printed line per case, "section/case : value", compared with the literal the case states (exit
// status 1 and a line on stderr where they differ).  The planes a call names as device memory are compared,
// never followed: the stand-ins here are host addresses with the alignment a case needs.
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
        fprintf(stderr, "denoise_check: %s: got %lld, expected %lld\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

void expect_text(const std::string &name, const char *got, const char *want) {
    printf("%s : %s\n", name.c_str(), got);
    if (strcmp(got, want)) {
        fprintf(stderr, "denoise_check: %s: got \"%s\", expected \"%s\"\n", name.c_str(), got, want);
        g_bad = 1;
    }
}

alignas(16) unsigned char g_mem[7 * 64];  // stand-ins for device memory: one 64-byte slot per plane

struct Call {
    rt_denoise_desc d;
    DenoisePlan plan;
    Call() {
        memset(&d, 0, sizeof(d));
        d.Size = sizeof(rt_denoise_desc);
        d.Width = 136;
        d.Height = 104;
        d.Iterations = 3;
        d.Flags = RT_DENOISE_DEMODULATE;
        d.NormalPower = 5;
        d.SigmaDepth = 0.25f;
        d.SigmaColor = 4.0f;
        d.Mean = (const float *)(g_mem + 0 * 64);
        d.Hit = (const rt_first_hit *)(g_mem + 1 * 64 + 8);  // 8-byte aligned, not 16
        d.Normal = (const float *)(g_mem + 2 * 64);
        d.Albedo = (const float *)(g_mem + 3 * 64);
        d.Out = (float *)(g_mem + 4 * 64);
        d.Scratch = (float *)(g_mem + 5 * 64);
        d.Rgba8 = (uint32_t *)(g_mem + 6 * 64 + 4);  // 4-byte aligned, no more
    }
    int run() {
        g_err[0] = 0;
        return plan_denoise(&d, plan);
    }
};

void refuse(const std::string &name, Call &c, const char *text) {
    expect("refuse/" + name, c.run(), RT_EINVAL);
    expect_text("refuse/" + name + "_text", g_err, text);
}

void refusals() {
    {
        g_err[0] = 0;
        DenoisePlan plan;
        expect("refuse/null_desc", plan_denoise(nullptr, plan), RT_EINVAL);
        expect_text("refuse/null_desc_text", g_err, "rt_denoise: NULL argument");
    }
    for (const uint32_t size : {0u, 80u, 96u}) {
        Call c;
        c.d.Size = size;
        expect("refuse/size" + std::to_string(size), c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.d.Size = 87;
        refuse("size87", c, "rt_denoise_desc: Size 87, this library's is 88");
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
        refuse("image", c, "rt_denoise: bad image size 0x104");
    }
    {
        Call c;
        c.d.Iterations = 0;
        refuse("iterations0", c, "rt_denoise: Iterations 0 (1..8)");
        c.d.Iterations = 9;
        refuse("iterations9", c, "rt_denoise: Iterations 9 (1..8)");
    }
    for (const uint32_t f : {4u, 7u, 0x80000000u}) {
        Call c;
        c.d.Flags = f;
        expect("refuse/flags" + std::to_string(f), c.run(), RT_EINVAL);
    }
    {
        Call c;
        c.d.Flags = 4u | RT_DENOISE_SRGB_POW;
        refuse("flags", c, "rt_denoise: unknown flags 0x6");
    }
    {
        Call c;
        c.d.NormalPower = 9;
        refuse("normal_power9", c, "rt_denoise: NormalPower 9 (0..8)");
    }
    const float bad[] = {-1.0f, -0.0f - 1e-30f, NAN, INFINITY, -INFINITY};
    for (int k = 0; k < 5; ++k) {
        Call c;
        c.d.SigmaDepth = bad[k];
        refuse("sigma_depth" + std::to_string(k), c, "rt_denoise: SigmaDepth is negative, NaN or infinite");
        Call e;
        e.d.SigmaColor = bad[k];
        refuse("sigma_color" + std::to_string(k), e, "rt_denoise: SigmaColor is negative, NaN or infinite");
    }
    {
        Call c;
        c.d.Mean = nullptr;
        refuse("no_mean", c, "rt_denoise: Mean is NULL");
    }
    {
        Call c;
        c.d.Hit = nullptr;
        refuse("no_hit", c, "rt_denoise: Hit is NULL");
    }
    {
        Call c;
        c.d.Out = nullptr;
        refuse("no_out", c, "rt_denoise: Out is NULL");
    }
    {
        Call c;
        c.d.Normal = nullptr;
        refuse("no_normal", c, "rt_denoise: Normal is NULL with NormalPower 5");
    }
    {
        Call c;
        c.d.Albedo = nullptr;
        refuse("no_albedo", c, "rt_denoise: Albedo is NULL with RT_DENOISE_DEMODULATE");
    }
    {
        Call c;
        c.d.Scratch = nullptr;
        refuse("no_scratch", c, "rt_denoise: Scratch is NULL with Iterations 3");
    }
    {
        Call c;
        c.d.Mean = (const float *)(g_mem + 8);
        refuse("mean_misaligned", c, "rt_denoise: Mean is not 16-byte aligned");
    }
    {
        Call c;
        c.d.Hit = (const rt_first_hit *)(g_mem + 64 + 4);
        refuse("hit_misaligned", c, "rt_denoise: Hit is not 8-byte aligned");
    }
    {
        Call c;
        c.d.Normal = (const float *)(g_mem + 2 * 64 + 8);
        refuse("normal_misaligned", c, "rt_denoise: Normal is not 16-byte aligned");
    }
    {
        Call c;
        c.d.Albedo = (const float *)(g_mem + 3 * 64 + 4);
        refuse("albedo_misaligned", c, "rt_denoise: Albedo is not 16-byte aligned");
    }
    {
        Call c;
        c.d.Out = (float *)(g_mem + 4 * 64 + 8);
        refuse("out_misaligned", c, "rt_denoise: Out is not 16-byte aligned");
    }
    {
        Call c;
        c.d.Scratch = (float *)(g_mem + 5 * 64 + 8);
        refuse("scratch_misaligned", c, "rt_denoise: Scratch is not 16-byte aligned");
    }
    {
        Call c;
        c.d.Rgba8 = (uint32_t *)(g_mem + 6 * 64 + 2);
        refuse("rgba8_misaligned", c, "rt_denoise: Rgba8 is not 4-byte aligned");
    }
    {
        Call c;
        c.d.Out = (float *)c.d.Mean;
        refuse("out_is_mean", c, "rt_denoise: Out is Mean (the filter does not run in place)");
    }
    {
        Call c;
        c.d.Scratch = (float *)c.d.Mean;
        refuse("scratch_is_mean", c, "rt_denoise: Scratch is Mean");
    }
    {
        Call c;
        c.d.Scratch = c.d.Out;
        refuse("scratch_is_out", c, "rt_denoise: Scratch is Out");
    }
}

void accepted() {
    {
        Call c;
        expect("accept/full", c.run(), RT_OK);
        expect_text("accept/no_text", g_err, "");
    }
    {
        Call c;  // every stop off, one pass: Mean, Hit and Out alone
        c.d.Iterations = 1;
        c.d.Flags = 0;
        c.d.NormalPower = 0;
        c.d.SigmaDepth = 0.0f;
        c.d.SigmaColor = 0.0f;
        c.d.Normal = nullptr;
        c.d.Albedo = nullptr;
        c.d.Scratch = nullptr;
        c.d.Rgba8 = nullptr;
        expect("accept/minimal", c.run(), RT_OK);
    }
    {
        Call c;  // a normal plane is not asked for without the normal stop, nor albedo without the flag
        c.d.NormalPower = 0;
        c.d.Normal = nullptr;
        c.d.Flags = RT_DENOISE_SRGB_POW;
        c.d.Albedo = nullptr;
        expect("accept/no_normal_no_albedo", c.run(), RT_OK);
    }
    {
        Call c;
        c.d.Flags = RT_DENOISE_DEMODULATE | RT_DENOISE_SRGB_POW;
        c.d.NormalPower = 8;
        c.d.Iterations = 8;
        expect("accept/both_flags_largest_counts", c.run(), RT_OK);
    }
    {
        Call c;
        c.d.Width = 1;
        c.d.Height = 1;
        expect("accept/1x1", c.run(), RT_OK);
        c.d.Width = 65536;
        c.d.Height = 65536;
        expect("accept/largest_image", c.run(), RT_OK);
    }
    {
        Call c;  // -0.0f is zero: the stop is off
        c.d.SigmaDepth = -0.0f;
        c.d.SigmaColor = -0.0f;
        expect("accept/minus_zero_sigmas", c.run(), RT_OK);
        expect("accept/minus_zero_ic0_is_zero", c.plan.ic0 == 0.0f ? 1 : 0, 1);
    }
}

// The passes: pass i at step 1 << i with ic = ic0 * step, pass 0 from Mean, each later one from the one before,
// Scratch and Out alternating so that the last lands in Out.
void passes() {
    for (const uint32_t n : {1u, 2u, 5u, 8u}) {
        Call c;
        c.d.Iterations = n;
        if (n == 1u) c.d.Scratch = nullptr;
        const std::string s = "plan/n" + std::to_string(n);
        expect(s + "_rc", c.run(), RT_OK);
        expect(s + "_passes", c.plan.n_passes, n);
        expect(s + "_ic0_is_a_quarter", c.plan.ic0 == 0.25f ? 1 : 0, 1);
        expect(s + "_first_source_is_mean", c.plan.pass[0].src == c.d.Mean ? 1 : 0, 1);
        expect(s + "_last_destination_is_out", c.plan.pass[n - 1].dst == c.d.Out ? 1 : 0, 1);
        int chained = 1, steps = 1, ics = 1, alternate = 1, scratch_used = 0, mean_written = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const DenoisePass &p = c.plan.pass[i];
            if (i > 0 && p.src != c.plan.pass[i - 1].dst) chained = 0;
            if (p.step != (1u << i)) steps = 0;
            if (p.ic != 0.25f * (float)(1u << i)) ics = 0;  // (powers of two: exact)
            if (p.dst != (((n - 1 - i) & 1u) ? c.d.Scratch : c.d.Out)) alternate = 0;
            if (p.dst == c.d.Scratch || p.src == c.d.Scratch) scratch_used = 1;
            if (p.dst == c.d.Mean || p.src == p.dst) mean_written = 1;
        }
        expect(s + "_chained", chained, 1);
        expect(s + "_steps", steps, 1);
        expect(s + "_ic", ics, 1);
        expect(s + "_alternate", alternate, 1);
        expect(s + "_scratch_used", scratch_used, n >= 2u ? 1 : 0);
        expect(s + "_never_in_place", mean_written, 0);
    }
    {
        Call c;  // no colour stop: every ic is 0
        c.d.SigmaColor = 0.0f;
        c.d.Iterations = 8;
        expect("plan/no_colour_rc", c.run(), RT_OK);
        int zero = c.plan.ic0 == 0.0f;
        for (uint32_t i = 0; i < 8; ++i) zero &= c.plan.pass[i].ic == 0.0f;
        expect("plan/no_colour_ic_zero", zero, 1);
        expect("plan/last_step", c.plan.pass[7].step, 128);
    }
    {
        Call c;  // ic0 is the f32 quotient, formed once
        c.d.SigmaColor = 3.0f;
        c.d.Iterations = 4;
        expect("plan/third_rc", c.run(), RT_OK);
        const volatile float one = 1.0f, three = 3.0f;
        const float ic0 = one / three;
        expect("plan/third_ic0", c.plan.ic0 == ic0 ? 1 : 0, 1);
        expect("plan/third_ic3", c.plan.pass[3].ic == ic0 * 8.0f ? 1 : 0, 1);
    }
    {
        Call c;  // a refused call leaves the caller's plan as it was
        expect("plan/keep_rc", c.run(), RT_OK);
        c.d.Iterations = 0;
        (void)c.run();
        expect("plan/kept_after_refusal", c.plan.n_passes, 3);
    }
}

}  // namespace

int main() {
    refusals();
    accepted();
    passes();
    printf("denoise_check : %s\n", g_bad ? "FAILED" : "ok");
    return g_bad;
}
