// TEST-ONLY: the device math layer of csrc/rtk_math.h, one function per entry point, element-wise.
// This file includes the header itself and holds no copy of any function under test; it is built
// with the kernel translation units' own flags (simd-ray-tracer_amd/Makefile, target math_probe)
// into tests/math_probe/libmath_probe.so, which is never linked into librt_trace.so.
// tests/math_probe.py loads it; tests/test_gpu_math_layer.py holds the references.
//
// Every entry point takes host pointers and a count, allocates and copies by itself, and returns
// 0, or a negative code: -1 NULL argument, -2 device allocation, -3 copy in, -4 launch
// (hipGetLastError), -5 copy out.  Kernels: a 1-D grid of 256-thread blocks, out[i] = f(in[i])
// for i < n, plain loads and stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtk_math.h"

namespace {

constexpr uint32_t kBlock = 256;

__global__ void __launch_bounds__(kBlock) k_sqrt(const float *in, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = rtk::sqrt_rn(in[i]);
}

__global__ void __launch_bounds__(kBlock) k_rcp(const float *in, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = rtk::rcp_rn(in[i]);
}

__global__ void __launch_bounds__(kBlock) k_div(const float *a, const float *b, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = rtk::div_rn(a[i], b[i], rtk::rcp_rn(b[i]));
}

__global__ void __launch_bounds__(kBlock) k_fold(const uint32_t *pc, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const float2 w = rtk::fold_weights(pc[i]);
        out[2u * i] = w.x;
        out[2u * i + 1u] = w.y;
    }
}

__global__ void __launch_bounds__(kBlock) k_normalize(const float *in, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        float x = in[3u * i], y = in[3u * i + 1u], z = in[3u * i + 2u];
        rtk::normalize(x, y, z);
        out[3u * i] = x;
        out[3u * i + 1u] = y;
        out[3u * i + 2u] = z;
    }
}

// in_lds (uniform over the launch): the block first copies the 2048-entry table to LDS, as the
// trace kernels' LDS image holds it; otherwise every lookup reads the table in global memory.
__global__ void __launch_bounds__(kBlock) k_rsqrt(const float *table, const float *in, float *out, uint32_t n,
                                                  uint32_t in_lds) {
    __shared__ float lds[2048];
    if (in_lds) {
        for (uint32_t k = threadIdx.x; k < 2048u; k += kBlock) lds[k] = table[k];
        __syncthreads();
    }
    const rtk::Lut lut = {lds, table, in_lds != 0u};
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = rtk::rsqrt_x86(lut, in[i]);
}

__global__ void __launch_bounds__(kBlock) k_seed(const uint64_t *in, uint64_t *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = rtk::seed_mix(in[i]);
}

__global__ void __launch_bounds__(kBlock) k_pcg(const uint64_t *in, uint32_t *value, uint64_t *state, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        uint64_t s = in[i];
        value[i] = rtk::pcg(s);
        state[i] = s;
    }
}

// The three (lo, inv) pairs the path draws with: the pixel jitter (-0.5, 0.5), the diffuse bounce's
// (-1, 1) and the dielectric's (0, 1); out[k * n + i] is pair k on state in[i] (each from in[i]).
__global__ void __launch_bounds__(kBlock) k_rand(const uint64_t *in, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        uint64_t s0 = in[i], s1 = in[i], s2 = in[i];
        out[i] = rtk::rand_float(s0, -0.5f, rtk::kInvRange1);
        out[n + i] = rtk::rand_float(s1, -1.0f, rtk::kInvRange2);
        out[2u * n + i] = rtk::rand_float(s2, 0.0f, rtk::kInvRange1);
    }
}

__global__ void __launch_bounds__(kBlock) k_refl(const float *cos_t, const float *r0, float *out, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = rtk::reflectance(cos_t[i], r0[i]);
}

// Device copies of up to three inputs and two outputs of one call, freed on return.
struct Buffers {
    void *p[5] = {};
    int n = 0;
    ~Buffers() {
        for (int k = 0; k < n; ++k) (void)hipFree(p[k]);
    }
    void *alloc(size_t bytes) {
        if (hipMalloc(&p[n], bytes ? bytes : 1) != hipSuccess) return nullptr;
        return p[n++];
    }
    void *upload(const void *host, size_t bytes, int &rc) {
        void *d = alloc(bytes);
        if (!d) rc = rc ? rc : -2;
        else if (hipMemcpy(d, host, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = rc ? rc : -3;
        return d;
    }
    void *output(size_t bytes, int &rc) {
        void *d = alloc(bytes);
        if (!d) rc = rc ? rc : -2;
        return d;
    }
};

inline dim3 grid_of(uint32_t n) { return dim3((n + kBlock - 1u) / kBlock); }

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -4; }

inline int download(void *host, const void *dev, size_t bytes) {
    return hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -5;  // (synchronises)
}

template <typename K>
int unary_f32(K kernel, const float *in, float *out, uint32_t n) {
    if (!in || !out) return -1;
    if (n == 0u) return 0;
    Buffers b;
    int rc = 0;
    const float *d_in = (const float *)b.upload(in, 4ull * n, rc);
    float *d_out = (float *)b.output(4ull * n, rc);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, grid_of(n), dim3(kBlock), 0, nullptr, d_in, d_out, n);
    if ((rc = launched())) return rc;
    return download(out, d_out, 4ull * n);
}

template <typename K>
int binary_f32(K kernel, const float *a, const float *b_in, float *out, uint32_t n) {
    if (!a || !b_in || !out) return -1;
    if (n == 0u) return 0;
    Buffers b;
    int rc = 0;
    const float *d_a = (const float *)b.upload(a, 4ull * n, rc);
    const float *d_b = (const float *)b.upload(b_in, 4ull * n, rc);
    float *d_out = (float *)b.output(4ull * n, rc);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, grid_of(n), dim3(kBlock), 0, nullptr, d_a, d_b, d_out, n);
    if ((rc = launched())) return rc;
    return download(out, d_out, 4ull * n);
}

}  // namespace

extern "C" int math_probe_sqrt(const float *in, float *out, uint32_t n) { return unary_f32(k_sqrt, in, out, n); }

extern "C" int math_probe_rcp(const float *in, float *out, uint32_t n) { return unary_f32(k_rcp, in, out, n); }

extern "C" int math_probe_div(const float *a, const float *b, float *out, uint32_t n) {
    return binary_f32(k_div, a, b, out, n);
}

extern "C" int math_probe_refl(const float *cos_t, const float *r0, float *out, uint32_t n) {
    return binary_f32(k_refl, cos_t, r0, out, n);
}

// out: n pairs {RN(1 / (f32)(pc + 1)), RN((f32)pc / (f32)(pc + 1))}
extern "C" int math_probe_fold(const uint32_t *pc, float *out, uint32_t n) {
    if (!pc || !out) return -1;
    if (n == 0u) return 0;
    Buffers b;
    int rc = 0;
    const uint32_t *d_in = (const uint32_t *)b.upload(pc, 4ull * n, rc);
    float *d_out = (float *)b.output(8ull * n, rc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_fold, grid_of(n), dim3(kBlock), 0, nullptr, d_in, d_out, n);
    if ((rc = launched())) return rc;
    return download(out, d_out, 8ull * n);
}

// in, out: n vectors of three floats
extern "C" int math_probe_normalize(const float *in, float *out, uint32_t n) {
    if (!in || !out) return -1;
    if (n == 0u) return 0;
    Buffers b;
    int rc = 0;
    const float *d_in = (const float *)b.upload(in, 12ull * n, rc);
    float *d_out = (float *)b.output(12ull * n, rc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_normalize, grid_of(n), dim3(kBlock), 0, nullptr, d_in, d_out, n);
    if ((rc = launched())) return rc;
    return download(out, d_out, 12ull * n);
}

// table: the caller's 2048 entries; in_lds picks Lut.in_lds
extern "C" int math_probe_rsqrt(const float *table, const float *in, float *out, uint32_t n, int in_lds) {
    if (!table || !in || !out) return -1;
    if (n == 0u) return 0;
    Buffers b;
    int rc = 0;
    const float *d_table = (const float *)b.upload(table, 4ull * 2048u, rc);
    const float *d_in = (const float *)b.upload(in, 4ull * n, rc);
    float *d_out = (float *)b.output(4ull * n, rc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rsqrt, grid_of(n), dim3(kBlock), 0, nullptr, d_table, d_in, d_out, n, in_lds ? 1u : 0u);
    if ((rc = launched())) return rc;
    return download(out, d_out, 4ull * n);
}

extern "C" int math_probe_seed(const uint64_t *in, uint64_t *out, uint32_t n) {
    if (!in || !out) return -1;
    if (n == 0u) return 0;
    Buffers b;
    int rc = 0;
    const uint64_t *d_in = (const uint64_t *)b.upload(in, 8ull * n, rc);
    uint64_t *d_out = (uint64_t *)b.output(8ull * n, rc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_seed, grid_of(n), dim3(kBlock), 0, nullptr, d_in, d_out, n);
    if ((rc = launched())) return rc;
    return download(out, d_out, 8ull * n);
}

// value[i] = pcg(s), state[i] = s afterwards, for s = in[i]
extern "C" int math_probe_pcg(const uint64_t *in, uint32_t *value, uint64_t *state, uint32_t n) {
    if (!in || !value || !state) return -1;
    if (n == 0u) return 0;
    Buffers b;
    int rc = 0;
    const uint64_t *d_in = (const uint64_t *)b.upload(in, 8ull * n, rc);
    uint32_t *d_value = (uint32_t *)b.output(4ull * n, rc);
    uint64_t *d_state = (uint64_t *)b.output(8ull * n, rc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pcg, grid_of(n), dim3(kBlock), 0, nullptr, d_in, d_value, d_state, n);
    if ((rc = launched())) return rc;
    if ((rc = download(value, d_value, 4ull * n))) return rc;
    return download(state, d_state, 8ull * n);
}

// out: three planes of n floats, (lo, inv) = (-0.5, 1), (-1, 2), (0, 1) over 2^32 - 1
extern "C" int math_probe_rand(const uint64_t *in, float *out, uint32_t n) {
    if (!in || !out) return -1;
    if (n == 0u) return 0;
    Buffers b;
    int rc = 0;
    const uint64_t *d_in = (const uint64_t *)b.upload(in, 8ull * n, rc);
    float *d_out = (float *)b.output(12ull * n, rc);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rand, grid_of(n), dim3(kBlock), 0, nullptr, d_in, d_out, n);
    if ((rc = launched())) return rc;
    return download(out, d_out, 12ull * n);
}
