// dir_table_check.cpp — the direction table of the scene packer (csrc/rt_pack.cpp direction_table) as a plain
// host program: no HIP, no device.  Links csrc/rt_pack.cpp and csrc/rt_scene.cpp only.  For Floating Spheres
// prefixes and for every scene file named on the command line (rt_scalar_sphere records, 80 bytes each) it
// builds the table of both rule sets through the public queries and prints one line per case: the table's
// shape and a 64-bit FNV-1a of its bytes and of the member entries.  It checks what needs no ray: every row
// holds its own pair's bit, no mask has a bit beyond the scene's pairs, and every direction of a sweep over the
// cube's faces, edges and corners maps to a cell inside the row.  Built with a host sanitizer
// (tests/test_direction_table_standalone.py) the run also checks every index the packer forms.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "rt_trace.h"

// the library's is in rt_host.cpp, beside the error text it sets
int rt_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return code;
}

namespace {

uint64_t fnv1a(const void *data, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    const unsigned char *b = (const unsigned char *)data;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

// A scene of its own spheres, laid out as the built-in ones are (padding lanes zero, one material more
// than spheres), as tests/pack_check builds its own.
struct OwnScene {
    std::vector<rt_scalar_sphere> s;
    std::vector<rt_sphere_group> g;
    std::vector<rt_material> m;
    rt_scene scene;
    OwnScene(const rt_scene &like, std::vector<rt_scalar_sphere> spheres) : s(std::move(spheres)) {
        const uint32_t n = (uint32_t)s.size();
        g.resize((n + 3u) / 4u);
        m.resize(n + 1u);
        memset(g.data(), 0, g.size() * sizeof(g[0]));
        memset(m.data(), 0, m.size() * sizeof(m[0]));
        for (uint32_t i = 0; i < n; ++i) {
            rt_sphere_group &G = g[i / 4u];
            G.X[i % 4u] = s[i].Position.x;
            G.Y[i % 4u] = s[i].Position.y;
            G.Z[i % 4u] = s[i].Position.z;
            G.Radii[i % 4u] = s[i].Radius;
            m[i] = s[i].Material;
        }
        scene = like;
        scene.ScalarSpheres.Data = s.data();
        scene.ScalarSpheres.Count = n;
        scene.SIMDSpheres.Data = g.data();
        scene.SIMDSpheres.Count = (uint32_t)g.size();
        scene.Materials.Data = m.data();
        scene.Materials.Count = n + 1u;
    }
    OwnScene(const OwnScene &) = delete;
};

int check(const std::string &name, const rt_scene &scene, uint32_t simd) {
    uint64_t bytes = 0;
    rt_direction_table_info info;
    if (rt_scene_direction_table(&scene, simd, nullptr, 0, &bytes, &info)) return 1;
    uint32_t member_f4 = 0;
    if (rt_scene_direction_members(&scene, simd, nullptr, 0, &member_f4)) return 1;
    if (bytes == 0) {
        if (member_f4 != 0 || info.Rows != 0) return 1;
        printf("%s simd=%u : none\n", name.c_str(), simd);
        return 0;
    }
    std::vector<unsigned char> tab((size_t)bytes);
    if (rt_scene_direction_table(&scene, simd, tab.data(), bytes, &bytes, &info)) return 1;
    std::vector<float> members((size_t)member_f4 * 4u);
    if (rt_scene_direction_members(&scene, simd, members.data(), member_f4, &member_f4)) return 1;
    const uint32_t n = info.CellsPerEdge;
    if (info.CellsPerRow != 6u * n * n || (info.MaskBits != 32u && info.MaskBits != 64u) ||
        bytes != (uint64_t)info.Rows * info.CellsPerRow * (info.MaskBits / 8u) || member_f4 != 4u * (info.Rows / 2u)) {
        fprintf(stderr, "dir_table_check: %s: inconsistent sizes\n", name.c_str());
        return 1;
    }
    // a capacity one byte short is refused and writes nothing
    if (rt_scene_direction_table(&scene, simd, tab.data(), bytes - 1u, &bytes, &info) == 0) return 1;
    const uint32_t n_pairs = info.Rows / 2u;
    const uint64_t every = n_pairs >= 64u ? ~0ull : (1ull << n_pairs) - 1ull;
    for (uint32_t j = 0; j < info.Rows; ++j)
        for (uint32_t c = 0; c < info.CellsPerRow; ++c) {
            uint64_t m = 0;
            memcpy(&m, &tab[((size_t)j * info.CellsPerRow + c) * (info.MaskBits / 8u)], info.MaskBits / 8u);
            if (!(m >> (j >> 1) & 1ull) || (m & ~every)) {
                fprintf(stderr, "dir_table_check: %s: row %u cell %u mask %llx\n", name.c_str(), j, c, (unsigned long long)m);
                return 1;
            }
        }
    // the cell function stays inside a row for any input: a sweep over the cube, ties, zeros, huge and non-finite values
    const float vals[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, -0.5f, 0.70710678f, -0.70710678f, 0.57735027f, 1e-30f, -1e30f,
                          1e30f, __builtin_inff(), -__builtin_inff(), __builtin_nanf("")};
    for (float x : vals)
        for (float y : vals)
            for (float z : vals)
                if (rt_direction_cell(x, y, z) >= info.CellsPerRow) return 1;
    printf("%s simd=%u : n=%u bits=%u rows=%u : %016llx %016llx\n", name.c_str(), simd, n, info.MaskBits, info.Rows,
           (unsigned long long)fnv1a(tab.data(), tab.size()), (unsigned long long)fnv1a(members.data(), members.size() * 4u));
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    rt_scene floating;
    if (rt_scene_builtin(1, &floating)) return 2;
    int bad = 0;
    for (uint32_t n : {4u, 16u, 33u, 64u, 128u, 129u}) {
        rt_scene s;
        if (rt_scene_prefix(&floating, n, &s)) return 2;
        for (uint32_t simd = 0; simd < 2u; ++simd) bad |= check("floating" + std::to_string(n), s, simd);
    }
    for (int i = 1; i < argc; ++i) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) return 2;
        std::vector<rt_scalar_sphere> sp;
        rt_scalar_sphere one;
        while (fread(&one, sizeof one, 1, f) == 1) sp.push_back(one);
        fclose(f);
        const OwnScene own(floating, sp);
        for (uint32_t simd = 0; simd < 2u; ++simd) bad |= check(argv[i], own.scene, simd);
    }
    return bad;
}
