// pack_check.cpp — the scene packer (csrc/rt_pack.cpp) as a plain host program: no HIP, no device.
// Links csrc/rt_pack.cpp and csrc/rt_scene.cpp only.  For every case of the matrix below it packs
// one rule set and prints one line: the case, the scalar results, and a 64-bit FNV-1a of each
// table's bytes.  Two builds of the packer computed the same tables exactly when their outputs are
// equal; built with a host sanitizer (tests/test_pack_standalone.py) the run also checks every
// index the packer forms.
//   pack_check          the thinned matrix: every scene at the defaults, and every override value
//                       once on a one-word, a two-word and a four-word scene
//   pack_check --full   the whole product scene x rule set x PrefilterRelative x ClusterCount x
//                       SubClusterSpheres
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "rt_pack.h"
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

uint64_t fnv1a(const std::vector<float> &v) {
    uint64_t h = 0xCBF29CE484222325ull;
    const unsigned char *b = (const unsigned char *)v.data();
    for (size_t i = 0; i < v.size() * sizeof(float); ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

// A scene of its own spheres, laid out as the built-in ones are (rt_scene.cpp to_simd: padding
// lanes zero, one material more than spheres).
struct OwnScene {
    std::vector<rt_scalar_sphere> s;
    std::vector<rt_sphere_group> g;
    std::vector<rt_material> m;
    rt_scene scene;
    explicit OwnScene(const rt_scene &like, std::vector<rt_scalar_sphere> spheres) : s(std::move(spheres)) {
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

std::vector<rt_scalar_sphere> spheres_of(const rt_scene &sc, uint32_t n) {
    const rt_scalar_sphere *s = (const rt_scalar_sphere *)sc.ScalarSpheres.Data;
    return std::vector<rt_scalar_sphere>(s, s + n);
}

struct Case {
    std::string name;
    rt_scene scene;
    uint32_t words;  // 0: in the matrix at the defaults only; else the overrides are varied on it too
};

int run(const Case &c, int rs, int pf_rel, uint32_t k, uint32_t sub) {
    PackedSet p;
    const int rc = pack_set(&c.scene, rs, p, pf_rel, k, sub);
    if (rc) {
        fprintf(stderr, "pack_check: %s rs %d: pack_set returned %d\n", c.name.c_str(), rs, rc);
        return 1;
    }
    printf("%s rs=%d pf_rel=%d k=%u sub=%u : groups=%u pays=%d relative=%d fast_sqrt=%u cpairs=%u words=%u levels=%u "
           "sub_pairs=%u x_ok=%d f4=%zu xf4=%zu : %016llx %016llx %016llx %016llx %016llx\n",
           c.name.c_str(), rs, pf_rel, k, sub, p.n_groups, (int)p.prefilter_pays, (int)p.relative, p.fast_sqrt,
           p.cl.n_cpairs, p.cl.words, p.cl.levels, p.cl.sub_pairs, (int)p.cl.x_ok, p.cl.tab.size() / 4u,
           p.cl.xtab.size() / 4u, (unsigned long long)fnv1a(p.groups), (unsigned long long)fnv1a(p.mats),
           (unsigned long long)fnv1a(p.cl.tab), (unsigned long long)fnv1a(p.cl.xtab),
           (unsigned long long)fnv1a(p.cl.own_rho));
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const bool full = argc > 1 && !strcmp(argv[1], "--full");
    rt_scene builtin[3];
    for (uint32_t i = 0; i < 3; ++i)
        if (rt_scene_builtin(i, &builtin[i])) return 2;
    std::vector<Case> cases;
    for (uint32_t i = 0; i < 3; ++i) cases.push_back({"scene" + std::to_string(i), builtin[i], 0u});
    // prefixes: below and at the 8-sphere minimum of a table, scalar padding lanes, one mask word
    // (32 groups), two (33), four (65), and scene 2 short of its last group's last lane
    const struct {
        uint32_t scene, n, words;
    } prefixes[] = {{1, 4, 0}, {1, 7, 0}, {1, 8, 0}, {1, 30, 0}, {1, 128, 1}, {1, 132, 2}, {2, 260, 4}, {2, 481, 0}};
    for (const auto &pf : prefixes) {
        Case c{"scene" + std::to_string(pf.scene) + "_first" + std::to_string(pf.n), {}, pf.words};
        if (rt_scene_prefix(&builtin[pf.scene], pf.n, &c.scene)) return 2;
        cases.push_back(c);
    }
    // a scene-wide scene far from its own origin: the expanded table is built and not in use
    std::vector<rt_scalar_sphere> far = spheres_of(builtin[1], 64);
    for (rt_scalar_sphere &s : far) s.Position.x += 1e4f;
    const OwnScene far_scene(builtin[1], far);
    cases.push_back({"scene1_first64_x1e4", far_scene.scene, 0u});
    // more groups than a table is built for (kClMaxGroups): 9 x 8 x 8 = 576 spheres, 144 groups
    std::vector<rt_scalar_sphere> grid;
    for (uint32_t i = 0; i < 576; ++i) {
        rt_scalar_sphere s = ((const rt_scalar_sphere *)builtin[1].ScalarSpheres.Data)[i % 256u];
        s.Position.x = 0.5f * (float)(i % 9u);
        s.Position.y = 0.5f * (float)(i / 9u % 8u);
        s.Position.z = 0.5f * (float)(i / 72u);
        s.Radius = 0.125f + 0.001f * (float)(i % 7u);
        grid.push_back(s);
    }
    const OwnScene grid_scene(builtin[1], grid);
    cases.push_back({"grid576", grid_scene.scene, 0u});
    // a radius-0 sphere: hittable under the scalar rules (dist == r^2 == 0), never under SIMD
    std::vector<rt_scalar_sphere> zero = spheres_of(builtin[1], 16);
    zero[5].Radius = 0.0f;
    const OwnScene zero_scene(builtin[1], zero);
    cases.push_back({"scene1_first16_r0", zero_scene.scene, 0u});

    const int pf_rels[] = {-1, 0, 1};
    const uint32_t ks[] = {0, 2, 3, 1000}, subs[] = {0, 1, 2, 5};
    int bad = 0;
    for (const Case &c : cases)
        for (int rs = 0; rs < 2; ++rs) {
            if (full) {
                for (int pf : pf_rels)
                    for (uint32_t k : ks)
                        for (uint32_t sub : subs) bad |= run(c, rs, pf, k, sub);
                continue;
            }
            bad |= run(c, rs, -1, 0, 0);
            if (!c.words) continue;
            for (int pf : {0, 1}) bad |= run(c, rs, pf, 0, 0);
            for (uint32_t k : {2u, 3u, 1000u}) bad |= run(c, rs, -1, k, 0);
            for (uint32_t sub : {1u, 2u, 5u}) bad |= run(c, rs, -1, 0, sub);
        }
    return bad;
}
