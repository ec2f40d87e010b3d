// rt_pack.cpp — the scene packer: sphere groups, sphere records, prefilter thresholds and the
// clustered prefilter tables of one rule set (rt_layout.h), with the proofs the cluster walk's
// exactness rests on.  Pure CPU arithmetic in f32 / f64 (built with -ffp-contract=off): no HIP call,
// no device state.  Each proof stands above the function that implements it.
#include "rt_pack.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "rt_layout.h"

namespace {

constexpr double kU = 0x1p-24, kK = 0x1p-16;  // u and K of every proof below

// where sphere slot s = 4 * group + lane has its value of row `row` in the group rows
size_t slot_at(uint32_t s, uint32_t row) { return (size_t)(s / 4u) * 4u * kGroupF4 + 4u * row + s % 4u; }

void put_u(float *at, uint32_t v) { memcpy(at, &v, 4); }

void put_material(float *dst, const rt_material &m) {
    dst[0] = m.Color.x;
    dst[1] = m.Color.y;
    dst[2] = m.Color.z;
    dst[3] = m.Specular;
    dst[4] = m.Emissive.x;
    dst[5] = m.Emissive.y;
    dst[6] = m.Emissive.z;
    dst[7] = m.IndexOfRefraction;
    // row 3: the dielectric path's per-material quotients, the reference's own f32 divisions done
    // once here (IEEE, as the kernel's were): eta outside = 1/IOR (main.cpp:463) and Reflectance's
    // r0 = ((1 - eta)/(1 + eta))^2 (main.cpp:292-295) for eta outside and inside (= IOR)
    if (m.IndexOfRefraction != 0.0f) {
        const float ior = m.IndexOfRefraction, eo = 1.0f / ior;
        const float ro = (1.0f - eo) / (1.0f + eo), ri = (1.0f - ior) / (1.0f + ior);
        dst[8] = eo;
        dst[9] = ro * ro;
        dst[10] = ri * ri;
    }
}

// Prefilter thresholds r2p (row 4 of each group) for the secondary-ray
// sphere loop (rtk_walk.h, pair_prefilter).  Secondary origins are hit
// points, i.e. lie within |r_i| of a hittable sphere centre s_i, so
//   M_j = (max_i |s_i - s_j| + |r_i|)^2   (with slack for origin rounding)
// bounds |C|^2 for sphere j, and r2p_j = r^2_j + M_j (32u + 1.01K) rounded
// up (u = 2^-24, K = 2^-16) exceeds the prefilter's error bound.  Spheres
// that can never pass the exact test (SIMD r^2 <= 0, scalar padding) get
// -inf: never flagged.  Returns whether the prefilter pays for this scene
// (thresholds not far above r^2 on average).
bool prefilter_rows(std::vector<float> &gv, uint32_t n_groups, bool simd) {
    std::vector<uint32_t> hit;
    for (uint32_t s = 0; s < 4u * n_groups; ++s) {
        const float r2 = gv[slot_at(s, kRowR2)];
        if (simd ? r2 > 0.0f : r2 >= 0.0f) hit.push_back(s);
    }
    double ratio = 0.0;
    uint32_t n_ratio = 0;
    for (uint32_t j = 0; j < 4u * n_groups; ++j) {
        const float r2 = gv[slot_at(j, kRowR2)];
        float &r2p = gv[slot_at(j, kRowR2P)];
        if (!(simd ? r2 > 0.0f : r2 >= 0.0f) || !std::isfinite(r2)) {
            r2p = -INFINITY;
            continue;
        }
        double reach = 0.0;
        for (uint32_t i : hit) {
            const double dx = (double)gv[slot_at(i, kRowX)] - gv[slot_at(j, kRowX)],
                         dy = (double)gv[slot_at(i, kRowY)] - gv[slot_at(j, kRowY)],
                         dz = (double)gv[slot_at(i, kRowZ)] - gv[slot_at(j, kRowZ)];
            const double ri = std::sqrt((double)gv[slot_at(i, kRowR2)]);
            reach = std::max(reach, std::sqrt(dx * dx + dy * dy + dz * dz) + ri);
        }
        const double m = (reach * 1.001 + 1e-3) * (reach * 1.001 + 1e-3);
        const double e = m * (32.0 * 0x1p-24 + 1.01 * 0x1p-16);
        r2p = std::nextafter((float)((double)r2 + e), INFINITY);
        ratio += std::min(e / std::max((double)r2, 1e-30), 10.0);
        n_ratio += 1;
    }
    return n_ratio > 0 && ratio / n_ratio < 0.5;
}

// Whether every r^2 the exact test can accept is 0 or in [2^-36, 2^60]: then
// a passing candidate's r^2 - dist is 0 or >= 2^-60 (it is >= ulp(r^2)/2 when
// positive), the range where the kernel's short sqrt is verified exact.
uint32_t sqrt_range_ok(const std::vector<float> &gv, uint32_t n_groups, bool simd) {
    for (uint32_t s = 0; s < 4u * n_groups; ++s) {
        const float r2 = gv[slot_at(s, kRowR2)];
        if (!(simd ? r2 > 0.0f : r2 >= 0.0f)) continue;  // never accepted (padding)
        if (r2 != 0.0f && !(r2 >= 0x1p-36f && r2 <= 0x1p60f)) return 0u;
    }
    return 1u;
}

// ---------------------------------------------------------------------------------------------
// The clustered prefilter table (rt_layout.h, cl_entry_f4(words) rows per entry) for the
// secondary-ray sphere loop: the hittable spheres are grouped into about sqrt(n) spatial clusters
// (deterministic k-means; any membership -- the exact test still runs in the reference's group
// order).  A wave skips a cluster when every lane's estimate clears the cluster's threshold
// (cluster_bounds); members of a passing cluster are tested with their own r2p (the per-sphere
// bound of prefilter_rows); a sphere pair some lane may hit sets its bit in the wave's pair mask,
// and the exact recheck walks that mask in group order.  The stages, in the order cluster_table
// runs them: hittable_spheres, choose_k, kmeans, cluster_bounds, behind_of_slot, lay_out,
// own_sphere_rho, expand_table.

// A hittable sphere: its slot, centre, radius and (scene-wide tables) its M.
struct Sph {
    uint32_t s;
    double x, y, z, r, m;
};

// M of point p: the squared reach of every origin (a point on some hittable sphere) from p, with
// the same slack for origin rounding as prefilter_rows
double bound_m(const std::vector<Sph> &sp, double px, double py, double pz) {
    double reach = 0.0;
    for (const Sph &o : sp)
        reach = std::max(reach, std::sqrt((o.x - px) * (o.x - px) + (o.y - py) * (o.y - py) + (o.z - pz) * (o.z - pz)) + o.r);
    return (reach * 1.001 + 1e-3) * (reach * 1.001 + 1e-3);
}

// The spheres some ray can be flagged for (a finite r2p), in slot order; scene-wide tables bound
// every |C_j|^2 by the sphere's M_j, per-lane ("relative") tables leave m 0.
std::vector<Sph> hittable_spheres(const std::vector<float> &gv, uint32_t n_groups, bool relative) {
    std::vector<Sph> sp;
    for (uint32_t s = 0; s < 4u * n_groups; ++s) {
        if (!std::isfinite(gv[slot_at(s, kRowR2P)])) continue;  // never flagged (-inf)
        sp.push_back({s, gv[slot_at(s, kRowX)], gv[slot_at(s, kRowY)], gv[slot_at(s, kRowZ)],
                      std::sqrt((double)std::max(gv[slot_at(s, kRowR2)], 0.0f)), 0.0});
    }
    if (!relative)
        for (Sph &o : sp) o.m = bound_m(sp, o.x, o.y, o.z);
    return sp;
}

// max(1.25 sqrt(n), n/8) clusters: measured on C2 (N = 64) K = 6/8/10/12/16 ->
// 112.4k/113.8k/114.6k/114.5k/111.4k Mrays/s; at 200 spheres K = 17/28 ->
// 45.0k/46.9k; at C5 (256) K = 20/26/32/40 -> 30.1k/31.3k/32.4k/32.4k
// per-lane tables carry the height-slab test, which culls most clusters of a
// ground-plane scene, so fewer (larger) clusters pay there: RTWeekend (482
// spheres) K = 32/40/60/90 -> 17.8k/18.5k/17.8k/16.7k Mrays/s, hence n/12
// Two-level tables (two or more mask words) take fewer, larger top
// clusters over sub-clusters of 3 (scene-wide) or 4 (per-lane) spheres:
// RTWeekend K/S = 40/4, 28/3, 28/4, 24/4 -> 21.1k/21.9k/21.9k/21.7k (one level
// at K 40: 19.6k); C5 at 512 spp K/S = 32/4, 24/3, 28/3, 24/2 -> 47.4k/48.2k/
// 48.3k/48.3k (one level: 46.3k).
// k_override: rt_device_options ClusterCount (A/B; 0: per scene).
uint32_t choose_k(uint32_t n, bool two_levels, bool relative, uint32_t k_override) {
    const uint32_t div = two_levels ? (relative ? 17u : 10u) : (relative ? 12u : 8u);
    const uint32_t k = std::max(2u, std::max((uint32_t)std::lround(1.25 * std::sqrt((double)n)), n / div));
    return k_override ? std::min(n, std::max(2u, k_override)) : k;
}

// One generator serves the top-level k-means and then every sub-cluster k-means, in top-cluster
// order: the tables are a function of the whole draw sequence.
struct Lcg {
    uint64_t state = 0x9E3779B97F4A7C15ull;
    uint32_t operator()(uint32_t m) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((state >> 33) % m);
    }
};

// sigma_j of cluster_bounds' proof: how far from s_j a line some lane accepts sphere j on can pass
double sigma(const Sph &o, bool relative) {
    return relative ? o.r : std::sqrt(o.r * o.r + 13.3 * kU * o.m) + kU * std::sqrt(o.m);
}

// k-means (f64, fixed LCG restarts) of the spheres idx into k clusters,
// minimising the sum of rho_c^2; returns each sphere's label
std::vector<uint32_t> kmeans(const std::vector<Sph> &sp, const std::vector<uint32_t> &idx, uint32_t k, int restarts,
                             bool relative, Lcg &rnd) {
    const uint32_t m = (uint32_t)idx.size();
    std::vector<uint32_t> best_lab(m, 0u);
    double best_cost = INFINITY;
    std::vector<double> cx(k), cy(k), cz(k);
    std::vector<uint32_t> lab(m);
    for (int restart = 0; restart < restarts; ++restart) {
        for (uint32_t c = 0; c < k; ++c) {  // k-means++ style seeding (farthest of a few random picks)
            uint32_t pick = rnd(m);
            double far = -1.0;
            for (int t = 0; t < 4 && c > 0; ++t) {
                const uint32_t cand = rnd(m);
                const Sph &o = sp[idx[cand]];
                double dmin = INFINITY;
                for (uint32_t q = 0; q < c; ++q)
                    dmin = std::min(dmin, (o.x - cx[q]) * (o.x - cx[q]) + (o.y - cy[q]) * (o.y - cy[q]) +
                                              (o.z - cz[q]) * (o.z - cz[q]));
                if (dmin > far) {
                    far = dmin;
                    pick = cand;
                }
            }
            const Sph &o = sp[idx[pick]];
            cx[c] = o.x;
            cy[c] = o.y;
            cz[c] = o.z;
        }
        for (int it = 0; it < 40; ++it) {
            for (uint32_t i = 0; i < m; ++i) {
                const Sph &o = sp[idx[i]];
                double dmin = INFINITY;
                for (uint32_t c = 0; c < k; ++c) {
                    const double d2 = (o.x - cx[c]) * (o.x - cx[c]) + (o.y - cy[c]) * (o.y - cy[c]) +
                                      (o.z - cz[c]) * (o.z - cz[c]);
                    if (d2 < dmin) {
                        dmin = d2;
                        lab[i] = c;
                    }
                }
            }
            std::vector<double> sx(k, 0.0), sy(k, 0.0), sz(k, 0.0), cnt(k, 0.0);
            for (uint32_t i = 0; i < m; ++i) {
                sx[lab[i]] += sp[idx[i]].x;
                sy[lab[i]] += sp[idx[i]].y;
                sz[lab[i]] += sp[idx[i]].z;
                cnt[lab[i]] += 1.0;
            }
            for (uint32_t c = 0; c < k; ++c)
                if (cnt[c] > 0.0) {
                    cx[c] = sx[c] / cnt[c];
                    cy[c] = sy[c] / cnt[c];
                    cz[c] = sz[c] / cnt[c];
                }
        }
        std::vector<double> rho(k, 0.0);
        for (uint32_t i = 0; i < m; ++i) {
            const Sph &o = sp[idx[i]];
            const uint32_t c = lab[i];
            const double d = std::sqrt((o.x - cx[c]) * (o.x - cx[c]) + (o.y - cy[c]) * (o.y - cy[c]) +
                                       (o.z - cz[c]) * (o.z - cz[c]));
            rho[c] = std::max(rho[c], d + sigma(o, relative));
        }
        double cost = 0.0;
        for (uint32_t c = 0; c < k; ++c) cost += rho[c] * rho[c];
        if (cost < best_cost) {
            best_cost = cost;
            best_lab = lab;
        }
    }
    return best_lab;
}

// the spheres idx by label, labels in ascending order, empty ones dropped
std::vector<std::vector<uint32_t>> parts_of(const std::vector<uint32_t> &idx, const std::vector<uint32_t> &lab, uint32_t k) {
    std::vector<std::vector<uint32_t>> parts;
    for (uint32_t c = 0; c < k; ++c) {
        std::vector<uint32_t> part;
        for (size_t i = 0; i < idx.size(); ++i)
            if (lab[i] == c) part.push_back(idx[i]);
        if (!part.empty()) parts.push_back(std::move(part));
    }
    return parts;
}

// A cluster as the table holds it: f32 centre (what the kernel subtracts), exact thresholds.
// As constructed: the padding half of an odd cluster's pair, never entered.
struct Cl {
    float qx = 0.0f, qy = 0.0f, qz = 0.0f, t = -INFINITY;
    float b = 0.0f;                                    // behind threshold
    float srho = 0.0f, ymid = 0.0f, yhalf = INFINITY;  // height-slab bound (per-lane tables)
    std::vector<uint32_t> mem;                         // sphere slots, ascending once sorted
};

// |s_i - q| as every bound below uses it
double delta(const Sph &o, double qx, double qy, double qz) {
    return std::sqrt((o.x - qx) * (o.x - qx) + (o.y - qy) * (o.y - qy) + (o.z - qz) * (o.z - qz));
}

// Scene-wide thresholds.  A cluster c with centre q_c is skipped by a wave when every lane's FMA
// estimate e_c = |Q|^2 - (Q.D)^2, Q = RN(q_c - O), satisfies e_c >= rc2p_c.  Proof that skipping is
// exact (u = 2^-24, K = 2^-16, l(p) = the exact squared distance from point p to the ray's line;
// distance to a line is 1-Lipschitz):
//  - e_c is within M_c (10.2u + K(1+K)/(1-K)) of l(O + Q) (as for spheres,
//    plus the 1/|D|^2 factor of l), M_c a bound on |Q|^2 over every secondary
//    origin; so e_c >= rc2p_c = rho_c^2 + M_c (32u + 1.01K) gives
//    l(O + Q) >= rho_c^2, and |Q - (q_c - O)| <= u sqrt(M_c) moves the point
//    by at most that: sqrt(l(q_c)) >= rho_c - u sqrt(M_c);
//  - member j: sqrt(l(s_j)) >= sqrt(l(q_c)) - |s_j - q_c|, and the
//    reference's rounded C_j moves s_j by <= u sqrt(M_j) again;
//  - the reference-rounded dist_j (exact ops on C_j: >= l(O + C_j)) is within
//    13.3u M_j of its exact value, so l(O + C_j) > sigma_j^2 = r_j^2 + 13.3u M_j
//    makes dist_j > r_j^2: a miss under both rule sets.
// Hence rho_c = max_j (|s_j - q_c| + sigma_j + u sqrt(M_j)) + u sqrt(M_c),
// inflated by 1e-6 relative.
// Behind: a member j cannot be accepted by a ray whose computed
// T_j + X_j stays below eps (it = T - X or T + X < eps), and X_j <= r_j(1+2u).
// With T_j within 4.2u sqrt(M_j)|D| of (S_j - O).D (one rounding in C_j, three
// in the dot) and the prefilter's FMA T_c within 4u sqrt(M_c)|D| of (q_c - O).D,
// (S_j - O).D <= (q_c - O).D + |S_j - q_c||D| gives: T_c < -b_c with
//   b_c = max_j (|S_j - q_c| + r_j)(1 + 2^-15) + 4.3u (sqrt(M_c) + sqrt(M_j))
// proves every member is behind every origin-side candidate (|D| <= 1 + 2^-17
// under the |D|^2 bound).
void scene_wide_bounds(Cl &C, const std::vector<Sph> &sp, const std::vector<uint32_t> &idx) {
    const double qx = C.qx, qy = C.qy, qz = C.qz;
    double rho = 0.0;
    for (uint32_t i : idx) rho = std::max(rho, delta(sp[i], qx, qy, qz) + sigma(sp[i], false));
    const double mc = bound_m(sp, qx, qy, qz);
    rho = (rho + kU * std::sqrt(mc)) * (1.0 + 1e-6);
    C.t = std::nextafter((float)(rho * rho + mc * (32.0 * kU + 1.01 * kK)), INFINITY);
    double bmax = 0.0;
    for (uint32_t i : idx)
        bmax = std::max(bmax, (delta(sp[i], qx, qy, qz) + sp[i].r) * (1.0 + 0x1p-15) +
                                  4.3 * kU * (std::sqrt(mc) + std::sqrt(sp[i].m)));
    C.b = std::nextafter((float)-bmax, -INFINITY);
}

// Per-lane ("relative") thresholds, where the scene-wide M makes the bound above useless (pack_set):
// they are formed per lane from the lane's own cc = |Q|^2 (rtk_walk.h kClRel / kPfRel / kBehindRel).
// With A_j = |Q|(1+u) + delta_j >= |C_j| (delta_j = |s_j - q_c|) the chain above reads
//   sqrt(l(O+Q)) > delta_j + sqrt(r_j^2 + 13.3u A_j^2) + 2u A_j + u|Q|
// and sqrt(r^2 + 13.3u A^2) <= r + sqrt(13.3u) A, so it holds when
//   sqrt(l(O+Q)) > rho_j + a|Q|,  rho_j = delta_j (1+s) + r_j,  s = sqrt(13.3u) + 2u,  a = s(1+u) + u;
// (rho + a|Q|)^2 <= rho^2 (1+a) + |Q|^2 (a + a^2), l(O+Q) >= e_c - E1 |Q|^2
// (E1 = 10.2u + K(1+K)/(1-K)) and |Q|^2 <= cc (1 + 5.1u), so the cluster is
// skipped when e_c >= RN(cc kClRel + R_c), R_c = rho_c^2 (1+a) rounded up,
// kClRel >= (a + a^2 + E1)(1 + 6u) (both inflated for the FMA's rounding).
// Members carry r^2 (the group rows' per-lane rule), behind thresholds lose
// their M terms (|Q|, |C_j| <= (1 + cc)/2 bound them per lane, kBehindRel):
//   cluster  -(max_j ((delta_j + r_j)(1 + 2^-15) + 4.3u delta_j) + 4.3u),
//   member   -(r_j (1 + 2^-15) + 4.3u),
// and a lane's behind test is T < RN(stored - 4.5u cc).
// Height slab.  A lane can accept member j only if its exact line passes
// within sigma_j = sqrt(r_j^2 + 13.3u |C_j|^2) <= r_j + k_s |C_j| of s_j
// (k_s = sqrt(13.3u) = 8.9e-4; the reference-rounded dist error, as above),
// so at some t with |O + tD - q_c| <= rho_s + k_s |C_j|, rho_s = max_j
// (delta_j + r_j), and height within [y_lo - k_s|C_j|, y_hi + k_s|C_j|]
// (y_lo/y_hi the members' extent).  Along the line the height O.y + t D.y
// over that t range lies within c +- |D.y| rho' (c = O.y + D.y T, T the
// projection of q_c): if |c - ymid| > yhalf + |D.y| rho' + E the line misses
// every member.  |C_j| <= |Q| + delta_j, |Q| <= (1 + cc)/2: the delta_j part
// is folded into srho / yhalf here, the |Q| part (twice, for height and t
// range) and the rounding of T, c, d and thr (< 2^-14 (1 + cc) + u |O.y|)
// into the kernel's per-lane E = cc kSlabRel + |O.y| 2^-21 + kSlabRel,
// kSlabRel = 2^-9 >= 2 (8.9e-4 (1.0001) / 2 + 2^-14).
void per_lane_bounds(Cl &C, const std::vector<Sph> &sp, const std::vector<uint32_t> &idx) {
    const double qx = C.qx, qy = C.qy, qz = C.qz;
    const double s_rel = std::sqrt(13.3 * kU) + 2.0 * kU, a_rel = s_rel * (1.0 + kU) + kU;
    double rho = 0.0, bmax = 0.0;
    for (uint32_t i : idx) {
        rho = std::max(rho, delta(sp[i], qx, qy, qz) * (1.0 + s_rel) + sp[i].r);
        bmax = std::max(bmax, (delta(sp[i], qx, qy, qz) + sp[i].r) * (1.0 + 0x1p-15) + 4.3 * kU * delta(sp[i], qx, qy, qz));
    }
    C.t = std::nextafter((float)(rho * rho * (1.0 + a_rel) * (1.0 + 1e-6)), INFINITY);
    C.b = std::nextafter((float)(-(bmax + 4.3 * kU) * (1.0 + 1e-6)), -INFINITY);
    double rs = 0.0, yhi = -INFINITY, ylo = INFINITY;
    for (uint32_t i : idx) {
        rs = std::max(rs, delta(sp[i], qx, qy, qz) + sp[i].r);
        yhi = std::max(yhi, sp[i].y + sp[i].r);
        ylo = std::min(ylo, sp[i].y - sp[i].r);
    }
    const double ks = 8.91e-4;
    C.srho = std::nextafter((float)(rs * (1.0 + ks) * (1.0 + 0x1p-12)), INFINITY);
    C.ymid = (float)((yhi + ylo) * 0.5);
    const double half = std::max(yhi - (double)C.ymid, (double)C.ymid - ylo) + ks * rs;
    C.yhalf = std::nextafter((float)(half * (1.0 + 0x1p-12)), INFINITY);
}

// The bound rows of a cluster over the spheres idx (any set: a top cluster's
// bound covers every sphere under it, as a sub-cluster's covers its members).
Cl cluster_bounds(const std::vector<Sph> &sp, const std::vector<uint32_t> &idx, bool relative) {
    Cl C;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t i : idx) {
        sx += sp[i].x;
        sy += sp[i].y;
        sz += sp[i].z;
    }
    C.qx = (float)(sx / idx.size());
    C.qy = (float)(sy / idx.size());
    C.qz = (float)(sz / idx.size());
    if (relative) per_lane_bounds(C, sp, idx);
    else scene_wide_bounds(C, sp, idx);
    for (uint32_t i : idx) C.mem.push_back(sp[i].s);
    return C;
}

// The clusters of both levels.  Second level (tables of two or more mask words: the kernel walks
// one-word tables, at most 32 groups, as one level -- rtk_walk.h clustered_groups): each top
// cluster's spheres in sub-clusters of about sub_spheres (k-means inside the top cluster); sub[c]
// is empty in a one-level table.  Both lists are padded to whole pairs.
struct Clusters {
    std::vector<Cl> top;
    std::vector<std::vector<Cl>> sub;
};
Clusters make_clusters(const std::vector<Sph> &sp, uint32_t k, bool two_levels, uint32_t sub_spheres, bool relative) {
    Lcg rnd;
    std::vector<uint32_t> all((uint32_t)sp.size());
    for (uint32_t i = 0; i < all.size(); ++i) all[i] = i;
    const std::vector<std::vector<uint32_t>> tops = parts_of(all, kmeans(sp, all, k, 16, relative, rnd), k);
    Clusters cs;
    for (const auto &idx : tops) cs.top.push_back(cluster_bounds(sp, idx, relative));
    if (cs.top.size() & 1u) cs.top.push_back(Cl{});
    cs.sub.resize(cs.top.size());
    if (two_levels)
        for (size_t c = 0; c < tops.size(); ++c) {
            const std::vector<uint32_t> &idx = tops[c];
            const uint32_t k2 = std::min((uint32_t)idx.size(), ((uint32_t)idx.size() + sub_spheres - 1u) / sub_spheres);
            if (k2 <= 1u) {
                cs.sub[c].push_back(cluster_bounds(sp, idx, relative));
            } else {
                for (const auto &part : parts_of(idx, kmeans(sp, idx, k2, 8, relative, rnd), k2))
                    cs.sub[c].push_back(cluster_bounds(sp, part, relative));
            }
            if (cs.sub[c].size() & 1u) cs.sub[c].push_back(Cl{});
        }
    for (Cl &C : cs.top) std::sort(C.mem.begin(), C.mem.end());
    for (auto &v : cs.sub)
        for (Cl &C : v) std::sort(C.mem.begin(), C.mem.end());
    return cs;
}

// Behind thresholds per slot: cluster_bounds' behind proofs with q_c = S_j.  Scene-wide
// b_j = r_j(1 + 2^-15) + 8.6u sqrt(M_j); per lane r_j (1 + 2^-15) + 4.3u.
std::vector<float> behind_of_slot(const std::vector<Sph> &sp, uint32_t n_groups, bool relative) {
    std::vector<float> behind(4u * n_groups, 0.0f);
    for (const Sph &o : sp)
        behind[o.s] = relative ? std::nextafter((float)(-(o.r * (1.0 + 0x1p-15) + 4.3 * kU) * (1.0 + 1e-6)), -INFINITY)
                               : std::nextafter((float)-(o.r * (1.0 + 0x1p-15) + 8.6 * kU * std::sqrt(o.m)), -INFINITY);
    return behind;
}

// Laying the entries out (rt_layout.h): cluster pairs, then the sub-cluster pairs of each top
// cluster, then member pairs in the order their clusters are reached.
struct Writer {
    std::vector<float> &tab;
    const std::vector<float> &gv, &behind;
    uint32_t ef;  // floats per entry
    bool relative;
    uint32_t next;  // the next free member-pair entry
    float *entry(uint32_t e) { return &tab[(size_t)e * ef]; }
};

// the bound rows of a cluster pair entry (both levels)
void put_pair(Writer &w, uint32_t p, const Cl &A, const Cl &B) {
    float *e = w.entry(p);
    const Cl *half[2] = {&A, &B};
    for (uint32_t h = 0; h < 2u; ++h) {
        const Cl &C = *half[h];
        e[cl_centre(0u, h)] = C.qx, e[cl_centre(1u, h)] = C.qy, e[cl_centre(2u, h)] = C.qz;
        e[cl_threshold(h)] = C.t;
        e[cl_behind(h)] = C.b;
        if (w.relative) e[cl_srho(h)] = C.srho, e[cl_ymid(h)] = C.ymid, e[cl_yhalf(h)] = C.yhalf;
    }
}

// the member pair entries of cluster C from entry w.next on, and their range in half h of entry e
void put_members(Writer &w, uint32_t e, uint32_t h, const Cl &C) {
    const uint32_t cnt = ((uint32_t)C.mem.size() + 1u) / 2u;
    put_u(&w.entry(e)[cl_first(h)], w.next);
    put_u(&w.entry(e)[cl_count(h)], cnt);
    for (uint32_t q = 0; q < cnt; ++q, ++w.next) {
        float *m = w.entry(w.next);
        for (uint32_t mh = 0; mh < 2u; ++mh) {
            const uint32_t idx = 2u * q + mh;
            if (idx >= C.mem.size()) {
                m[cl_threshold(mh)] = -INFINITY;  // padding member: never flagged, no bit
                continue;
            }
            const uint32_t s = C.mem[idx];
            m[cl_centre(0u, mh)] = w.gv[slot_at(s, kRowX)];
            m[cl_centre(1u, mh)] = w.gv[slot_at(s, kRowY)];
            m[cl_centre(2u, mh)] = w.gv[slot_at(s, kRowZ)];
            // member threshold: the scene-wide r2p, or r^2 for the per-lane rule
            m[cl_threshold(mh)] = w.gv[slot_at(s, w.relative ? kRowR2 : kRowR2P)];
            m[cl_behind(mh)] = w.behind[s];
            if (!w.relative) put_u(&m[cl_slot(mh)], s);  // its slot (the own-sphere rule)
            // the u64 bit of pair q = s >> 1 in the row of word q >> 6 (the other words' rows stay 0)
            const uint64_t bit = 1ull << ((s >> 1) & 63u);
            float *bits = &m[cl_bits((s >> 1) >> 6) + 2u * mh];
            put_u(bits, (uint32_t)bit);
            put_u(bits + 1, (uint32_t)(bit >> 32));
        }
    }
}

// Returns the entry counts {cluster pairs, sub-cluster pairs, member pairs}.
struct Counts {
    uint32_t cp, sp, mp;
};
Counts lay_out(const Clusters &cs, bool two_levels, const std::vector<float> &gv, const std::vector<float> &behind,
               uint32_t words, bool relative, std::vector<float> &tab) {
    Counts n{(uint32_t)cs.top.size() / 2u, 0u, 0u};
    for (size_t c = 0; c < cs.top.size(); ++c) {
        n.sp += (uint32_t)cs.sub[c].size() / 2u;
        for (const Cl &S : cs.sub[c]) n.mp += ((uint32_t)S.mem.size() + 1u) / 2u;
        if (!two_levels) n.mp += ((uint32_t)cs.top[c].mem.size() + 1u) / 2u;
    }
    const uint32_t ef = cl_entry_f4(words, relative) * 4u;
    tab.assign((size_t)(n.cp + n.sp + n.mp) * ef, 0.0f);
    Writer w{tab, gv, behind, ef, relative, n.cp + n.sp};
    uint32_t next_sub = n.cp;
    for (uint32_t p = 0; p < n.cp; ++p) {
        put_pair(w, p, cs.top[2u * p], cs.top[2u * p + 1u]);
        for (uint32_t h = 0; h < 2u; ++h) {
            const size_t c = 2u * p + h;
            if (!two_levels) {
                put_members(w, p, h, cs.top[c]);
                continue;
            }
            // a top cluster: its sub-cluster pair entries, then their members
            const uint32_t first = next_sub, cnt = (uint32_t)cs.sub[c].size() / 2u;
            put_u(&w.entry(p)[cl_first(h)], first);
            put_u(&w.entry(p)[cl_count(h)], cnt);
            next_sub += cnt;
            for (uint32_t q = 0; q < cnt; ++q) {
                put_pair(w, first + q, cs.sub[c][2u * q], cs.sub[c][2u * q + 1u]);
                for (uint32_t h2 = 0; h2 < 2u; ++h2) put_members(w, first + q, h2, cs.sub[c][2u * q + h2]);
            }
        }
    }
    return n;
}

// Own sphere (scene-wide tables; rtk_walk.h own_sphere).  A lane that continues a path from sphere j
// (slot j: word 2 / 3 of row 3 of j's member entry) leaves j out of its own member flags when
//   |d| < RN(-T lambda),   d = RN(rho_j - cc kappa),   kappa = 1 - 320u,  lambda = 1.9 eps,
// with C = RN(S_j - O) per axis -- the reference's own C_j, bit for bit -- and the FMA values
// cc ~ |C|^2, T ~ C.D of pair_prefilter; rho_j = r_j^2 (the f32 the exact test compares with; word 3
// of the record's centre row) for the table's members with r_j^2 in [kOwnR2Min, kOwnR2Max], else +inf
// (d = +inf or NaN: never).  Everything below is a function of C, D and r_j^2 alone, so nothing is
// assumed about the segment that led to O (its length, its direction's norm, which root was taken, how
// O was rounded): the test measures how far O lies off the sphere instead of bounding it.
// Claim: under the rule the reference's candidate j (main.cpp:413-429, 561-578) is rejected by both
// rule sets whatever the running minima are: if dist_r <= r^2 at all, then RN(T_r - X_r) < eps and
// RN(T_r + X_r) < eps strictly (SIMD accepts only it > eps, scalar only !(it < eps)).
// With a = |C|, c* = a^2, T* = C.D exact, |D|^2 = 1 + k, |k| <= K = 2^-16, u = 2^-24:
//  (1) the lane's values: cc within 3.01u c* of c*, T within 3.01u a|D| of T*.  The rule gives T < 0
//      and |d| < 2.001 a eps, so |r^2 - c*| <= 2.01 a eps + 324u c*: with r in [16.1 eps, 16],
//      14.9 eps <= a <= 16.01 (no product underflows, and 3.01u a <= 0.029 eps);
//  (2) the reference: T_r = dot3 within 3.01u a of T*; its dist_r (exact ops on C) is within 8u c* of
//      |C - D T_r|^2 >= c* - T*^2 / (1 + k) (q's two roundings 4.1u c*, the dot's three 3.1u c*:
//      the 13.3u M term above with M = c*), so
//        r^2 - dist_r <= r^2 - c* (1 - 8u - 1.03K) + T*^2;
//      X_r = RN(sqrt(RN(r^2 - dist_r))) <= sqrt((r^2 - dist_r)(1 + 3.3u)), and by (1)
//      3.3u (r^2 - dist_r) <= 3.4u c* + 6.7u a eps, so X_r^2 <= T*^2 + Delta,
//        Delta = r^2 - c* (1 - 11.4u - 1.03K) + 6.7u a eps;
//  (3) kappa: cc kappa <= c* (1 + 3.01u)(1 - 320u) <= c* (1 - 316u), and 1.03K + 11.4u = 275.1u, so
//      rho - cc kappa >= Delta + 40u c*  (6.7u a eps <= 0.45u c* by a >= 14.9 eps);
//  (4) Delta <= 0: X_r <= |T*|, T_r + X_r <= 3.01u a <= 0.029 eps.  Else sqrt(T*^2 + Delta) <=
//      |T*| + Delta / (2|T*|) and the rule gives Delta + 40u c* <= d (1 + u) < |T| lambda (1 + 2.1u)
//      <= (|T*| + 3.01u a) lambda (1 + 2.1u), where 3.01u a lambda (1 + 2.1u) <= 0.4u c* is inside the
//      40u c*: Delta < |T*| lambda (1 + 2.1u), hence
//        T_r + X_r <= 3.01u a + lambda (1 + 2.1u) / 2 <= 0.029 eps + 0.9501 eps < eps (1 - 2u),
//      and RN of a sum below eps (1 - 2u) is below eps; T_r - X_r <= T_r + X_r.  dist_r == r^2 (the
//      scalar rules' hit) has X_r = 0 and T_r <= 0.029 eps + T* < eps.
// The square root is the reference's correctly rounded one; the kernel's own candidate code is not
// involved -- a dropped lane runs no candidate for j unless another lane flags the pair, and then its
// exact test reproduces this rejection.  tests/test_own_sphere_skip.py checks the claim on rays formed
// as the reference forms them.
constexpr float kOwnR2Min = 2.6e-6f, kOwnR2Max = 256.0f;  // r in [16.1 eps, 16]
void own_sphere_rho(const std::vector<Sph> &sp, const std::vector<float> &gv, std::vector<float> &own_rho) {
    for (const Sph &o : sp) {
        const float r2 = gv[slot_at(o.s, kRowR2)];
        if (r2 >= kOwnR2Min && r2 <= kOwnR2Max) own_rho[o.s] = r2;
    }
}

// Expanded (scene-wide tables; rtk_walk.h pair_prefilter_x, the walk-specialised kernels).  A second table
// t.xtab of the same entries, in front of it one row {c0, 0}: c0 = the midpoint of the bounding box of all
// entry centres (cluster and member; f32).  Centres are S' = RN(S - c0), the kernel forms O' = RN(O - c0),
//   T^ = fma(S'x, Dx, fma(S'y, Dy, fma(S'z, Dz, p))),          p = -RN-chain(O'.D)
//   A^ = fma(S'x, -2O'x, fma(S'y, -2O'y, fma(S'z, -2O'z, oo))), oo = RN-chain(|O'|^2)
//   e' = fma(-T^, T^, A^)
// and skips on e' >= t' = RN+(t - |S'|^2 + G), t the entry's threshold above; behind on T^ < b' = b - H.
// Mask rows, ranges, slots and rho are copied.  Bounds: a = max |S'| over the entries, b >= |O'| over every
// origin (each lies on a scene sphere: sqrt(bound_m(c0)), the slack of M included), R = a + b, m = sqrt(M) of
// the entry (M_j or M_c above: |C| <= m), C^ = S' - O' as a real vector.  Roundings (u each, |D| <= 1 + K/2):
//  - S' and O': |C^ - (S - O)| <= u (|S'| + |O'|) <= u R, so |C^ - C_r| <= 1.01u (R + m) =: d for the
//    reference's C_r = RN(S - O), and |C^| <= m (1 + 1e-3) inside M's own slack (R <= 10m where the table is used, below);
//  - the chains: p and oo carry three roundings of partial sums <= |O'||D| and |O'|^2: 3.01u b|D|, 3.01u b^2;
//    T^ adds three of partial sums <= (a + b)|D|:  |T^ - C^.D| <= 3.01u (a + 2b)|D| =: eT;
//    A^ adds three of partial sums <= b^2 + 2ab:    |A^ - (|C^|^2 - |S'|^2)| <= u (6.02 b^2 + 6.02 ab);
//  - the product T^2 is exact inside the last FMA, whose one rounding is of |A^ - T^2| <= max(a, m)^2 (1.01):
//    u 1.01 max(a, m)^2;  and |T^2 - (C^.D)^2| <= eT (2|C^||D| + eT) <= 6.1u (a + 2b) m.
//   Hence e' + |S'|^2 is within  u (6.02 b^2 + 6.02 ab + 1.01 max(a, m)^2 + 6.1 (a + 2b) m)  of f(C^) = |C^|^2 - (C^.D)^2.
//  - f(C^) - l(O + C^) = (C^.D)^2 (1 - 1/|D|^2), at most K|C^|^2 <= K M (1 + 2.1e-3) in size;
//  - member j: sqrt(l(O + C_r)) >= sqrt(l(O + C^)) - d, i.e. l(O + C_r) >= l(O + C^) - 2 d m - d^2, and the
//    reference's dist_j >= l(O + C_r) - 13.3u M_j as above: the M-only terms (K (1 + 2.1e-3) + 13.3u + 2.02u) M_j
//    (K + 15.9u) stay inside E_j = M_j (32u + 1.01K), which t already holds, and what is left is
//      G >= u (6.02 b^2 + 6.02 ab + 1.01 max(a, m)^2 + 6.1 (a + 2b) m + 2.02 R m) + d^2;
//  - cluster c: the proof above needs sqrt(l(q_c)) >= rho_c - u sqrt(M_c); now the point moves by u R 1.01, so
//    it needs l(O + Q^) >= (rho_c + 1.01u R)^2, and rho_c <= 1.01 m: 2.05u R m more, M-only terms K M_c (1 + 2.1e-3).
//  G = 1.25 u (6.02 b^2 + 6.02 ab + 1.01 max(a, m)^2 + 6.1 (a + 2b) m + 2.1 R m) per entry covers both (the head-room
//  of 32u over the 23.5u derived above; d^2 <= 1.1 u^2 (R + m)^2 vanishes in it).  t' is rounded up after
//  t - |S'|^2 + G is formed in f64 (|S'|^2 exact to 2^-52); t itself was rounded up.
//  - behind: T^ is within eT + u R |D| <= u (4.02a + 7.03b)(1 + K) of (S - O).D where the proofs above allowed
//    the prefilter's T 4u sqrt(M)|D|; H = u (4.5a + 7.5b) lowers every b by the whole new error (the old
//    allowance is kept as slack), rounded down.
// t.x_ok (the launch fact "proven and useful", rt_kernel.h kPrefilterExpanded): every value of the table is
// finite; G <= E/4 for every entry, E = M (32u + 1.01K) the slack already in t -- so the expanded form flags
// at most what a threshold 1.25 E would, and R <= 10m as used above; and the scene lies near the origin of
// its own coordinates.  The last is the premise's own margin: recentring makes G itself independent of where
// the scene lies, but "every origin lies on a scene sphere" holds for an f32 origin only to its rounding,
// (sqrt(3)/2) ulp(L) with L = max_i (|s_i|_inf + r_i), which M's slack (1e-3 + 1e-3 reach) was sized to absorb
// for scenes near the origin and which the step |C^| <= m (1 + 1e-3) above draws on once more.  The expanded
// table is used only where that rounding is below 1e-4, a tenth of the slack's absolute part (L < 1024);
// a scene placed far from its own extent's scale keeps the plain table and the run-time kernel.
// Every entry half with a finite threshold is a real cluster or member; padding halves keep centre 0 and
// -inf (never entered, never flagged).
void expand_table(const std::vector<Sph> &sp, uint32_t n_ent, uint32_t ef, ClusterTable &t) {
    const std::vector<float> &tab = t.tab;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t e = 0; e < n_ent; ++e)
        for (uint32_t w = 0; w < 2u; ++w) {
            const float *en = &tab[(size_t)e * ef];
            if (!std::isfinite(en[cl_threshold(w)])) continue;
            for (uint32_t ax = 0; ax < 3u; ++ax) {
                lo[ax] = std::min(lo[ax], (double)en[cl_centre(ax, w)]);
                hi[ax] = std::max(hi[ax], (double)en[cl_centre(ax, w)]);
            }
        }
    const float c0[3] = {(float)(0.5 * (lo[0] + hi[0])), (float)(0.5 * (lo[1] + hi[1])), (float)(0.5 * (lo[2] + hi[2]))};
    t.xtab.assign(4u + tab.size(), 0.0f);
    float *xt = t.xtab.data() + 4u;
    memcpy(xt, tab.data(), tab.size() * sizeof(float));
    for (int ax = 0; ax < 3; ++ax) t.xtab[(size_t)ax] = c0[ax];
    double ra = 0.0;  // a = max |S'|
    for (uint32_t e = 0; e < n_ent; ++e)
        for (uint32_t w = 0; w < 2u; ++w) {
            float *en = xt + (size_t)e * ef;
            if (!std::isfinite(en[cl_threshold(w)])) continue;
            double ss = 0.0;
            for (uint32_t ax = 0; ax < 3u; ++ax) {
                en[cl_centre(ax, w)] = (float)((double)en[cl_centre(ax, w)] - (double)c0[ax]);  // S' = RN(S - c0)
                ss += (double)en[cl_centre(ax, w)] * en[cl_centre(ax, w)];
            }
            ra = std::max(ra, std::sqrt(ss));
        }
    const double rb = std::sqrt(bound_m(sp, c0[0], c0[1], c0[2])) * (1.0 + 1e-6);  // b >= |O'|
    double place = 0.0;  // L = the largest coordinate an origin can have
    for (const Sph &o : sp) place = std::max(place, std::max(std::fabs(o.x), std::max(std::fabs(o.y), std::fabs(o.z))) + o.r);
    const float place_f = (float)place;
    const double origin_rounding = 0.8661 * ((double)std::nextafter(place_f, INFINITY) - (double)place_f);
    bool ok = std::isfinite(ra) && std::isfinite(rb) && origin_rounding <= 1e-4;
    for (uint32_t e = 0; e < n_ent; ++e)
        for (uint32_t w = 0; w < 2u; ++w) {
            const float *src = &tab[(size_t)e * ef];
            float *en = xt + (size_t)e * ef;
            const uint32_t x = cl_centre(0u, w), y = cl_centre(1u, w), z = cl_centre(2u, w);
            const uint32_t thr = cl_threshold(w), beh = cl_behind(w);
            if (!std::isfinite(src[thr])) continue;
            const double mm = bound_m(sp, src[x], src[y], src[z]), m = std::sqrt(mm);
            const double am = std::max(ra, m);
            const double g = 1.25 * kU * (6.02 * rb * rb + 6.02 * ra * rb + 1.01 * am * am + 6.1 * (ra + 2.0 * rb) * m +
                                          2.1 * (ra + rb) * m);
            const double ss = (double)en[x] * en[x] + (double)en[y] * en[y] + (double)en[z] * en[z];
            en[thr] = std::nextafter((float)((double)src[thr] - ss + g), INFINITY);
            en[beh] = std::nextafter((float)((double)src[beh] - kU * (4.5 * ra + 7.5 * rb)), -INFINITY);
            ok = ok && g <= 0.25 * mm * (32.0 * kU + 1.01 * kK) && std::isfinite(en[x]) && std::isfinite(en[y]) &&
                 std::isfinite(en[z]) && std::isfinite(en[thr]) && std::isfinite(en[beh]);
        }
    t.x_ok = ok && std::isfinite(c0[0]) && std::isfinite(c0[1]) && std::isfinite(c0[2]);
}

// Direction table (one-word scene-wide tables with x_ok; rt_layout.h has the layout and the cell function
// dir_cell, rtk_walk.h direction_groups the walk).  Row j, cell c holds bit i >> 1 for every hittable sphere i
// that some ray of the premise below can be accepted on; a lane tests the member entries of its row's bits
// only, so a clear bit must be a proven miss under both rule sets.
// Premise of a lane that reads row j, cell c: (a) |D|^2 = 1 + k, |k| <= K = 2^-16 (every prefiltered round);
// (b) c = dir_cell(D); (c) |O - S_j| <= R_j = 1.008 r_j, with S_j, r_j^2 the f32 values of the sphere record.
// (c) is not assumed of the path: the lane measures it (rtk_walk.h origin_near: |rho_j - cc kOwnCc| < rho_j 2^-6 with
// cc the FMA value of |RN(S_j - O)|^2, within 3.01u of it, and RN(S_j - O) within u per axis of S_j - O, so
// |O - S_j|^2 <= r_j^2 (1 + 2^-6) / ((1 - 1.9e-5)(1 - 4u)) < (1.0079 r_j)^2) and reads all-ones where the test fails
// or rho_j is +inf.  (The width 2^-6: a hit point formed with |D|^2 = 1 + k over a segment of length t lies k t^2
// off the sphere in squared distance, a few 1e-5 at C2 against r^2 / 64 >= 1e-3.)
// Origins inside ball j (dielectric paths) are covered: (c) bounds the distance from above only.
// Cell (cell_cone).  The face fixes the sign and the axis of the major component m, |m| >= |a|, |b| for the two minor
// ones.  Index i of a minor component v is floor(fma(v, kDirScale, kDirHalf)) clamped to [0, kDirN): the FMA is within
// half an ulp of a value below 16, 2^-21, of v kDirScale + kDirHalf, i.e. v is within 2^-21 / kDirScale < 5e-8 of
// [(i - kDirHalf) / kDirScale, (i + 1 - kDirHalf) / kDirScale): the interval is widened by 1e-6 and, for the two end
// indices the clamp feeds, opened to the bound |v| <= sqrt((1 + K)/2) that |m| >= |v| and (a) give.  Host and device
// run the same IEEE operations (dir_cell is one function), so there is no other index error to cover.  With
// m^2 = 1 + k - a^2 - b^2, interval arithmetic over the two intervals and |m| >= min|a|, min|b| gives
// |m| in [m_lo, m_hi]; an empty range means no direction of (a) reaches the cell, and the cell is all-ones
// (reachability is no premise).  Otherwise every D of the cell lies within delta = |(ha, hb, hm)| (the three
// half-widths) of the centre vector Cc, so its angle to Cc is at most alpha = asin(delta / |Cc|) (+ 1e-3 rad for
// the f64 arithmetic here); delta >= |Cc| makes the cell all-ones.
// Sphere i != j.  A lane that accepts i has dist_r <= r_i^2 and RN(T_r + X_r) >= eps > 0 (it = T - X or T + X, both
// rule sets).  With l the exact squared distance of S_i from the lane's line and T* = (S_i - O).D/|D|: the
// reference-rounded dist_r >= l - 13.3u M_i and C_i = RN(S_i - O) moves S_i by u sqrt(M_i) (cluster_bounds), so
// X_r^2 <= (r_i^2 - l + 13.4u M_i)(1 + 4u), and T_r is within 4.2u sqrt(M_i)|D| of the exact dot, so
// T* > -(X_r + 4.3u sqrt(M_i)).  The point of the ray (t >= 0) nearest S_i is at t = max(T*, 0): at T* >= 0 its
// squared distance is l <= r_i^2 + 13.4u M_i, at T* < 0 it is l + T*^2 <= l + (X_r + 4.3u sqrt(M_i))^2.  Either way
// the forward ray meets the ball of radius s_i = (sigma_i + 6u sqrt(M_i))(1 + 2^-15) about S_i (sigma_i as in
// cluster_bounds; the factor covers 4u, the cross term and |D| within 2^-17 of 1).  So D points from a point O of
// ball(S_j, R_j) to a point P of ball(S_i, s_i): with V = S_i - S_j, L = |V|, P - O = V + w, |w| <= rho = s_i + R_j,
// and the angle theta between D and V has sin(theta) <= rho / L and cos(theta) > 0 when rho < L: theta <= A =
// asin(rho / L); L <= rho allows every direction (O may lie inside ball i).
// Bit i >> 1 is set when theta_c - alpha <= A, theta_c the angle of Cc to V, tested on cosines (A + alpha < pi).
// rho is inflated by 1e-6.
// M_i bounds |C_i|^2 over every origin on a scene sphere: the premise every scene-wide table rests on
// (prefilter_rows, scene_wide_bounds), with the launch fact x_ok's "coordinates below 1024" for its slack.
// Sphere j itself and its pair partner: the own-pair bit is always set.  A slot that is not hittable, or whose
// record's rho is not r^2 (own_sphere_rho's range), has an all-ones row.
// n = 16: C2 (64 spheres) tests 7.7 member entries per secondary round in place of 5 cluster and 8.9 member
// entries (profiles/r20a_dir_walk_stats.txt); the rows are 6 x 16 x 16 u32 = 6 KB per sphere, 384 KB at C2, and
// building them takes 21 ms per rule set there, four times cluster_table's 5.5 ms: n = 32 would quadruple both.
struct CellCone {
    double x = 0.0, y = 0.0, z = 0.0, cos_a = 1.0, sin_a = 0.0;
    bool all = true;
};
CellCone cell_cone(uint32_t face, uint32_t ia, uint32_t ib) {
    const double vmax = std::sqrt((1.0 + kK) * 0.5) + 1e-6;
    double lo[2], hi[2], h[2], c[2], sq_min[2], sq_max[2];
    const uint32_t idx[2] = {ia, ib};
    CellCone cone;
    for (int t = 0; t < 2; ++t) {
        lo[t] = idx[t] == 0u ? -vmax : ((double)idx[t] - (double)kDirHalf) / (double)kDirScale - 1e-6;
        hi[t] = idx[t] == kDirN - 1u ? vmax : ((double)idx[t] + 1.0 - (double)kDirHalf) / (double)kDirScale + 1e-6;
        lo[t] = std::max(lo[t], -vmax);
        hi[t] = std::min(hi[t], vmax);
        if (lo[t] > hi[t]) return cone;
        h[t] = 0.5 * (hi[t] - lo[t]);
        c[t] = 0.5 * (hi[t] + lo[t]);
        sq_max[t] = std::max(lo[t] * lo[t], hi[t] * hi[t]);
        sq_min[t] = lo[t] <= 0.0 && hi[t] >= 0.0 ? 0.0 : std::min(lo[t] * lo[t], hi[t] * hi[t]);
    }
    double m_lo = std::sqrt(std::max(0.0, 1.0 - kK - sq_max[0] - sq_max[1]));
    m_lo = std::max(m_lo, std::sqrt(std::max(sq_min[0], sq_min[1])));
    const double m_hi = std::sqrt(std::max(0.0, 1.0 + kK - sq_min[0] - sq_min[1]));
    if (m_hi < m_lo) return cone;
    const double hm = 0.5 * (m_hi - m_lo), mc = (face & 1u ? -0.5 : 0.5) * (m_hi + m_lo);
    const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + mc * mc);
    const double delta = std::sqrt(h[0] * h[0] + h[1] * h[1] + hm * hm);
    if (!(delta < len)) return cone;
    const double alpha = std::asin(delta / len) + 1e-3;
    if (!(alpha < 1.5)) return cone;
    // dir_cell's axes: face 0/1 major x (a = y, b = z), 2/3 major y (a = x, b = z), 4/5 major z (a = x, b = y)
    const double a = c[0] / len, b = c[1] / len, m = mc / len;
    switch (face >> 1) {
        case 0: cone.x = m, cone.y = a, cone.z = b; break;
        case 1: cone.x = a, cone.y = m, cone.z = b; break;
        default: cone.x = a, cone.y = b, cone.z = m; break;
    }
    cone.cos_a = std::cos(alpha);
    cone.sin_a = std::sin(alpha);
    cone.all = false;
    return cone;
}

void direction_table(const std::vector<Sph> &sp, const std::vector<float> &gv, uint32_t n_groups, uint32_t first_member,
                     uint32_t n_ent, uint32_t ef, ClusterTable &t) {
    const bool wide = dir_mask64(n_groups);
    const uint32_t words = wide ? 2u : 1u, n_slots = 4u * n_groups;
    const size_t rows_at = 4u * (size_t)dir_member_f4(n_groups);
    t.dir.assign(dir_block_floats(n_groups), 0.0f);
    // the member entries in pair order, each half copied from the expanded table's own entry of its sphere
    for (uint32_t p = 0; p < 2u * n_groups; ++p)
        for (uint32_t h = 0; h < 2u; ++h) t.dir[(size_t)p * ef + cl_threshold(h)] = -INFINITY;
    const float *xt = t.xtab.data() + 4u;
    for (uint32_t e = first_member; e < n_ent; ++e)
        for (uint32_t h = 0; h < 2u; ++h) {
            const float *src = xt + (size_t)e * ef;
            if (!std::isfinite(src[cl_threshold(h)])) continue;
            uint32_t s;
            memcpy(&s, &src[cl_slot(h)], 4);
            float *dst = &t.dir[(size_t)(s >> 1) * ef];
            const uint32_t dh = s & 1u;
            for (uint32_t ax = 0; ax < 3u; ++ax) dst[cl_centre(ax, dh)] = src[cl_centre(ax, h)];
            dst[cl_threshold(dh)] = src[cl_threshold(h)];
            dst[cl_behind(dh)] = src[cl_behind(h)];
            dst[cl_slot(dh)] = src[cl_slot(h)];
            memcpy(&dst[cl_bits(0u) + 2u * dh], &src[cl_bits(0u) + 2u * h], 8);
        }
    std::vector<CellCone> cones(kDirCells);
    for (uint32_t c = 0; c < kDirCells; ++c) cones[c] = cell_cone(c / (kDirN * kDirN), c / kDirN % kDirN, c % kDirN);
    std::vector<uint64_t> row(kDirCells);
    const uint64_t valid = n_groups == 32u ? ~0ull : (1ull << (2u * n_groups)) - 1ull;  // the pairs there are entries for
    std::vector<const Sph *> of_slot(n_slots, nullptr);
    for (const Sph &o : sp) of_slot[o.s] = &o;
    for (uint32_t j = 0; j < n_slots; ++j) {
        const Sph *oj = of_slot[j];
        const bool measured = oj && std::isfinite(t.own_rho[j]);  // (the lane's test of (c) can pass)
        std::fill(row.begin(), row.end(), measured ? 1ull << (j >> 1) : ~0ull);
        for (uint32_t c = 0; measured && c < kDirCells; ++c)
            if (cones[c].all) row[c] = ~0ull;
        for (size_t ii = 0; measured && ii < sp.size(); ++ii) {
            const Sph &oi = sp[ii];
            if (oi.s == j) continue;
            const uint64_t bit = 1ull << (oi.s >> 1);
            const double rj = std::sqrt((double)gv[slot_at(j, kRowR2)]) * 1.008;
            const double vx = oi.x - oj->x, vy = oi.y - oj->y, vz = oi.z - oj->z, len = std::sqrt(vx * vx + vy * vy + vz * vz);
            const double rho = ((sigma(oi, false) + 6.0 * kU * std::sqrt(oi.m)) * (1.0 + 0x1p-15) + rj) * (1.0 + 1e-6);
            if (!(rho < len)) {
                for (uint64_t &m : row) m |= bit;
                continue;
            }
            const double sa = rho / len, ca = std::sqrt(1.0 - sa * sa);
            const double ux = vx / len, uy = vy / len, uz = vz / len;
            for (uint32_t c = 0; c < kDirCells; ++c) {
                const CellCone &k = cones[c];
                if (k.all) continue;
                // cos(theta_c) >= cos(A + alpha)
                if (ux * k.x + uy * k.y + uz * k.z >= ca * k.cos_a - sa * k.sin_a - 1e-9) row[c] |= bit;
            }
        }
        float *out = &t.dir[rows_at + (size_t)j * kDirCells * words];
        for (uint32_t c = 0; c < kDirCells; ++c) {
            const uint32_t lo = (uint32_t)(row[c] & valid), hi = (uint32_t)((row[c] & valid) >> 32);
            put_u(out + (size_t)c * words, lo);
            if (wide) put_u(out + (size_t)c * words + 1u, hi);
        }
    }
}

// The table of the packed group rows gv (prefilter_rows done).  relative: per-lane thresholds.
// k_override / sub_override: rt_device_options ClusterCount / SubClusterSpheres (0: per scene).
// No table (n_cpairs 0; the result is then as constructed, with `words` set and every rho +inf)
// beyond kClMaxGroups groups and below 8 hittable spheres.  Only a scene-wide table has rho and
// the expanded table, and only a one-word one whose expanded table is in use the direction block
// (dir_table: rt_device_options DirectionTable off builds none).
ClusterTable cluster_table(const std::vector<float> &gv, uint32_t n_groups, bool relative, uint32_t k_override,
                           uint32_t sub_override, bool dir_table) {
    ClusterTable t;
    t.own_rho.assign(4u * (size_t)n_groups, INFINITY);
    t.words = n_groups <= 32u ? 1u : n_groups <= 64u ? 2u : 4u;
    if (n_groups > kClMaxGroups) return t;
    const std::vector<Sph> sp = hittable_spheres(gv, n_groups, relative);
    const uint32_t n = (uint32_t)sp.size();
    if (n < 8u) return t;
    const bool two_levels = t.words >= 2u;
    // sub-clusters of 3 (scene-wide) or 4 (per-lane) spheres (choose_k's measurements)
    const uint32_t sub_spheres = sub_override ? sub_override : relative ? 4u : 3u;
    const Clusters cs = make_clusters(sp, choose_k(n, two_levels, relative, k_override), two_levels, sub_spheres, relative);
    const Counts cnt = lay_out(cs, two_levels, gv, behind_of_slot(sp, n_groups, relative), t.words, relative, t.tab);
    if (!relative) {
        own_sphere_rho(sp, gv, t.own_rho);
        const uint32_t n_ent = cnt.cp + cnt.sp + cnt.mp, ef = cl_entry_f4(t.words, relative) * 4u;
        expand_table(sp, n_ent, ef, t);
        if (dir_table && t.x_ok && t.words == 1u) direction_table(sp, gv, n_groups, cnt.cp + cnt.sp, n_ent, ef, t);
    }
    t.n_cpairs = cnt.cp;
    t.levels = two_levels ? 2u : 1u;
    t.sub_pairs = cnt.sp;
    return t;
}

}  // namespace

int pack_set(const rt_scene *scene, int rs, PackedSet &p, int pf_rel_env, uint32_t cluster_k, uint32_t sub_spheres,
             bool dir_table) {
    const uint32_t ng = scene->SIMDSpheres.Count;
    const uint32_t ns = scene->ScalarSpheres.Count;
    if (ng == 0 || !scene->SIMDSpheres.Data || !scene->Materials.Data || ns == 0 || !scene->ScalarSpheres.Data)
        return rt_fail(RT_EINVAL, "scene: empty scene");
    const uint32_t ngs = (ns + 3u) / 4u;
    if (ng > kMaxGroups || ngs > kMaxGroups)
        return rt_fail(RT_EINVAL, "scene: %u spheres exceed the limit of %u", ns, 4u * kMaxGroups);
    const uint32_t n = rs == 0 ? ng : ngs;
    p.n_groups = n;
    p.groups.assign((size_t)n * 4 * kGroupF4, 0.0f);
    p.mats.assign((size_t)n * 16u * kSphereF4, 0.0f);  // sphere records (rt_layout.h kSphereF4)
    std::vector<float> &gv = p.groups;
    if (rs == 0) {
        const rt_sphere_group *g = (const rt_sphere_group *)scene->SIMDSpheres.Data;
        const rt_material *m = (const rt_material *)scene->Materials.Data;
        for (uint32_t s = 0; s < 4u * ng; ++s) {
            const uint32_t i = s / 4u, l = s % 4u;
            gv[slot_at(s, kRowX)] = g[i].X[l];
            gv[slot_at(s, kRowY)] = g[i].Y[l];
            gv[slot_at(s, kRowZ)] = g[i].Z[l];
            gv[slot_at(s, kRowR2)] = g[i].Radii[l] * g[i].Radii[l];
            float *rec = &p.mats[(size_t)s * 4u * kSphereF4];
            rec[0] = g[i].X[l];
            rec[1] = g[i].Y[l];
            rec[2] = g[i].Z[l];
            if (s < scene->Materials.Count) put_material(rec + 4, m[s]);
        }
    } else {
        const rt_scalar_sphere *s = (const rt_scalar_sphere *)scene->ScalarSpheres.Data;
        for (uint32_t i = 0; i < ns; ++i) {
            gv[slot_at(i, kRowX)] = s[i].Position.x;
            gv[slot_at(i, kRowY)] = s[i].Position.y;
            gv[slot_at(i, kRowZ)] = s[i].Position.z;
            gv[slot_at(i, kRowR2)] = s[i].Radius * s[i].Radius;
            float *rec = &p.mats[(size_t)i * 4u * kSphereF4];
            rec[0] = s[i].Position.x;
            rec[1] = s[i].Position.y;
            rec[2] = s[i].Position.z;
            put_material(rec + 4, s[i].Material);
        }
        for (uint32_t i = ns; i < ngs * 4u; ++i) gv[slot_at(i, kRowR2)] = -INFINITY;
    }
    p.prefilter_pays = prefilter_rows(gv, n, rs == 0);
    p.fast_sqrt = sqrt_range_ok(gv, n, rs == 0);
    // Where the scene-wide bound M_j makes r2p useless (a huge sphere: RTWeekend's
    // ground), the thresholds are formed per lane from the lane's own |C|^2 instead
    // (rtk_walk.h kPfRel, kClRel): the cluster table is built for that rule, and
    // the threshold row (kRowR2P) then holds r^2 (-inf: never hit).
    p.relative = pf_rel_env == 1 || (pf_rel_env < 0 && !p.prefilter_pays);
    p.cl = cluster_table(gv, n, p.relative, cluster_k, sub_spheres, dir_table);
    // (a record per real sphere of the scalar set, per slot of the SIMD set; without a table every rho is +inf)
    for (uint32_t sl = 0; sl < (rs == 0 ? 4u * n : ns); ++sl) p.mats[(size_t)sl * 4u * kSphereF4 + 3u] = p.cl.own_rho[sl];
    if (p.relative)
        for (uint32_t sl = 0; sl < 4u * n; ++sl)
            gv[slot_at(sl, kRowR2P)] = std::isfinite(gv[slot_at(sl, kRowR2P)]) ? gv[slot_at(sl, kRowR2)] : -INFINITY;
    return RT_OK;
}

// ---------------------------------------------------------------------------------------------
// The queries of include/rt_trace.h: what rt_scene_upload derives for one rule set at the default
// options, no device involved.  Each checks its arguments and packs the rule set:
// (only rt_scene_direction_table builds the direction block)
static int query(const char *who, bool args_ok, const rt_scene *scene, uint32_t enable_simd, PackedSet &p,
                 bool dir_table = false) {
    if (!args_ok) return rt_fail(RT_EINVAL, "%s: NULL argument", who);
    return pack_set(scene, enable_simd ? 0 : 1, p, -1, 0, 0, dir_table);
}

extern "C" int rt_scene_prefilter(const rt_scene *scene, uint32_t enable_simd, float *out_r2, float *out_r2p,
                                  uint32_t capacity, uint32_t *out_count, uint32_t *out_flags) {
    PackedSet p;
    if (const int rc = query("rt_scene_prefilter", scene && out_count, scene, enable_simd, p)) return rc;
    const uint32_t n = 4u * p.n_groups;
    *out_count = n;
    if (out_flags) *out_flags = (p.prefilter_pays ? 1u : 0u) | (p.fast_sqrt ? 2u : 0u) | (p.relative ? 4u : 0u);
    if ((out_r2 || out_r2p) && capacity < n) return rt_fail(RT_EINVAL, "rt_scene_prefilter: capacity %u < %u", capacity, n);
    for (uint32_t s = 0; s < n; ++s) {
        if (out_r2) out_r2[s] = p.groups[slot_at(s, kRowR2)];
        if (out_r2p) out_r2p[s] = p.groups[slot_at(s, kRowR2P)];
    }
    return RT_OK;
}

extern "C" int rt_scene_own_sphere(const rt_scene *scene, uint32_t enable_simd, float *out_rho, uint32_t capacity,
                                   uint32_t *out_count) {
    PackedSet p;
    if (const int rc = query("rt_scene_own_sphere", scene && out_count, scene, enable_simd, p)) return rc;
    const uint32_t n = 4u * p.n_groups;
    *out_count = n;
    if (out_rho && capacity < n) return rt_fail(RT_EINVAL, "rt_scene_own_sphere: capacity %u < %u", capacity, n);
    for (uint32_t s = 0; out_rho && s < n; ++s) out_rho[s] = p.cl.own_rho[s];
    return RT_OK;
}

extern "C" int rt_scene_groups(const rt_scene *scene, uint32_t enable_simd, float *out, uint32_t capacity_f4,
                               uint32_t *out_f4, uint32_t *out_rows) {
    PackedSet p;
    if (const int rc = query("rt_scene_groups", scene && out_f4, scene, enable_simd, p)) return rc;
    const uint32_t nf4 = p.n_groups * kGroupF4;
    *out_f4 = nf4;
    if (out_rows) {
        const uint32_t rows[6] = {kGroupF4, kRowX, kRowY, kRowZ, kRowR2, kRowR2P};
        memcpy(out_rows, rows, sizeof rows);
    }
    if (out) {
        if (capacity_f4 < nf4) return rt_fail(RT_EINVAL, "rt_scene_groups: capacity %u < %u", capacity_f4, nf4);
        memcpy(out, p.groups.data(), (size_t)nf4 * 16u);
    }
    return RT_OK;
}

extern "C" int rt_scene_clusters(const rt_scene *scene, uint32_t enable_simd, float *out, uint32_t capacity_f4,
                                 uint32_t *out_f4, uint32_t *out_cpairs) {
    PackedSet p;
    if (const int rc = query("rt_scene_clusters", scene && out_f4 && out_cpairs, scene, enable_simd, p)) return rc;
    const uint32_t nf4 = (uint32_t)(p.cl.tab.size() / 4u);
    *out_f4 = nf4;
    *out_cpairs = p.cl.n_cpairs;
    if (out) {
        if (capacity_f4 < nf4) return rt_fail(RT_EINVAL, "rt_scene_clusters: capacity %u < %u", capacity_f4, nf4);
        memcpy(out, p.cl.tab.data(), (size_t)nf4 * 16u);
    }
    return RT_OK;
}

extern "C" int rt_scene_clusters_expanded(const rt_scene *scene, uint32_t enable_simd, float *out, uint32_t capacity_f4,
                                          uint32_t *out_f4, float *out_c0, uint32_t *out_in_use) {
    PackedSet p;
    if (const int rc = query("rt_scene_clusters_expanded", scene && out_f4 && out_c0 && out_in_use, scene, enable_simd, p))
        return rc;
    const uint32_t nf4 = p.cl.xtab.empty() ? 0u : (uint32_t)(p.cl.xtab.size() / 4u) - 1u;
    *out_f4 = nf4;
    *out_in_use = p.cl.x_ok ? 1u : 0u;
    for (int ax = 0; ax < 3; ++ax) out_c0[ax] = nf4 ? p.cl.xtab[(size_t)ax] : 0.0f;
    if (out) {
        if (capacity_f4 < nf4) return rt_fail(RT_EINVAL, "rt_scene_clusters_expanded: capacity %u < %u", capacity_f4, nf4);
        if (nf4) memcpy(out, p.cl.xtab.data() + 4u, (size_t)nf4 * 16u);
    }
    return RT_OK;
}

extern "C" int rt_scene_cluster_layout(const rt_scene *scene, uint32_t enable_simd, uint32_t *out_levels,
                                       uint32_t *out_sub_pairs) {
    PackedSet p;
    if (const int rc = query("rt_scene_cluster_layout", scene && out_levels && out_sub_pairs, scene, enable_simd, p)) return rc;
    *out_levels = p.cl.levels;
    *out_sub_pairs = p.cl.sub_pairs;
    return RT_OK;
}

extern "C" int rt_scene_direction_table(const rt_scene *scene, uint32_t enable_simd, void *out, uint64_t capacity_bytes,
                                        uint64_t *out_bytes, rt_direction_table_info *info) {
    PackedSet p;
    if (const int rc = query("rt_scene_direction_table", scene && out_bytes && info, scene, enable_simd, p, true)) return rc;
    const bool have = !p.cl.dir.empty();
    const size_t rows_at = have ? 4u * (size_t)dir_member_f4(p.n_groups) : 0u;
    const uint64_t bytes = have ? (uint64_t)(p.cl.dir.size() - rows_at) * 4u : 0u;
    *out_bytes = bytes;
    info->CellsPerEdge = have ? kDirN : 0u;
    info->MaskBits = have ? (dir_mask64(p.n_groups) ? 64u : 32u) : 0u;
    info->Rows = have ? 4u * p.n_groups : 0u;
    info->CellsPerRow = have ? kDirCells : 0u;
    if (out && bytes) {
        if (capacity_bytes < bytes)
            return rt_fail(RT_EINVAL, "rt_scene_direction_table: capacity %llu < %llu", (unsigned long long)capacity_bytes,
                           (unsigned long long)bytes);
        memcpy(out, p.cl.dir.data() + rows_at, (size_t)bytes);
    }
    return RT_OK;
}

extern "C" int rt_scene_direction_members(const rt_scene *scene, uint32_t enable_simd, float *out, uint32_t capacity_f4,
                                          uint32_t *out_f4) {
    PackedSet p;
    if (const int rc = query("rt_scene_direction_members", scene && out_f4, scene, enable_simd, p, true)) return rc;
    const uint32_t nf4 = p.cl.dir.empty() ? 0u : dir_member_f4(p.n_groups);
    *out_f4 = nf4;
    if (out && nf4) {
        if (capacity_f4 < nf4) return rt_fail(RT_EINVAL, "rt_scene_direction_members: capacity %u < %u", capacity_f4, nf4);
        memcpy(out, p.cl.dir.data(), (size_t)nf4 * 16u);
    }
    return RT_OK;
}

extern "C" uint32_t rt_direction_cell(float dx, float dy, float dz) { return dir_cell(dx, dy, dz); }
