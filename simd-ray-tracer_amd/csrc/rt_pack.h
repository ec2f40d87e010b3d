// rt_pack.h — the scene packer (rt_pack.cpp): one rule set of a scene in the layout the kernels read
// (rt_layout.h).  Pure CPU arithmetic, no HIP: rt_scene_upload (rt_host.cpp) copies the result to the
// device, the rt_scene_* queries report it, tests/pack_check runs it as a plain host program.
#pragma once
#include <stdint.h>

#include <vector>

#include "rt_trace.h"

// sets rt_last_error()'s text and returns `code` (rt_host.cpp)
int rt_fail(int code, const char *fmt, ...);

// The clustered prefilter table of one rule set (rt_pack.cpp cluster_table).  "No table" (more than
// kClMaxGroups groups, fewer than 8 hittable spheres) is this struct as constructed, with `words` set and
// own_rho one +inf per slot; a per-lane table has no xtab and every rho +inf.  No caller patches it up.
struct ClusterTable {
    std::vector<float> tab;      // the entries: cluster pairs, sub-cluster pairs, member pairs (rt_layout.h)
    std::vector<float> xtab;     // the expanded table of a scene-wide table: the row {c0, 0}, then the entries
    std::vector<float> own_rho;  // per slot: word 3 of the sphere record's centre row (own-sphere rule), else +inf
    uint32_t n_cpairs = 0;       // cluster-pair entries at the start of tab; 0: no table
    uint32_t words = 0;          // u64 words of the pair mask (set without a table too)
    uint32_t levels = 0;         // 1 or 2 (words >= 2); 0: no table
    uint32_t sub_pairs = 0;      // sub-cluster pair entries of a two-level table
    bool x_ok = false;           // xtab proven and useful (the launch fact kPrefilterExpanded)
    // the direction block of a one-word scene-wide table with x_ok (rt_layout.h; rt_pack.cpp direction_table):
    // member entries in pair order, then the mask rows as bit patterns; empty: none
    std::vector<float> dir;
};

// One rule set of a scene: rs 0 = SIMD rules from SIMDSpheres (main.cpp:399-400) + Materials[4g+l]
// (main.cpp:443-444); rs 1 = scalar rules from ScalarSpheres[s].Position/Radius/Material
// (main.cpp:547-590), padding lanes r^2 = -inf (the kernel also skips them by its s < n_spheres test:
// the scalar loop runs to Count).
struct PackedSet {
    std::vector<float> groups, mats;
    uint32_t n_groups = 0;
    bool prefilter_pays = false;
    bool relative = false;  // the threshold row (kRowR2P) rewritten to r^2 / -inf for the per-lane threshold
    uint32_t fast_sqrt = 0;
    ClusterTable cl;
};

// pf_rel_env, cluster_k, sub_spheres (rt_plan.h Switches): rt_device_options PrefilterRelative (-1 auto, 0 never, 1 always),
// ClusterCount and SubClusterSpheres (0: per scene); dir_table: DirectionTable (off builds no direction block)
int pack_set(const rt_scene *scene, int rs, PackedSet &p, int pf_rel_env = -1, uint32_t cluster_k = 0,
             uint32_t sub_spheres = 0, bool dir_table = false);
