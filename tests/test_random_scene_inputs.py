"""The inputs of tests/test_gpu_random_scene_kernels.py, checked on the CPU (no GPU needed):
- random_scenes.make(seed) still produces, byte for byte, what it produced before it had overrides
  (tests/golden/random_scene_digests.json);
- each sized or derived input (random_scenes.NAMED) is in the regime it was added for, as the host
  packer sees it (rt.scene_prefilter, rt.scene_clusters, rt.scene_cluster_layout, both rule sets, with
  the grazing spheres added as the GPU tests add them);
- the seeds are in the regimes the GPU tests count on, so that a change of the packer's choices that
  empties one is noticed here and not as a coverage hole on the GPU.
The host bounds of the same scenes are tests/test_random_scene_bounds.py."""
import json
import pathlib
import sys

import numpy as np
import pytest

import random_scenes

sys.path.insert(0, str(pathlib.Path(__file__).with_name("golden")))
from make_random_scene_digests import digest  # noqa: E402

W, H = 40, 24
GOLDEN = pathlib.Path(__file__).with_name("golden") / "random_scene_digests.json"
SQRT_RANGE_MIN = 2.0 ** -36   # rt_kernel.h fast_sqrt: every hittable r^2 is 0 or in [2^-36, 2^60]
CL_MAX_GROUPS = 128           # rt_layout.h kClMaxGroups == kClAutoGroups
MAX_LDS_GROUPS = 164          # rt_kernel.h kMaxLdsGroups
_facts = {}


def facts(rt, orc, name):
    """Per rule set (SIMD, scalar): groups, flags, cluster pairs, levels, sub-cluster pairs, mask words of
    the table's entries, whether the expanded table is in use, the smallest positive r^2; plus the spec."""
    if name not in _facts:
        spec, grazing_seed = random_scenes.named(name)
        spheres = random_scenes.add_grazing_spheres(rt, spec, W, H, seed=grazing_seed)
        look, dist, ang, yh, _ = spec["cameras"][0]
        s, _ = random_scenes.build(rt, orc, spheres, spec["use_sky"], look, dist, ang, yh)
        per_set = []
        for simd in (True, False):
            r2, _, flags = rt.scene_prefilter(s, simd)
            table, pairs = rt.scene_clusters(s, simd)
            levels, sub_pairs = rt.scene_cluster_layout(s, simd)
            groups = len(r2) // 4
            # the mask words follow the group count (rt_pack.cpp cluster_table), and the entry rows the words
            # (rt_layout.h cl_entry_f4: 4 rows at one word, 5 with per-lane thresholds, else 3 + words)
            words = 1 if groups <= 32 else 2 if groups <= 64 else 4
            assert table.shape[1] == ((5 if flags & 4 else 4) if words == 1 else 3 + words)
            per_set.append({"groups": groups, "flags": flags, "pairs": pairs, "levels": levels, "sub_pairs": sub_pairs,
                            "words": words if pairs else 0,
                            "expanded": bool(pairs) and rt.scene_clusters_expanded(s, simd)[2],
                            "min_r2": float(r2[np.isfinite(r2) & (r2 > 0)].min())})
        _facts[name] = (spec, spheres, per_set)
    return _facts[name]


def test_seeds_keep_every_byte():
    """The overrides of make() consume the seed's own draws: seeds 0..55 give the recorded digests."""
    want = json.loads(GOLDEN.read_text())["seeds"]
    assert sorted(want, key=int) == [str(s) for s in range(56)]
    got = {str(s): digest(random_scenes.make(s)) for s in range(56)}
    assert got == want, [s for s in want if got[s] != want[s]]
    # and n_max still fixes the count of the two seeds that draw the maximum
    assert random_scenes.make(18, n_max=400)["n"] == 400 and random_scenes.make(47, n_max=7)["n"] == 7


def test_overrides_fix_count_and_kind():
    for seed in (0, 1, 18):
        for cloud in (True, False):
            spec = random_scenes.make(seed, n=37, cloud=cloud)
            assert spec["n"] == 37 and spec["cloud"] is cloud and spec["spheres"].shape == (37, 20)
            r = spec["spheres"][:, 4] / np.float32(spec["scale"])
            if cloud:  # radii within one decade (0.05 .. 0.3 of the scale; nested pairs only swap radii)
                assert r.min() >= 0.049 and r.max() <= 0.31
    base = random_scenes.make(3)
    same = random_scenes.make(3, n=base["n"], cloud=base["cloud"])
    assert digest(same) == digest(base)


@pytest.mark.parametrize("name", random_scenes.NAMED)
def test_named_input_is_in_its_regime(rt, orc, name):
    spec, spheres, sets = facts(rt, orc, name)
    for f in sets:
        if name == "tiny":
            assert f["flags"] & 2 == 0 and f["min_r2"] < SQRT_RANGE_MIN, f
            assert f["min_r2"] == float(np.float32(random_scenes.TINY_RADIUS) ** 2)
            continue
        assert f["flags"] & 2, f
        assert f["flags"] == (3 if spec["cloud"] else 6), f  # scene-wide prefilter / per-lane thresholds
        if name == "wide400":
            assert len(spheres) == 404 and f["levels"] == 2 and f["words"] == 4 and 61 <= f["sub_pairs"] <= 63, f
        elif name in ("wide130", "cloud130"):  # the first sizes past the table's limit: no table, whatever Clusters says
            assert f["groups"] == 131 and (spec["n"] + 3) // 4 == 130 and f["pairs"] == 0, f
            assert f["groups"] > CL_MAX_GROUPS and f["groups"] <= MAX_LDS_GROUPS
        elif name in ("wide165", "cloud165"):
            assert f["groups"] == 166 and (spec["n"] + 3) // 4 == 165 and f["pairs"] == 0, f
            assert (spec["n"] + 3) // 4 > MAX_LDS_GROUPS
        elif name == "cloud2w":
            assert 32 < f["groups"] <= 64 and f["levels"] == 2 and f["words"] == 2 and f["expanded"], f
        elif name == "cloud4w":
            assert 64 < f["groups"] <= CL_MAX_GROUPS and f["levels"] == 2 and f["words"] == 4 and f["expanded"], f
        else:
            raise AssertionError(name)


def test_seed_regimes(rt, orc):
    """What the GPU tests count on from the 56 seeds (both rule sets agree on every one of these)."""
    words_seen = {"cloud": set(), "wide": set()}
    for seed in range(56):
        spec, _, sets = facts(rt, orc, f"seed{seed}")
        for f in sets:
            # flags 3: scene-wide prefilter, short sqrt; 6: per-lane thresholds, short sqrt.  Never the
            # prefilter off (0 or 2), never outside the short square root's range (bit 1 clear).
            if spec["cloud"]:
                assert f["flags"] == (6 if seed == 14 else 3), (seed, f)
            else:
                assert f["flags"] == (3 if seed == 29 else 6), (seed, f)
            assert f["min_r2"] >= SQRT_RANGE_MIN, (seed, f)
            # group counts: nothing between 65 and 264, so nothing straddles the table's 128 groups or the
            # LDS image's 164; seeds 18 and 47 draw the maximum and get no table
            assert f["groups"] <= 64 or (seed in (18, 47) and f["groups"] == 265 and f["pairs"] == 0), (seed, f)
            assert f["pairs"] <= 13 and f["sub_pairs"] <= 55, (seed, f)
            assert f["words"] <= 2, (seed, f)  # four-word tables come from the sized inputs alone
            if f["pairs"]:
                assert f["expanded"] == (f["flags"] == 3), (seed, f)
                words_seen["cloud" if f["flags"] == 3 else "wide"].add(f["words"])
    assert words_seen == {"cloud": {1, 2}, "wide": {1, 2}}, words_seen
    assert facts(rt, orc, "seed34")[2][0]["min_r2"] == min(facts(rt, orc, f"seed{s}")[2][0]["min_r2"] for s in range(56))


def test_option_inputs_hold_what_they_are_chosen_for(rt, orc):
    """The subset the forced options run on (random_scenes.OPTION_INPUTS; the named inputs among it are
    checked by test_named_input_is_in_its_regime)."""
    f = {name: facts(rt, orc, name) for name in random_scenes.OPTION_INPUTS}
    assert f["seed29"][2][0]["groups"] <= 2                                     # merged rounds
    assert not f["seed1"][0]["cloud"] and f["seed1"][2][0]["groups"] <= 8       # a small wide scene
    spec = f["seed16"][0]                                                        # a wide scene with a huge sphere
    assert not spec["cloud"] and spec["spheres"][:, 4].max() >= 10.0 * spec["scale"]
    assert f["seed3"][0]["cloud"] and f["seed3"][2][0]["levels"] == 1 and f["seed3"][2][0]["groups"] <= 16
    assert f["seed31"][0]["cloud"] and f["seed31"][2][0]["levels"] == 2
    assert f["seed18"][2][0]["groups"] == 265
