"""CPU-side checks of the tile-list entry point (no GPU needed): the header
declares rt_tile_count and rt_trace_tiles and the library exports them, the tile
count is OnRender's ceil division, tiles_of_rect lists what a brute-force
enumeration lists, and rt_trace_tiles refuses a NULL device."""
import ctypes
import re

import numpy as np
import pytest

from test_abi import HEADER, declared_functions


def test_header_declares_and_library_exports_the_tile_entry_points(rt):
    names = declared_functions()
    L = rt.lib()
    for name in ("rt_tile_count", "rt_trace_tiles"):
        assert name in names and name in rt.SIGNATURES and hasattr(L, name), name
    text = HEADER.read_text()
    assert re.search(r"#define\s+RT_TILE_SIZE\s+32u", text) and rt.RT_TILE_SIZE == 32
    # the info struct gained its field at the end, in the header and in the mirror
    body = re.search(r"typedef struct rt_trace_info \{(.*?)\} rt_trace_info;", text, flags=re.S).group(1)
    fields = re.findall(r"^\s*uint(?:32|64)_t\s+(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    assert fields[-1] == "TilesSelected" and fields == [n for n, _ in rt.RtTraceInfo._fields_]


@pytest.mark.parametrize("W,H,count,tiles_x", [(136, 104, 20, 5), (1, 1, 1, 1), (32, 32, 1, 1), (33, 32, 2, 2),
                                               (65536, 65536, 2048 * 2048, 2048), (1920, 1080, 2040, 60),
                                               (0, 17, 0, 0), (17, 0, 0, 0), (65537, 8, 0, 0), (8, 65537, 0, 0)])
def test_tile_count_is_onrenders(rt, W, H, count, tiles_x):
    tx = ctypes.c_uint32(99)
    assert rt.lib().rt_tile_count(W, H, ctypes.byref(tx)) == count and tx.value == tiles_x
    assert rt.lib().rt_tile_count(W, H, None) == count  # out_tiles_x is optional
    assert rt.tile_count(W, H) == count


def _brute_force(W, H, x0, y0, x1, y1):
    ys, xs = np.mgrid[0:H, 0:W]
    inside = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    tiles_x = (W + 31) // 32
    return sorted(set(((ys[inside] // 32) * tiles_x + xs[inside] // 32).tolist()))


def test_tiles_of_rect_matches_a_brute_force_enumeration(rt):
    rng = np.random.default_rng(32)
    cases = [(136, 104, 0, 0, 136, 104), (136, 104, 128, 96, 136, 104), (136, 104, 31, 31, 33, 33),
             (136, 104, 32, 32, 64, 64), (136, 104, 40, 0, 40, 104), (136, 104, -5, -5, 1, 1),
             (136, 104, 130, 100, 500, 500), (136, 104, 200, 0, 300, 10), (1, 1, 0, 0, 1, 1), (33, 32, 32, 0, 33, 32)]
    for W, H in [(136, 104), (37, 91), (64, 64), (95, 33)]:
        for _ in range(12):
            x0, x1 = sorted(rng.integers(-8, W + 8, 2).tolist())
            y0, y1 = sorted(rng.integers(-8, H + 8, 2).tolist())
            cases.append((W, H, x0, y0, x1, y1))
    for c in cases:
        assert rt.tiles_of_rect(*c) == _brute_force(*c), c
    assert rt.tiles_of_rect(136, 104, 0, 0, 136, 104) == list(range(rt.tile_count(136, 104)))
    assert rt.tiles_of_rect(136, 104, 40, 0, 40, 104) == []


def test_trace_tiles_rejects_a_null_device(rt):
    L = rt.lib()
    cam = rt.RtCameraInfo()
    d = rt.RtTraceDesc()
    tiles = (ctypes.c_uint32 * 1)(0)
    assert L.rt_trace_tiles(None, ctypes.byref(cam), ctypes.byref(d), tiles, 1, None, None) == -22
    assert b"NULL argument" in L.rt_last_error()
    assert L.rt_trace_tiles(None, None, None, None, 0, None, None) == -22
