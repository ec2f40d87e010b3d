"""Reaching the scheduling kernels of the built librt_trace.so alone (test helper).  rtk_launch_tile_sort,
rtk_tile_sort_scratch, rtk_launch_xcd_group and rtk_launch_sum_u64 take only pointers and integers and are called in
the package's loaded library itself; rtk_launch_pixel_sort takes a TraceArgs, which tests/sched_probe/
libsched_probe.so (tests/sched_probe/sched_probe.cpp, built by __graft_entry__.build() and linked against the
library) fills from plain arguments.  No kernel is compiled a second time: what runs is what ships.

Every function takes and returns numpy arrays and works on torch device tensors.  Every buffer a kernel may write
is allocated with GUARD_WORDS words of a pattern behind it, and the call fails if one of them changed."""
import ctypes
import pathlib

import numpy as np

LIB_PATH = pathlib.Path(__file__).resolve().parent / "sched_probe" / "libsched_probe.so"
GUARD_WORDS = 64
GUARD_BYTE = 0xA5
_RT = None
_P = None


def libs():
    """(librt_trace.so as the package loaded it, libsched_probe.so), with the argument types of what is called."""
    global _RT, _P
    if _P is None:
        if not LIB_PATH.exists():
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        import torch  # noqa: F401  (one HIP runtime per process: tests/math_probe.py's rule)
        import __graft_entry__ as graft
        rt = graft.load_package().lib()  # first, so that the probe's dependency is this very library
        v, u32, u64, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
        for name, res, args in (("rtk_tile_sort_scratch", ctypes.c_size_t, [u32]),
                                ("rtk_launch_tile_sort", i, [v, v, v, u32, v]),
                                ("rtk_launch_xcd_group", i, [v, v, u32, v, v, v, v]),
                                ("rtk_launch_sum_u64", i, [v, u32, v, v])):
            fn = getattr(rt, name)
            fn.restype = res
            fn.argtypes = args
        p = ctypes.CDLL(str(LIB_PATH))
        p.sched_probe_pixel_sort.restype = i
        p.sched_probe_pixel_sort.argtypes = [u32, u32, i, u32, v, v, u32, v, u32, v, v]
        # the probe must have bound to the library the package loaded, not to a second copy of it
        with open("/proc/self/maps") as maps:
            mapped = {line.split()[-1] for line in maps if "/librt_trace" in line}
        if len(mapped) != 1:
            raise RuntimeError(f"libsched_probe.so resolved a second librt_trace.so: {sorted(mapped)}")
        _RT, _P = rt, p
    return _RT, _P


class Buf:
    """A device buffer of `data`'s bytes with a guard behind it.  (Allocated as bytes: any offset or size goes.)"""

    def __init__(self, data, offset=0):
        import torch
        self.host = np.ascontiguousarray(data)
        raw = self.host.view(np.uint8).reshape(-1)
        self.n = raw.size
        full = np.full(offset + self.n + 4 * GUARD_WORDS, GUARD_BYTE, np.uint8)
        full[offset:offset + self.n] = raw
        self.offset = offset
        self.t = torch.from_numpy(full).cuda()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.offset

    def read(self):
        """The buffer's contents now, in the dtype and shape it was made from; raises if the guard changed."""
        full = self.t.cpu().numpy()
        lo, hi = full[:self.offset], full[self.offset + self.n:]
        if not (np.all(lo == GUARD_BYTE) and np.all(hi == GUARD_BYTE)):
            bad = np.flatnonzero(hi != GUARD_BYTE)
            raise AssertionError(f"guard overwritten: {len(bad)} bytes behind the buffer, first at +{bad[:1]}, "
                                 f"{np.count_nonzero(lo != GUARD_BYTE)} in front")
        return full[self.offset:self.offset + self.n].view(self.host.dtype).reshape(self.host.shape).copy()


def _stream_and_sync():
    import torch
    return torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def sort_scratch_bytes(n: int) -> int:
    return int(libs()[0].rtk_tile_sort_scratch(n))


def tile_sort(cost):
    """(order, cost afterwards) of rtk_launch_tile_sort over the n costs."""
    rt, _ = libs()
    cost = np.ascontiguousarray(cost, np.uint32)
    n = len(cost)
    d_cost, d_order = Buf(cost), Buf(np.full(n, 0xDDDDDDDD, np.uint32))
    d_scratch = Buf(np.full(sort_scratch_bytes(n) // 4, 0xCCCCCCCC, np.uint32))
    stream, sync = _stream_and_sync()
    _ok(rt.rtk_launch_tile_sort(d_cost.ptr, d_order.ptr, d_scratch.ptr, n, stream), "rtk_launch_tile_sort")
    sync()
    d_scratch.read()
    return d_order.read(), d_cost.read()


def xcd_group(order_in, live_tiles: int):
    """(order_out, order_in afterwards) of rtk_launch_xcd_group, buffers sized as the host sizes them."""
    rt, _ = libs()
    order_in = np.ascontiguousarray(order_in, np.uint32)
    n = len(order_in)
    n_tiles = (n + 3) // 4
    d_in, d_out = Buf(order_in), Buf(np.full(n, 0xDDDDDDDD, np.uint32))
    d_live = Buf(np.array([live_tiles], np.uint64))
    d_scratch = Buf(np.full(sort_scratch_bytes(n) // 4, 0xCCCCCCCC, np.uint32))
    d_aux = Buf(np.full(2 * n_tiles, 0xBBBBBBBB, np.uint32))
    stream, sync = _stream_and_sync()
    _ok(rt.rtk_launch_xcd_group(d_in.ptr, d_out.ptr, n, d_live.ptr, d_scratch.ptr, d_aux.ptr, stream),
        "rtk_launch_xcd_group")
    sync()
    d_scratch.read(), d_aux.read()
    assert int(d_live.read()[0]) == live_tiles
    return d_out.read(), d_in.read()


def sum_u64(slots, dst: int) -> int:
    """dst after rtk_launch_sum_u64(slots, len(slots), &dst)."""
    rt, _ = libs()
    slots = np.ascontiguousarray(slots, np.uint64)
    d_slots, d_dst = Buf(slots), Buf(np.array([dst], np.uint64))
    stream, sync = _stream_and_sync()
    _ok(rt.rtk_launch_sum_u64(d_slots.ptr, len(slots), d_dst.ptr, stream), "rtk_launch_sum_u64")
    sync()
    assert np.array_equal(d_slots.read(), slots)
    return int(d_dst.read()[0])


def pixel_sort(P, W, rows, pix_seg, cost, masks=None, n_groups=0, sel=None, prefill=0xEE):
    """The perm table (n_tiles x 64 bytes, prefilled) after rtk_launch_pixel_sort; arguments as sched_ref.pixel_perm."""
    rt, p = libs()
    cost = np.ascontiguousarray(cost, np.uint32).reshape(rows, W)
    import sched_ref
    TW, TH = sched_ref.SHAPES[P]
    n_tiles = -(-W // (2 * TW)) * -(-rows // (2 * TH))
    d_cost, d_perm = Buf(cost), Buf(np.full((n_tiles, 64), prefill, np.uint8))
    d_masks = d_sel = None
    if masks is not None:
        masks = np.ascontiguousarray(masks, np.uint64)
        assert masks.shape == (n_tiles, 4, sched_ref.mask_words(n_groups))
        d_masks = Buf(masks)
    if sel is not None:
        sel = np.ascontiguousarray(sel, np.uint32)
        d_sel = Buf(sel)
    stream, sync = _stream_and_sync()
    _ok(p.sched_probe_pixel_sort(W, rows, P, n_groups, d_masks.ptr if d_masks else None, d_sel.ptr if d_sel else None,
                                 -(-W // sched_ref.REF_TILE), d_cost.ptr, pix_seg, d_perm.ptr, stream),
        "rtk_launch_pixel_sort")
    sync()
    assert np.array_equal(d_cost.read(), cost)
    if d_masks:
        assert np.array_equal(d_masks.read(), masks)
    if d_sel:
        assert np.array_equal(d_sel.read(), sel)
    return d_perm.read()
