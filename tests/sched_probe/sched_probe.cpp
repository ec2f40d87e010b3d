// TEST-ONLY: the one scheduling launcher of librt_trace.so that takes a TraceArgs, reached from Python.
// rtk_launch_pixel_sort reads nine fields of the struct; this file fills those from plain arguments and
// calls it.  It holds no kernel and no copy of one: it is linked against the built librt_trace.so
// (simd-ray-tracer_amd/Makefile, target sched_probe), so the kernel that runs is the library's own.
// tests/sched_probe.py loads it; tests/test_gpu_sched_layer.py holds the references.  The launchers
// that take only pointers and integers (tile sort, XCD grouping, u64 sum) need no probe: the tests
// call them in the library itself.
#include <stdint.h>

#include "rt_kernel.h"

// Every pointer is a device pointer.  masks and sel may be NULL (no cull masks / every tile selected).
// Returns rtk_launch_pixel_sort's code.
extern "C" int sched_probe_pixel_sort(uint32_t width, uint32_t local_rows, int lanes_per_pixel, uint32_t n_groups,
                                      const uint64_t *masks, const uint32_t *sel, uint32_t sel_tiles_x,
                                      uint32_t *pix_cost, uint32_t pix_seg, uint8_t *perm, void *stream) {
    TraceArgs a = {};
    a.width = width;
    a.local_rows = local_rows;
    a.tiles_x = rtk_tiles_x(width, lanes_per_pixel);
    a.n_groups = n_groups;
    a.masks = masks;
    a.sel = sel;
    a.sel_tiles_x = sel_tiles_x;
    a.pix_cost = pix_cost;
    a.pix_seg = pix_seg;
    return rtk_launch_pixel_sort(&a, lanes_per_pixel, perm, (hipStream_t)stream);
}
