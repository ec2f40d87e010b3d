// rt_sched.hip — the kernels around the trace launch: the primary-ray cull
// pass, dead-tile fold, primary group rows, pixel sort, heaviest-first tile
// sort, XCD grouping, RGBA8 encode, per-tile RGBA8 change statistics, the per-tile counts' table pass and stopping
// rule, ray-counter sum and band assembly, with their launchers and the tile geometry queries.  A launch over a list of
// reference tiles (rt_trace_tiles, TraceArgs.sel) is decided here alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_kernel.h"
#include "rtk_cull.h"
#include "rtk_math.h"
#include "rtk_shape.h"

namespace rtk {

// (the cone test and the tile selection: rtk_cull.h, shared with rt_first_hit.hip)

// Striped launch counters of the cull pass (one atomic per block tile, spread
// over kCullStripes addresses so they do not serialise on one): [0, 64) live
// block tiles, [64, 128) image pixels of dead block tiles.
constexpr uint32_t kCullStripes = 64;

// The cull pass: one block per block tile, one wave per wave tile (the trace
// kernel's geometry).  Runs once per camera / scene / launch geometry; the
// trace launches reuse its masks and live-tile list.
template <int P>
__global__ __launch_bounds__(256) void cull_kernel(TraceArgs a, uint32_t *live, uint32_t *cost,
                                                   unsigned long long *counters, uint32_t empty_capable) {
    constexpr uint32_t TW = Shape<P>::TW, TH = Shape<P>::TH;
    __shared__ uint32_t s_any;
    const uint32_t tile = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t tile_x = tile % a.tiles_x, tile_y = tile / a.tiles_x;
    // A block tile outside the launch's selection is neither live nor dead: not traced, not
    // folded, not counted, its mask words not written (block-uniform, before the barrier).
    // This holds for launches that fold nothing too (!empty_capable), where every other tile is live.
    if (!tile_selected<P>(a, tile_x, tile_y)) {
        if (threadIdx.x == 0) {
            live[tile] = kTileSkipped;
            if (a.unit_waves) {
                for (uint32_t w = 0; w < 4u; ++w) cost[4u * tile + w] = 0u;
            } else {
                cost[tile] = 0u;
            }
        }
        return;
    }
    // the wave tile's pixel extent [x0, x1] x [ly0, ly1] (see trace_kernel)
    const uint32_t x0 = tile_x * (2u * TW) + (a.interleave ? (wave & 1u) : (wave & 1u) * TW);
    const uint32_t ly0 = tile_y * (2u * TH) + (a.interleave ? (wave >> 1) : (wave >> 1) * TH);
    const uint32_t x1 = x0 + (a.interleave ? 2u : 1u) * (TW - 1u), ly1 = ly0 + (a.interleave ? 2u : 1u) * (TH - 1u);
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    // the image rows of the wave tile's first and last band-local rows: the band
    // map is increasing, so every row of the tile lies between them (a tile of
    // 16 rows may span two 8-row bands, whose rows between are other devices':
    // the cone then covers them too, which only makes it wider)
    const uint32_t y0 = ((ly0 / a.band_rows) * a.band_count + a.band_index) * a.band_rows + ly0 % a.band_rows;
    const uint32_t y1 = ((ly1 / a.band_rows) * a.band_count + a.band_index) * a.band_rows + ly1 % a.band_rows;
    const Cone c = tile_cone(a, (double)x0 - 0.501, (double)x1 + 0.501, (double)y0 - 0.501, (double)y1 + 0.501);
    const uint32_t n_words = rtk_mask_words(a.n_groups);
    bool any = false;
    for (uint32_t w = 0; w < n_words; ++w) {
        const uint64_t gm = wave_tile_mask<P>(a, c, w, lane);
        if (lane == 0) const_cast<uint64_t *>(a.masks)[((size_t)tile * 4u + wave) * n_words + w] = gm;
        any = any || gm != 0;
    }
    // a wave tile entirely outside the image does no work
    if (lane == 0 && any && x0 < a.width && ly0 < a.local_rows) atomicOr(&s_any, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool l = s_any != 0 || !empty_capable;
        live[tile] = l ? 1u : 0u;
        if (a.unit_waves) {  // the one-wave kernels' order ranks waves (4 * tile + quadrant)
            for (uint32_t w = 0; w < 4u; ++w) cost[4u * tile + w] = l ? 2u : 0u;
        } else {
            cost[tile] = l ? 2u : 0u;
        }
        const uint32_t stripe = tile % kCullStripes;
        if (l) {
            atomicAdd(counters + stripe, 1ull);
        } else {
            const uint32_t bx = tile_x * 2u * TW, by = tile_y * 2u * TH;
            const uint32_t w = min(2u * TW, a.width - bx), h = min(2u * TH, a.local_rows - by);
            atomicAdd(counters + kCullStripes + stripe, (unsigned long long)w * h);
        }
    }
}

// The cull pass's striped counters summed on the device (one wave), so no
// launch needs the host to read them: counters[kCullTotals] = live block
// tiles, counters[kCullTotals + 1] = image pixels of dead block tiles.
__global__ __launch_bounds__(64) void cull_total_kernel(unsigned long long *counters) {
    const uint32_t lane = threadIdx.x;
    unsigned long long live = counters[lane], dead = counters[kCullStripes + lane];
    for (int off = 32; off > 0; off >>= 1) {
        live += __shfl_xor(live, off);
        dead += __shfl_xor(dead, off);
    }
    if (lane == 0) {
        counters[kCullTotals] = live;
        counters[kCullTotals + 1] = dead;
    }
}

// The selection on a device without a cull pass (rt_device_options Cull off): one thread per
// block tile writes what cull_kernel would for a scene it cannot cull -- selected tiles live
// with cost 2, the others skipped with cost 0 -- so the tile sort that follows puts the
// selected tiles first and the trace grid is their count.
template <int P>
__global__ __launch_bounds__(256) void select_kernel(TraceArgs a, uint32_t n_tiles, uint32_t *live, uint32_t *cost) {
    const uint32_t tile = blockIdx.x * 256u + threadIdx.x;
    if (tile >= n_tiles) return;
    const bool l = tile_selected<P>(a, tile % a.tiles_x, tile / a.tiles_x);
    live[tile] = l ? kTileLive : kTileSkipped;
    if (a.unit_waves) {
        for (uint32_t w = 0; w < 4u; ++w) cost[4u * tile + w] = l ? 2u : 0u;
    } else {
        cost[tile] = l ? 2u : 0u;
    }
}

// Pixels of dead block tiles: no sphere group passes any of the tile's
// (conservative) cone tests, so every primary ray of every sample misses;
// without a sky term each sample's Out is exactly 0 (main.cpp:433-440), its
// one segment still counts (main.cpp:390; dead pixels x frames, the pixels
// from the cull pass's device total, added once), and its blend is
// Final = 0*(1/n) + Prev*((n-1)/n) = RN(Prev*((n-1)/n)) -- folded here without
// generating the rays (an all-zero running mean stays exactly zero).  The
// ratios are the trace kernel's fold-table values.
template <int P>
__global__ __launch_bounds__(256) void empty_kernel(TraceArgs a, const uint32_t *live,
                                                    const unsigned long long *dead_pixels) {
    constexpr uint32_t BW = 2u * Shape<P>::TW, BH = 2u * Shape<P>::TH;
    __shared__ float ratio[kFoldTable];
    const bool fold = a.prev_count > 0 && !(a.flags & kFlagAccumZero);
    if (fold)
        for (uint32_t i = threadIdx.x; i < kFoldTable; i += blockDim.x) {
            const uint32_t pc = a.prev_count + i;
            ratio[i] = (float)pc / (float)(pc + 1u);
        }
    __syncthreads();
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        const unsigned long long dead_rays = *dead_pixels * a.frames;
        if (dead_rays) atomicAdd(a.rays, dead_rays);
    }
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, ly = blockIdx.y;
    // (dead tiles only: a tile outside the launch's selection is kTileSkipped and keeps every byte)
    if (!(x < a.width && live[(ly / BH) * a.tiles_x + x / BW] == kTileDead)) return;
    const size_t pix = (size_t)ly * a.width + x;
    float accx = 0.0f, accy = 0.0f, accz = 0.0f;
    if (fold) {
        const float4 pv = a.prev[pix];
        accx = pv.x;
        accy = pv.y;
        accz = pv.z;
    }
    if (accx != 0.0f || accy != 0.0f || accz != 0.0f) {
        for (uint32_t q = 0; q < a.frames; ++q) {
            float r;
            if (q < kFoldTable) {
                r = ratio[q];
            } else {
                const uint32_t pc = a.prev_count + q;
                r = (float)pc / (float)(pc + 1u);
            }
            accx = 0.0f + accx * r;
            accy = 0.0f + accy * r;
            accz = 0.0f + accz * r;
        }
    }
    a.prev[pix] = make_float4(accx, accy, accz, 1.0f);
    if (!a.skip_cur) a.cur[pix] = rgba8(accx, accy, accz, (a.flags & kFlagSrgbPow) != 0u);
}

// empty_kernel for a launch with per-tile counts (TraceArgs.tile_counts_at): a dead block tile's pixels
// fold by the {PreviousRayCount, Frames} pair of the reference tile around them, the ratios being
// the same IEEE f32 quotients (a 256-pixel row segment spans up to eight reference tiles, so there
// is no one table to stage).  The segments can no longer be one product: the thread on a dead block
// tile's first pixel contributes in-image pixels x the tile's frames, a wave sums its lanes, and one
// lane adds the sum to the ray counter and to *folded (rt_trace_info.SegmentsFolded).
template <int P>
__global__ __launch_bounds__(256) void empty_counts_kernel(TraceArgs a, const uint32_t *live,
                                                           unsigned long long *folded) {
    constexpr uint32_t BW = 2u * Shape<P>::TW, BH = 2u * Shape<P>::TH;
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, ly = blockIdx.y;
    // (dead tiles only: a tile outside the launch's selection is kTileSkipped and keeps every byte)
    bool dead = x < a.width && live[(ly / BH) * a.tiles_x + x / BW] == kTileDead;
    uint32_t prev_count = 0, frames = 0;
    if (dead) {  // (a dead tile is a selected one: its reference tile has a pair)
        const uint32_t rt = (ly / kRefTile) * a.sel_tiles_x + x / kRefTile;
        const uint32_t *pair = rtk_tile_counts(a) + 2u * rt;
        prev_count = pair[0];
        frames = pair[1];
        // a resting tile (rt_trace_tile_counts: a listed tile folding no frame) keeps every byte and
        // counts no segment, like a tile outside the selection: with prev_count 0 the store below
        // would otherwise write a zero mean
        dead = frames != 0u;
    }
    unsigned long long seg = 0;
    if (dead && x % BW == 0u && ly % BH == 0u)
        seg = (unsigned long long)min(BW, a.width - x) * min(BH, a.local_rows - ly) * frames;
    for (int off = 32; off > 0; off >>= 1) seg += __shfl_xor(seg, off);  // (every lane active)
    if ((threadIdx.x & 63u) == 0u && seg) {
        atomicAdd(a.rays, seg);
        atomicAdd(folded, seg);
    }
    if (!dead) return;
    const size_t pix = (size_t)ly * a.width + x;
    float accx = 0.0f, accy = 0.0f, accz = 0.0f;
    if (prev_count > 0 && !(a.flags & kFlagAccumZero)) {
        const float4 pv = a.prev[pix];
        accx = pv.x;
        accy = pv.y;
        accz = pv.z;
    }
    if (accx != 0.0f || accy != 0.0f || accz != 0.0f) {
        for (uint32_t q = 0; q < frames; ++q) {
            const uint32_t pc = prev_count + q;
            const float r = (float)pc / (float)(pc + 1u);
            accx = 0.0f + accx * r;
            accy = 0.0f + accy * r;
            accz = 0.0f + accz * r;
        }
    }
    a.prev[pix] = make_float4(accx, accy, accz, 1.0f);
    if (!a.skip_cur) a.cur[pix] = rgba8(accx, accy, accz, (a.flags & kFlagSrgbPow) != 0u);
}

// One wave per block tile: rank its pixels by the last launch's cost (ties by
// index), so wave w of the next launch gets ranks [NPIX w, NPIX (w + 1)).
// With pix_seg = S > 1 the ranked units are row segments of S pixels (summed
// cost), dealt whole: a wave's pixels then form S-pixel runs of a row.
template <int P>
__global__ __launch_bounds__(64) void pixel_sort_kernel(TraceArgs a, uint8_t *perm) {
    constexpr uint32_t TW = Shape<P>::TW, TH = Shape<P>::TH, BW = 2u * TW, NB = 4u * TW * TH;
    static_assert(NB <= 64, "a block tile's pixels fit one wave");
    const uint32_t tile = blockIdx.x, lane = threadIdx.x;
    const uint32_t tile_x = tile % a.tiles_x, tile_y = tile / a.tiles_x;
    uint8_t *pp = perm + (size_t)tile * 64u;
    // a block tile outside the launch's selection is never traced: its masks and costs were never
    // written, and its entry stays "not permuted" (the key's first launch marked every tile so)
    if (!tile_selected<P>(a, tile_x, tile_y)) return;
    // a quadrant without candidate groups folds without tracing: keep such blocks as they are
    if (a.masks) {
        const uint32_t n_words = rtk_mask_words(a.n_groups);
        bool live = false;
        for (uint32_t w = 0; lane < 4u && w < n_words; ++w) live = live || a.masks[((size_t)tile * 4u + lane) * n_words + w] != 0;
        if (__builtin_popcountll(__ballot(lane < 4u && live)) != 4) {
            if (lane == 0) pp[0] = 0xFFu;
            return;
        }
    }
    uint32_t c = 0;
    if (lane < NB) {
        const uint32_t x = tile_x * BW + lane % BW, ly = tile_y * (2u * TH) + lane / BW;
        c = x < a.width && ly < a.local_rows ? a.pix_cost[(size_t)ly * a.width + x] : 0u;
    }
    // segment size: a power of two dividing the block row (BW) and the wave's pixels
    constexpr uint32_t NPIX = NB / 4u;
    const uint32_t S = a.pix_seg >= 4u && NPIX >= 4u && BW % 4u == 0 ? 4u : a.pix_seg >= 2u && NPIX >= 2u ? 2u : 1u;
    for (uint32_t off = 1; off < S; off <<= 1) c += (uint32_t)__shfl_xor((int)c, (int)off, 64);  // (every lane active)
    const uint32_t seg = lane / S, nseg = NB / S;
    uint32_t rank = 0;
    for (uint32_t i = 0; i < nseg; ++i) {
        const uint32_t ci = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)(i * S));
        rank += ci < c || (ci == c && i < seg) ? 1u : 0u;
    }
    if (lane < NB) pp[rank * S + lane % S] = (uint8_t)lane;
}

// Scatter RCCL-gathered compact band images into the full framebuffer.
__global__ __launch_bounds__(256) void assemble_kernel(const uint8_t *src, uint64_t rank_stride, uint8_t *dst,
                                                       uint32_t width, uint32_t height, uint32_t elem,
                                                       uint32_t band_rows, uint32_t band_count) {
    const uint32_t y = blockIdx.y;
    const uint32_t band = y / band_rows;
    const uint32_t owner = band % band_count;
    const uint32_t ly = (band / band_count) * band_rows + y % band_rows;
    const uint8_t *s = src + owner * rank_stride + (uint64_t)ly * width * elem;
    uint8_t *d = dst + (uint64_t)y * width * elem;
    const uint32_t row_bytes = width * elem;
    if ((row_bytes & 15u) == 0 && (((uintptr_t)s | (uintptr_t)d) & 15u) == 0) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(s);
        uint4 *d4 = reinterpret_cast<uint4 *>(d);
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < row_bytes / 16u; i += gridDim.x * blockDim.x)
            d4[i] = s4[i];
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < row_bytes; i += gridDim.x * blockDim.x)
            d[i] = s[i];
    }
}

// ---- heaviest-first tile order for the next launch (counting sort of the
// per-tile costs this launch measured into 32 log2 buckets, descending)
// Counting sort of the tiles by log2(cost), heaviest bucket first, stable,
// without atomics, over the whole grid (a single-block version was latency
// bound at ~60 us; grid-wide device atomics on the few busy buckets ~300 us).
// A wave walks its 64 tiles visiting only the distinct buckets present
// (readlane of the first pending lane + ballot) and keeps per-bucket counters
// in lane k of one VGPR.  Blocks cover 1024 tiles:
//   tile_count_kernel: block j's kSortBuckets bucket counts -> bcount[kSortBuckets*j + k]
//   tile_scan_kernel:  exclusive scan in (bucket descending, block ascending)
//                      order, staged through LDS
//   tile_rank_kernel:  per-wave bases inside the block, the walk again ->
//                      order[rank] = tile
// Consecutive ranks keep similar cost: blocks are dealt round-robin to the 8
// XCDs, so alternating heavy and light tiles would put all heavy work on half
// of them (measured 2x slower).
constexpr uint32_t kSortBlock = 1024, kSortWaves = kSortBlock / 64, kScanLds = 16384;
constexpr uint32_t kSortBuckets = 64;  // one counter per lane

// Quarter-octave buckets of the cost (cycles): 4 log2(c) + the two bits after
// the leading one, offset so octaves 10..25 (1k..64M cycles) are resolved;
// bucket 0 is cost 0 only (dead tiles), so the live-first prefix survives.
// (Measured against whole octaves: 8-rank C2 share 1.035 -> 0.957 ms, C2
// +1.3 %; eighth-octave buckets measured the same as quarter-octave ones.)
__device__ __forceinline__ uint32_t tile_bucket(const uint32_t *cost, uint32_t i, uint32_t n) {
    if (i >= n) return kSortBuckets;  // past the end
    const uint32_t c = cost[i];
    if (c == 0u) return 0u;
    const int l = 31 - __builtin_clz(c);
    const int q = 4 * l + (l >= 2 ? (int)((c >> (l - 2)) & 3u) : 0) - 40;
    return (uint32_t)(q < 1 ? 1 : q > (int)kSortBuckets - 1 ? (int)kSortBuckets - 1 : q);
}

// lane k < kSortBuckets of the result: run[k] + (this wave's count of bucket k);
// *rank: run[b] + this lane's position among the wave's lanes with bucket b
__device__ __forceinline__ uint32_t wave_walk(uint32_t b, uint32_t run, uint32_t lane, uint32_t *rank) {
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t pend = b;
    for (uint64_t live = __ballot(pend < kSortBuckets); live; live = __ballot(pend < kSortBuckets)) {
        const uint32_t b0 = __builtin_amdgcn_readlane(pend, (int)__builtin_ctzll(live));
        const uint64_t m = __ballot(pend == b0);
        if (pend == b0) {
            *rank = __builtin_amdgcn_readlane(run, (int)b0) + (uint32_t)__popcll(m & lt);
            pend = kSortBuckets;
        }
        if (lane == b0) run += (uint32_t)__popcll(m);
    }
    return run;
}

__global__ __launch_bounds__(kSortBlock) void tile_count_kernel(const uint32_t *cost, uint32_t n, uint32_t *bcount) {
    __shared__ uint32_t wc[kSortWaves][kSortBuckets];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t rank;
    const uint32_t c = wave_walk(tile_bucket(cost, blockIdx.x * kSortBlock + threadIdx.x, n), 0u, lane, &rank);
    if (lane < kSortBuckets) wc[wave][lane] = c;
    __syncthreads();
    if (threadIdx.x < kSortBuckets) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kSortWaves; ++w) t += wc[w][threadIdx.x];
        bcount[kSortBuckets * blockIdx.x + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void tile_scan_kernel(uint32_t *bcount, uint32_t n_blk) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t stage[kScanLds];
    const uint32_t len = kSortBuckets * n_blk, t = threadIdx.x, per = (len + 1023u) / 1024u;
    const bool in_lds = len <= kScanLds;
    if (in_lds)
        for (uint32_t j = t; j < len; j += 1024u) stage[j] = bcount[j];
    __syncthreads();
    uint32_t *const src = in_lds ? stage : bcount;
    // scan position p -> (bucket kSortBuckets-1 - p / n_blk, block p % n_blk)
    auto at = [&](uint32_t p) -> uint32_t & { return src[kSortBuckets * (p % n_blk) + (kSortBuckets - 1u - p / n_blk)]; };
    const uint32_t p0 = min(len, t * per), p1 = min(len, p0 + per);
    uint32_t sum = 0;
    for (uint32_t p = p0; p < p1; ++p) sum += at(p);
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {  // inclusive Hillis-Steele scan of the partials
        const uint32_t x = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint32_t off = part[t] - sum;
    for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t c = at(p);
        at(p) = off;
        off += c;
    }
    __syncthreads();
    if (in_lds)
        for (uint32_t j = t; j < len; j += 1024u) bcount[j] = stage[j];
}

__global__ __launch_bounds__(kSortBlock) void tile_rank_kernel(uint32_t *cost, uint32_t n, const uint32_t *bbase,
                                                               uint32_t *order) {
    __shared__ uint32_t wc[kSortWaves][kSortBuckets];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kSortBlock + threadIdx.x, b = tile_bucket(cost, i, n);
    uint32_t rank = 0;
    const uint32_t c = wave_walk(b, 0u, lane, &rank);
    if (lane < kSortBuckets) wc[wave][lane] = c;
    __syncthreads();
    if (threadIdx.x < kSortBuckets) {  // the block's base -> each wave's base, in wave order
        uint32_t off = bbase[kSortBuckets * blockIdx.x + threadIdx.x];
        for (uint32_t w = 0; w < kSortWaves; ++w) {
            const uint32_t x = wc[w][threadIdx.x];
            wc[w][threadIdx.x] = off;
            off += x;
        }
    }
    __syncthreads();
    (void)wave_walk(b, lane < kSortBuckets ? wc[wave][lane] : 0u, lane, &rank);
    if (b < kSortBuckets) {
        order[rank] = i;
        cost[i] = 0;  // measured afresh by the next launch
    }
}

// ---- XCD grouping of the wave order (one-wave kernels).  Workgroups are dealt
// round-robin to the 8 XCDs (block b and b + 8 share one; MI355X_MICROARCH.md,
// "Workgroup dispatch"), so the four waves of a block tile, which store
// neighbouring pixels of the same 128-B lines, land on up to four XCDs whose
// L2s each write their part of every line back (the excess HBM writes of §4).
// Grouping keeps the per-wave heaviest-first order but moves every unit of block
// tile t into one XCD group x = grp[t] (below): the live prefix [0, L) of the sorted order is
// partitioned stably by x (each group stays heaviest first), and group x's r-th
// unit goes to position 8r + x while r < m (the smallest group's size), so block
// 8r + x runs on the group's XCD; the r >= m leftovers (the lightest units of the
// larger groups) follow at 8m + ..., group by group.  A permutation of [0, L):
// no unit is lost or repeated; [L, n) (dead tiles' units) is copied as is.
constexpr uint32_t kXgBlock = 1024, kXgWaves = kXgBlock / 64;

// The group of a block tile is its rank, among the live tiles, in the order of
// their heaviest wave (the tile's first unit in the sorted order), modulo 8: the
// groups then take every eighth tile of a cost-sorted list, so the eight XCDs get
// equal work (a group by tile & 7 measured C2 -1.2 %: its columns' costs differ).
// xg_first_kernel: first[t] = the smallest sorted position of tile t's units;
// xg_flag_count / xg_scan / xg_tile_rank: grp[t] = (rank of tile t among the live
// tiles, by first[t]) & 7 (first and grp: two n_tiles-word arrays in aux).
__device__ __forceinline__ uint32_t xg_group(const uint32_t *in, uint32_t i, uint32_t live_units,
                                             const uint32_t *grp) {
    return i < live_units ? grp[in[i] >> 2] : 8u;
}

__global__ __launch_bounds__(kXgBlock) void xg_first_kernel(const uint32_t *in, uint32_t n,
                                                            const unsigned long long *live_tiles, uint32_t *first) {
    const uint32_t i = blockIdx.x * kXgBlock + threadIdx.x;
    const uint32_t L = (uint32_t)min((unsigned long long)n, 4ull * *live_tiles);
    if (i < L) atomicMin(first + (in[i] >> 2), i);
}

// per block: the number of positions that are their tile's first (bc[blk])
__global__ __launch_bounds__(kXgBlock) void xg_flag_count_kernel(const uint32_t *in, uint32_t n,
                                                                 const unsigned long long *live_tiles,
                                                                 const uint32_t *first, uint32_t *bc) {
    __shared__ uint32_t wc[kXgWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, i = blockIdx.x * kXgBlock + threadIdx.x;
    const uint32_t L = (uint32_t)min((unsigned long long)n, 4ull * *live_tiles);
    const bool f = i < L && first[in[i] >> 2] == i;
    const uint64_t m = __ballot(f);
    if (lane == 0) wc[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kXgWaves; ++w) t += wc[w];
        bc[blockIdx.x] = t;
    }
}

// one wave: exclusive scan of bc[0, n_blk) in place
__global__ __launch_bounds__(64) void xg_scan1_kernel(uint32_t *bc, uint32_t n_blk) {
    if (threadIdx.x != 0) return;
    uint32_t run = 0;
    for (uint32_t b = 0; b < n_blk; ++b) {
        const uint32_t c = bc[b];
        bc[b] = run;
        run += c;
    }
}

__global__ __launch_bounds__(kXgBlock) void xg_tile_rank_kernel(const uint32_t *in, uint32_t n,
                                                                const unsigned long long *live_tiles,
                                                                const uint32_t *first, const uint32_t *bc,
                                                                uint32_t *grp) {
    __shared__ uint32_t wc[kXgWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, i = blockIdx.x * kXgBlock + threadIdx.x;
    const uint32_t L = (uint32_t)min((unsigned long long)n, 4ull * *live_tiles);
    const bool f = i < L && first[in[i] >> 2] == i;
    const uint64_t m = __ballot(f);
    if (lane == 0) wc[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!f) return;
    uint32_t rank = bc[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) rank += wc[w];
    grp[in[i] >> 2] = rank & 7u;
}

__global__ __launch_bounds__(kXgBlock) void xg_count_kernel(const uint32_t *in, uint32_t n,
                                                            const unsigned long long *live_tiles, const uint32_t *grp,
                                                            uint32_t *bc) {
    __shared__ uint32_t wc[kXgWaves][8];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, i = blockIdx.x * kXgBlock + threadIdx.x;
    const uint32_t L = (uint32_t)min((unsigned long long)n, 4ull * *live_tiles);
    const uint32_t x = xg_group(in, i, L, grp);
    for (uint32_t v = 0; v < 8u; ++v) {
        const uint64_t m = __ballot(x == v);
        if (lane == v) wc[wave][v] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < 8u) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kXgWaves; ++w) t += wc[w][threadIdx.x];
        bc[8u * blockIdx.x + threadIdx.x] = t;
    }
}

// one wave: per-group exclusive scan over the blocks (in place), then the group
// sizes c_x, m = min c_x and the leftover bases at bc[8 n_blk ..]
__global__ __launch_bounds__(64) void xg_scan_kernel(uint32_t *bc, uint32_t n_blk) {
    const uint32_t lane = threadIdx.x;
    uint32_t run = 0;
    if (lane < 8u)
        for (uint32_t b = 0; b < n_blk; ++b) {
            const uint32_t c = bc[8u * b + lane];
            bc[8u * b + lane] = run;
            run += c;
        }
    uint32_t m = lane < 8u ? run : 0xFFFFFFFFu;
    for (int off = 1; off < 8; off <<= 1) m = min(m, (uint32_t)__shfl_xor((int)m, off, 64));
    m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
    // base_x = sum over y < x of (c_y - m)
    uint32_t extra = lane < 8u ? run - m : 0u, base = 0;
    for (uint32_t y = 0; y < 8u; ++y) {
        const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)extra, (int)y);
        if (y < lane) base += e;
    }
    if (lane == 0) bc[8u * n_blk] = m;
    if (lane < 8u) bc[8u * n_blk + 1u + lane] = base;
}

__global__ __launch_bounds__(kXgBlock) void xg_place_kernel(const uint32_t *in, uint32_t *out, uint32_t n,
                                                            const unsigned long long *live_tiles, const uint32_t *grp,
                                                            const uint32_t *bc, uint32_t n_blk) {
    __shared__ uint32_t wc[kXgWaves][8];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, i = blockIdx.x * kXgBlock + threadIdx.x;
    const uint32_t L = (uint32_t)min((unsigned long long)n, 4ull * *live_tiles);
    const uint32_t x = xg_group(in, i, L, grp);
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t rank = 0;
    for (uint32_t v = 0; v < 8u; ++v) {
        const uint64_t m = __ballot(x == v);
        if (x == v) rank = (uint32_t)__popcll(m & lt);
        if (lane == v) wc[wave][v] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (i >= n) return;
    if (x >= 8u) {  // a dead tile's unit (or past the live prefix): unchanged
        out[i] = in[i];
        return;
    }
    for (uint32_t w = 0; w < wave; ++w) rank += wc[w][x];
    const uint32_t r = bc[8u * blockIdx.x + x] + rank;
    const uint32_t m = bc[8u * n_blk];
    const uint32_t pos = r < m ? 8u * r + x : 8u * m + bc[8u * n_blk + 1u + x] + (r - m);
    out[pos] = in[i];
}
}  // namespace rtk

extern "C" size_t rtk_tile_sort_scratch(uint32_t n) {
    return rtk::kSortBuckets * 4u * (size_t)((n + rtk::kSortBlock - 1u) / rtk::kSortBlock);
}

extern "C" int rtk_launch_tile_sort(uint32_t *cost, uint32_t *order, uint32_t *scratch, uint32_t n, hipStream_t stream) {
    const uint32_t n_blk = (n + rtk::kSortBlock - 1u) / rtk::kSortBlock;
    if (n_blk == 0) return 0;
    const dim3 grid(n_blk), block(rtk::kSortBlock);
    hipLaunchKernelGGL(rtk::tile_count_kernel, grid, block, 0, stream, (const uint32_t *)cost, n, scratch);
    hipLaunchKernelGGL(rtk::tile_scan_kernel, dim3(1), dim3(1024), 0, stream, scratch, n_blk);
    hipLaunchKernelGGL(rtk::tile_rank_kernel, grid, block, 0, stream, cost, n, (const uint32_t *)scratch, order);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int rtk_launch_xcd_group(const uint32_t *order_in, uint32_t *order_out, uint32_t n_units,
                                    const unsigned long long *live_tiles, uint32_t *scratch, uint32_t *aux,
                                    hipStream_t stream) {
    const uint32_t n_blk = (n_units + rtk::kXgBlock - 1u) / rtk::kXgBlock;
    if (n_blk == 0) return 0;
    const uint32_t n_tiles = (n_units + 3u) / 4u;
    uint32_t *first = aux, *grp = aux + n_tiles;
    const dim3 grid(n_blk), block(rtk::kXgBlock);
    if (hipMemsetAsync(first, 0xFF, (size_t)n_tiles * 4u, stream) != hipSuccess) return -5;
    hipLaunchKernelGGL(rtk::xg_first_kernel, grid, block, 0, stream, order_in, n_units, live_tiles, first);
    hipLaunchKernelGGL(rtk::xg_flag_count_kernel, grid, block, 0, stream, order_in, n_units, live_tiles,
                       (const uint32_t *)first, scratch);
    hipLaunchKernelGGL(rtk::xg_scan1_kernel, dim3(1), dim3(64), 0, stream, scratch, n_blk);
    hipLaunchKernelGGL(rtk::xg_tile_rank_kernel, grid, block, 0, stream, order_in, n_units, live_tiles,
                       (const uint32_t *)first, (const uint32_t *)scratch, grp);
    hipLaunchKernelGGL(rtk::xg_count_kernel, grid, block, 0, stream, order_in, n_units, live_tiles,
                       (const uint32_t *)grp, scratch);
    hipLaunchKernelGGL(rtk::xg_scan_kernel, dim3(1), dim3(64), 0, stream, scratch, n_blk);
    hipLaunchKernelGGL(rtk::xg_place_kernel, grid, block, 0, stream, order_in, order_out, n_units, live_tiles,
                       (const uint32_t *)grp, (const uint32_t *)scratch, n_blk);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

// (rtk_tile_count and rtk_tiles_x, host arithmetic on the launch shapes: rt_plan.cpp)

namespace rtk {
// The primary rounds' group rows for this camera (TraceArgs.prim): one sphere
// slot per thread, c = RN(centre - CameraPosition) as main.cpp:401 rounds it
// (one f32 subtraction: no contraction, IEEE denormals), and r*r copied.
__global__ __launch_bounds__(256) void prim_kernel(TraceArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // sphere slot 4 g + l
    if (i >= 4u * a.n_groups) return;
    const uint32_t g = i >> 2, l = i & 3u;
    const float *src = reinterpret_cast<const float *>(a.groups + (size_t)kGroupF4 * g);
    float *dst = reinterpret_cast<float *>(a.prim + (size_t)kPrimF4 * g);
    dst[0u + l] = src[4u * kRowX + l] - a.cam_pos[0];
    dst[4u + l] = src[4u * kRowY + l] - a.cam_pos[1];
    dst[8u + l] = src[4u * kRowZ + l] - a.cam_pos[2];
    dst[12u + l] = src[4u * kRowR2 + l];
}
}  // namespace rtk

template <int P>
static void launch_cull_p(const TraceArgs *a, uint32_t *live, uint32_t *cost, unsigned long long *counters,
                          int empty_capable, hipStream_t stream) {
    const uint32_t n = rtk_tile_count(a->width, a->local_rows, P);
    if (a->n_groups)
        hipLaunchKernelGGL(rtk::prim_kernel, dim3((4u * a->n_groups + 255u) / 256u), dim3(256), 0, stream, *a);
    (void)hipMemsetAsync(counters, 0, 2u * rtk::kCullStripes * sizeof(unsigned long long), stream);
    hipLaunchKernelGGL(rtk::cull_kernel<P>, dim3(n), dim3(256), 0, stream, *a, live, cost, counters,
                       (uint32_t)(empty_capable != 0));
    hipLaunchKernelGGL(rtk::cull_total_kernel, dim3(1), dim3(64), 0, stream, counters);
}

extern "C" int rtk_launch_cull(const TraceArgs *a, int lanes_per_pixel, uint32_t *live, uint32_t *cost,
                               unsigned long long *counters, int empty_capable, hipStream_t stream) {
    if (!a->masks || !a->prim) return -1;
    RTK_BY_P(launch_cull_p, a, live, cost, counters, empty_capable, stream)
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <int P>
static void launch_select_p(const TraceArgs *a, uint32_t *live, uint32_t *cost, hipStream_t stream) {
    const uint32_t n = rtk_tile_count(a->width, a->local_rows, P);
    hipLaunchKernelGGL(rtk::select_kernel<P>, dim3((n + 255u) / 256u), dim3(256), 0, stream, *a, n, live, cost);
}

extern "C" int rtk_launch_select(const TraceArgs *a, int lanes_per_pixel, uint32_t *live, uint32_t *cost,
                                 hipStream_t stream) {
    if (!a->sel) return -1;
    RTK_BY_P(launch_select_p, a, live, cost, stream)
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <int P>
static void launch_empty_p(const TraceArgs *a, const uint32_t *live, const unsigned long long *dead_pixels,
                           hipStream_t stream) {
    hipLaunchKernelGGL(rtk::empty_kernel<P>, dim3((a->width + 255u) / 256u, a->local_rows), dim3(256), 0, stream, *a,
                       live, dead_pixels);
}

extern "C" int rtk_launch_empty(const TraceArgs *a, int lanes_per_pixel, const uint32_t *live,
                                const unsigned long long *dead_pixels, hipStream_t stream) {
    RTK_BY_P(launch_empty_p, a, live, dead_pixels, stream)
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <int P>
static void launch_empty_counts_p(const TraceArgs *a, const uint32_t *live, unsigned long long *folded,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(rtk::empty_counts_kernel<P>, dim3((a->width + 255u) / 256u, a->local_rows), dim3(256), 0,
                       stream, *a, live, folded);
}

extern "C" int rtk_launch_empty_counts(const TraceArgs *a, int lanes_per_pixel, const uint32_t *live,
                                       unsigned long long *folded, hipStream_t stream) {
    if (!a->tile_counts_at || !a->sel || !folded) return -1;
    RTK_BY_P(launch_empty_counts_p, a, live, folded, stream)
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

template <int P>
static void launch_pixel_sort_p(const TraceArgs *a, uint8_t *perm, hipStream_t stream) {
    const uint32_t n = rtk_tile_count(a->width, a->local_rows, P);
    hipLaunchKernelGGL(rtk::pixel_sort_kernel<P>, dim3(n), dim3(64), 0, stream, *a, perm);
}

extern "C" int rtk_launch_pixel_sort(const TraceArgs *a, int lanes_per_pixel, uint8_t *perm, hipStream_t stream) {
    switch (a->pix_cost ? lanes_per_pixel : 0) {  // (a block tile of 64 pixels at most: P >= 4)
        case 32: launch_pixel_sort_p<32>(a, perm, stream); break;
        case 16: launch_pixel_sort_p<16>(a, perm, stream); break;
        case 8: launch_pixel_sort_p<8>(a, perm, stream); break;
        case 4: launch_pixel_sort_p<4>(a, perm, stream); break;
        default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

namespace rtk {
// Re-encode a resident running mean (v4 f32) as RGBA8: the store of
// main.cpp:490 on its own (rt_encode_rgba8).
__global__ __launch_bounds__(256) void encode_kernel(const float4 *accum, uint32_t *out, uint64_t n, uint32_t pw) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const float4 v = accum[i];
        out[i] = rgba8(v.x, v.y, v.z, pw != 0u);
    }
}
}  // namespace rtk

extern "C" int rtk_launch_encode(const void *accum, void *out, uint64_t n, uint32_t pow_mode, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + 255u) / 256u;
    const uint32_t grid = (uint32_t)(blocks < 8192u ? blocks : 8192u);
    hipLaunchKernelGGL(rtk::encode_kernel, dim3(grid), dim3(256), 0, stream, (const float4 *)accum, (uint32_t *)out, n,
                       pow_mode);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

namespace rtk {
// encode_kernel over the listed reference tiles of a full image (rt_trace_tiles with the encode
// pass): one thread per pixel of a row; a pixel of an unlisted tile is neither read nor written.
__global__ __launch_bounds__(256) void encode_selected_kernel(const float4 *accum, uint32_t *out, uint32_t width,
                                                              const uint32_t *sel, uint32_t sel_tiles_x, uint32_t pw) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
    if (x >= width) return;
    const uint32_t t = (y / kRefTile) * sel_tiles_x + x / kRefTile;
    if (!((sel[t >> 5] >> (t & 31u)) & 1u)) return;
    const size_t i = (size_t)y * width + x;
    const float4 v = accum[i];
    out[i] = rgba8(v.x, v.y, v.z, pw != 0u);
}
}  // namespace rtk

extern "C" int rtk_launch_encode_selected(const TraceArgs *a, hipStream_t stream) {
    if (!a->sel || a->width == 0 || a->local_rows == 0) return -1;
    hipLaunchKernelGGL(rtk::encode_selected_kernel, dim3((a->width + 255u) / 256u, a->local_rows), dim3(256), 0, stream,
                       (const float4 *)a->prev, a->cur, a->width, a->sel, a->sel_tiles_x,
                       (a->flags & kFlagSrgbPow) ? 1u : 0u);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

namespace rtk {
// One pixel's share of a tile's rt_tile_delta (rt_trace.h): alpha masked out of both words, then
// v_sad_u8 sums the three byte differences in one op; a byte lane alone under the same op is that
// channel's |new - old| (the other lanes are zero), for the maximum and the squares.
__device__ __forceinline__ void delta_pixel(uint32_t o, uint32_t n, uint32_t &changed, uint32_t &mx, uint32_t &sum,
                                            uint32_t &sq) {
    o &= 0x00FFFFFFu;
    n &= 0x00FFFFFFu;
    changed += o != n ? 1u : 0u;
    sum = __builtin_amdgcn_sad_u8(o, n, sum);
    const uint32_t d0 = __builtin_amdgcn_sad_u8(o & 0xFFu, n & 0xFFu, 0u);
    const uint32_t d1 = __builtin_amdgcn_sad_u8(o & 0xFF00u, n & 0xFF00u, 0u);
    const uint32_t d2 = __builtin_amdgcn_sad_u8(o & 0xFF0000u, n & 0xFF0000u, 0u);
    mx = max(mx, max(d0, max(d1, d2)));
    sq += d0 * d0 + d1 * d1 + d2 * d2;
}

// Per-tile RGBA8 change statistics (rt_tile_delta: {Changed, MaxDelta, SumDelta, SumSquares} over the
// R, G, B bytes), one 256-thread block per reference tile of a width x height image, grid (TilesX,
// TilesY); thread t owns row t >> 3 of the tile and the four pixels at columns 4 (t & 7) ..+3, so a
// wave covers 8 tile rows and a lane 16 contiguous RGBA8 bytes (64 of the running mean).
//   ENCODE: the closing pass of rt_trace_tile_work_delta in place of encode_selected_kernel -- "new"
//           is rgba8() of the running mean (the same function, the same bytes), "old" what old_img
//           (== new_img, CurrentImage) held, read before the new bytes are stored there.
//   else:   old_img against new_img, nothing stored (rt_tile_delta_rgba8).
// A block whose bit of `sel` is clear (sel != NULL) leaves before any vector memory access: a uniform
// branch on a scalar load.  vec (launch-uniform: width % 4 == 0 and 16-byte aligned RGBA8 bases): one
// 16-byte access per lane and image, else four dwords.  Pixels outside the image are neither read nor
// written and add nothing.  Integers only: lanes fold by __shfl_xor, the four waves through 64 B of
// LDS, and one lane stores the tile's entry with one 16-byte store -- no atomics, nothing pre-zeroed,
// no summation order to speak of.
template <bool ENCODE>
__global__ __launch_bounds__(256) void tile_delta_kernel(const float4 *accum, const uint32_t *old_img,
                                                         uint32_t *new_img, uint32_t width, uint32_t height,
                                                         const uint32_t *sel, uint32_t pw, uint32_t vec,
                                                         uint4 *delta) {
    __shared__ uint4 part[4];
    const uint32_t tile = blockIdx.y * gridDim.x + blockIdx.x;
    if (sel && !((sel[tile >> 5] >> (tile & 31u)) & 1u)) return;
    const uint32_t t = threadIdx.x;
    const uint32_t x = blockIdx.x * kRefTile + 4u * (t & 7u), y = blockIdx.y * kRefTile + (t >> 3);
    const uint32_t npix = y < height && x < width ? min(4u, width - x) : 0u;  // (vec: 0 or 4)
    const size_t pix = (size_t)y * width + x;
    // (a pixel outside the image is never seen: it adds nothing)
    uint32_t changed = 0, mx = 0, sum = 0, sq = 0;
    if (npix && vec) {  // (four pixels: every load is issued before the first use)
        const uint4 ov = *reinterpret_cast<const uint4 *>(old_img + pix);
        uint4 nv;
        if (ENCODE) {
            float4 v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) v[k] = accum[pix + k];
            nv.x = rgba8(v[0].x, v[0].y, v[0].z, pw != 0u);
            nv.y = rgba8(v[1].x, v[1].y, v[1].z, pw != 0u);
            nv.z = rgba8(v[2].x, v[2].y, v[2].z, pw != 0u);
            nv.w = rgba8(v[3].x, v[3].y, v[3].z, pw != 0u);
            *reinterpret_cast<uint4 *>(new_img + pix) = nv;
        } else {
            nv = *reinterpret_cast<const uint4 *>(new_img + pix);
        }
        delta_pixel(ov.x, nv.x, changed, mx, sum, sq);
        delta_pixel(ov.y, nv.y, changed, mx, sum, sq);
        delta_pixel(ov.z, nv.z, changed, mx, sum, sq);
        delta_pixel(ov.w, nv.w, changed, mx, sum, sq);
    } else {  // (a width off the 4-pixel grid or an unaligned image: pixel by pixel, dwords)
#pragma nounroll
        for (uint32_t k = 0; k < npix; ++k) {
            const uint32_t o = old_img[pix + k];
            uint32_t n;
            if (ENCODE) {
                const float4 v = accum[pix + k];
                new_img[pix + k] = n = rgba8(v.x, v.y, v.z, pw != 0u);
            } else {
                n = new_img[pix + k];
            }
            delta_pixel(o, n, changed, mx, sum, sq);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {  // (every lane active)
        changed += (uint32_t)__shfl_xor((int)changed, off);
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
        sum += (uint32_t)__shfl_xor((int)sum, off);
        sq += (uint32_t)__shfl_xor((int)sq, off);
    }
    if ((t & 63u) == 0u) part[t >> 6] = make_uint4(changed, mx, sum, sq);
    __syncthreads();
    if (t == 0u) {
        uint4 r = part[0];
        for (uint32_t w = 1; w < 4u; ++w) {
            const uint4 p = part[w];
            r.x += p.x;
            r.y = max(r.y, p.y);
            r.z += p.z;
            r.w += p.w;
        }
        delta[tile] = r;
    }
}
}  // namespace rtk

namespace rtk {
// The table pass of rt_trace_tile_counts: the launch's internal counts table (rtk_sel_table_at) from the
// caller's device table and the key's bitmap, one thread per reference tile of the image.  A listed tile
// gets {prev, effective frames} (rtk_effective_frames), every other tile {0, 0} without its entry being
// read: the trace and empty-tile kernels' pairs hold what the host-built table would (a pair that fits the
// u32 frame count, frames <= the launch's), whatever the caller's memory holds.  `active` receives the
// bitmap of the listed tiles that fold a frame, for the closing pass (a resting tile stores no RGBA8 and
// no statistics): lane 0 of each wave stores its 64 tiles' two words with one 8-byte store (the bitmaps
// are whole 64-tile words, 8-byte aligned: rtk_sel_table_at).
__global__ __launch_bounds__(256) void counts_table_kernel(const uint32_t *counts, const uint32_t *sel, uint32_t n_tiles,
                                                           uint32_t max_frames, uint2 *table, uint2 *active) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint2 pair = make_uint2(0u, 0u);
    if (t < n_tiles) {
        if ((sel[t >> 5] >> (t & 31u)) & 1u) {  // (the caller's struct is 4-byte aligned: two dword loads)
            const uint32_t prev = counts[2u * t], f = rtk_effective_frames(prev, counts[2u * t + 1u], max_frames);
            pair = make_uint2(f ? prev : 0u, f);
        }
        table[t] = pair;
    }
    const uint64_t m = __ballot(pair.y != 0u);
    if ((threadIdx.x & 63u) == 0u && (t & ~63u) < n_tiles) active[t >> 6] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
}

// The library's per-tile stopping rule (rt_tile_counts_step; rt_trace.h states it): every entry of the
// table that folded a frame in the round just traced advances by it and rests, or takes the next round's
// frames by the doubling rule.  Integers only.  One block walks the image's tiles (8160 at 8K: eight per
// thread), so the summary is a plain sum folded through the lanes and 1 KB of LDS -- no atomics, nothing
// pre-zeroed, one value for a given input.
constexpr uint32_t kStepBlock = 1024;
__global__ __launch_bounds__(kStepBlock) void tile_counts_step_kernel(uint32_t *counts, const uint4 *delta, uint32_t n_tiles,
                                                                      uint32_t max_round, uint32_t max_tile,
                                                                      uint32_t rest_max_delta, uint32_t rest_sum_squares,
                                                                      uint32_t *summary) {
    __shared__ unsigned long long s_next[kStepBlock / 64u];
    __shared__ uint32_t s_active[kStepBlock / 64u], s_rested[kStepBlock / 64u];
    unsigned long long next = 0;
    uint32_t active = 0, rested = 0;
    for (uint32_t t = threadIdx.x; t < n_tiles; t += kStepBlock) {
        const uint32_t prev = counts[2u * t];
        const uint32_t f = rtk_effective_frames(prev, counts[2u * t + 1u], max_round);
        if (f == 0u) continue;  // (a resting or impossible entry stays as it is and folds nothing next round either)
        const uint32_t done = prev + f;  // (fits: rtk_effective_frames)
        bool rest = done >= max_tile;
        if (!rest && prev != 0u) {  // (a first round never rests on its statistics: "old" was the caller's)
            const uint4 d = delta[t];
            rest = d.y <= rest_max_delta && d.w <= rest_sum_squares;
        }
        // the doubling rule: as many frames again as the tile has, within the round's and the tile's bounds
        // (done + these <= max_tile, so the new entry's effective frames are its Frames)
        const uint32_t frames = rest ? 0u : min(done, min(max_round, max_tile - done));
        counts[2u * t] = done;
        counts[2u * t + 1u] = frames;
        next += frames;
        active += frames != 0u ? 1u : 0u;
        rested += rest ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) {  // (every lane active)
        next += __shfl_xor(next, off);
        active += (uint32_t)__shfl_xor((int)active, off);
        rested += (uint32_t)__shfl_xor((int)rested, off);
    }
    if (!summary) return;  // (launch-uniform)
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        s_next[w] = next;
        s_active[w] = active;
        s_rested[w] = rested;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t i = 1; i < kStepBlock / 64u; ++i) {
            next += s_next[i];
            active += s_active[i];
            rested += s_rested[i];
        }
        summary[0] = (uint32_t)next;  // (rt_tile_step_summary: u64 NextFrames, little-endian)
        summary[1] = (uint32_t)(next >> 32);
        summary[2] = active;
        summary[3] = rested;
    }
}
}  // namespace rtk

extern "C" int rtk_launch_counts_table(const void *counts, const uint32_t *sel, uint32_t n_ref_tiles, uint32_t max_frames,
                                       uint32_t *table, uint32_t *active, hipStream_t stream) {
    if (!counts || !sel || !table || !active || n_ref_tiles == 0 || max_frames == 0) return -1;
    hipLaunchKernelGGL(rtk::counts_table_kernel, dim3((n_ref_tiles + 255u) / 256u), dim3(256), 0, stream,
                       (const uint32_t *)counts, sel, n_ref_tiles, max_frames, (uint2 *)table, (uint2 *)active);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int rtk_launch_tile_counts_step(void *counts, const void *delta, uint32_t n_ref_tiles, uint32_t max_round,
                                           uint32_t max_tile, uint32_t rest_max_delta, uint32_t rest_sum_squares,
                                           void *summary, hipStream_t stream) {
    if (!counts || !delta || n_ref_tiles == 0 || max_round == 0 || max_tile == 0) return -1;
    hipLaunchKernelGGL(rtk::tile_counts_step_kernel, dim3(1), dim3(rtk::kStepBlock), 0, stream, (uint32_t *)counts,
                       (const uint4 *)delta, n_ref_tiles, max_round, max_tile, rest_max_delta, rest_sum_squares,
                       (uint32_t *)summary);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0u; }

extern "C" int rtk_launch_tile_delta_encode(const TraceArgs *a, void *delta, hipStream_t stream) {
    if (!a->sel || !delta || a->width == 0 || a->local_rows == 0) return -1;
    const dim3 grid(a->sel_tiles_x, (a->local_rows + kRefTile - 1u) / kRefTile);
    hipLaunchKernelGGL(rtk::tile_delta_kernel<true>, grid, dim3(256), 0, stream, (const float4 *)a->prev,
                       (const uint32_t *)a->cur, a->cur, a->width, a->local_rows, a->sel,
                       (a->flags & kFlagSrgbPow) ? 1u : 0u, (a->width & 3u) == 0u && aligned16(a->cur) ? 1u : 0u,
                       (uint4 *)delta);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int rtk_launch_tile_delta(const uint32_t *old_img, const uint32_t *new_img, uint32_t width, uint32_t height,
                                     void *delta, hipStream_t stream) {
    if (!old_img || !new_img || !delta || width == 0 || height == 0) return -1;
    const dim3 grid((width + kRefTile - 1u) / kRefTile, (height + kRefTile - 1u) / kRefTile);
    hipLaunchKernelGGL(rtk::tile_delta_kernel<false>, grid, dim3(256), 0, stream, (const float4 *)nullptr, old_img,
                       const_cast<uint32_t *>(new_img), width, height, (const uint32_t *)nullptr, 0u,
                       (width & 3u) == 0u && aligned16(old_img) && aligned16(new_img) ? 1u : 0u, (uint4 *)delta);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

__global__ void sum_u64_kernel(const uint64_t *slots, uint32_t n, uint64_t *dst) {
    if (threadIdx.x != 0) return;
    uint64_t s = 0;
    for (uint32_t i = 0; i < n; ++i) s += slots[i];
    dst[0] += s;
}

extern "C" int rtk_launch_sum_u64(const uint64_t *slots, uint32_t n, uint64_t *dst, hipStream_t stream) {
    hipLaunchKernelGGL(sum_u64_kernel, dim3(1), dim3(64), 0, stream, slots, n, dst);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int rtk_launch_assemble(const void *src, uint64_t rank_stride, void *dst, uint32_t width, uint32_t height,
                                   uint32_t elem, uint32_t band_rows, uint32_t band_count, hipStream_t stream) {
    const dim3 block(256);
    const dim3 grid(4, height);
    hipLaunchKernelGGL(rtk::assemble_kernel, grid, block, 0, stream, (const uint8_t *)src, rank_stride, (uint8_t *)dst,
                       width, height, elem, band_rows, band_count);
    return hipGetLastError() == hipSuccess ? 0 : -5;
}
