/*
 * rt_trace.h — C-ABI of the MI355X-native brute-force sphere trace path.
 *
 * Drop-in boundary for the per-pixel trace loop of Ne0nWinds/SIMD-Ray-Tracer
 * (reference @ 2025-01-03).  The reference has no FFI; its path boundary is
 *   (a) the tile callback launched by WorkQueueStart(RenderTile | RenderTileScalar,
 *       TilesX*TilesY, ThreadCount)                     main.cpp:851-856, base.h:166-178
 *       reading the globals CameraInfo, Scenes[SceneIndex], PreviousRayCount,
 *       ThreadContexts                                   main.cpp:7, 53-54, 289-290
 *   (b) the app entry points OnInit / OnRender           base.h:163-164, main.cpp:645-859
 * Every entry point below names the reference interface it replaces.
 *
 * Conventions: plain C types, pointers and sizes only.  Functions return 0 on
 * success or a negative errno-style code (RT_E*).  Calls on one rt_device are
 * single-threaded; each device owns one HIP stream unless a stream is passed.
 * Structs marked "byte-compatible" have the reference's exact layout
 * (offsets asserted in simd-ray-tracer_amd/csrc/rt_scene.cpp and tests/).
 */
#ifndef RT_TRACE_H
#define RT_TRACE_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_TRACE_ABI_VERSION 1u
#define RT_ALIGN16 __attribute__((aligned(16)))

/* Error codes (negative errno values). */
#define RT_OK 0
#define RT_EINVAL (-22)  /* bad argument / shape */
#define RT_ENOMEM (-12)  /* allocation failed */
#define RT_ENODEV (-19)  /* no HIP device / HIP runtime error */
#define RT_EBUSY (-16)   /* previous frame still in flight */
#define RT_EIO (-5)      /* HIP/RCCL error while running */

/* ------------------------------------------------ byte-compatible structs */

/* v3: base.h:357-375 (4 floats, 16-byte aligned, _w padding lane). */
typedef struct rt_v3 {
    float x, y, z, _w;
} RT_ALIGN16 rt_v3;

/* material: main.cpp:11-16 — 48 B. */
typedef struct rt_material {
    rt_v3 Color;
    rt_v3 Emissive;
    float Specular;
    float IndexOfRefraction; /* 0 = diffuse/specular, else dielectric */
} rt_material;

/* scalar_sphere: main.cpp:17-21 — 80 B. */
typedef struct rt_scalar_sphere {
    rt_v3 Position;
    float Radius;
    rt_material Material;
} rt_scalar_sphere;

/* sphere_group: main.cpp:23-26 with SIMD_WIDTH = 4 (v3x4 + f32x4) — 64 B. */
typedef struct rt_sphere_group {
    float X[4], Y[4], Z[4], Radii[4];
} RT_ALIGN16 rt_sphere_group;

/* array<T>: main.cpp:28-40 — 16 B. */
typedef struct rt_array {
    void *Data;
    uint32_t Count;
} rt_array;

/* scene: main.cpp:42-51 — 80 B. */
typedef struct rt_scene {
    rt_v3 LookAt;
    bool UseSkyColor;
    float DefaultDistanceFromLookAt;
    float DefaultXAngle;
    float DefaultYHeight;
    rt_array ScalarSpheres; /* rt_scalar_sphere[Count] */
    rt_array SIMDSpheres;   /* rt_sphere_group[Count]  */
    rt_array Materials;     /* rt_material[Count]      */
} rt_scene;

/* format / image: base.h:117-136 — 24 B. */
#define RT_FORMAT_R32B32G32A32_F32 1u
#define RT_FORMAT_R8G8B8A8_U32 2u
typedef struct rt_image {
    void *Data;
    uint32_t Width, Height;
    uint32_t Format;
} rt_image;

/* camera_info: main.cpp:270-282 — 144 B. */
typedef struct rt_camera_info {
    rt_v3 CameraPosition;
    rt_v3 CameraZ;
    rt_v3 CameraX;
    rt_v3 CameraY;
    rt_v3 FilmCenter;
    float FilmW;
    float FilmH;
    uint32_t TilesX;
    rt_image CurrentImage;  /* RGBA8 u32 per pixel   */
    rt_image PreviousImage; /* v4 f32 running mean   */
} rt_camera_info;

/* render_params: base.h:157-161 — 12 B. */
typedef struct rt_render_params {
    uint32_t ThreadCount; /* ignored on the GPU (kept for the signature) */
    bool EnableSIMD;      /* true: RenderTile rules, false: RenderTileScalar rules */
    uint32_t SceneIndex;
} rt_render_params;

/* init_params: base.h:152-155 (string8 = {char*, u32}). */
typedef struct rt_init_params {
    uint32_t WindowWidth, WindowHeight;
    const char *WindowTitle;
    uint32_t WindowTitleSize;
} rt_init_params;

/* ------------------------------------------------------ host-side inputs */

/* Built-in scenes 0 RGB Glass, 1 Floating Spheres, 2 RTWeekend, generated
 * exactly as InitRGBSphereScene / InitRandomizedSphereScene /
 * InitRTWeekendSphereScene (main.cpp:96-268).  The returned scene points at
 * library-owned static storage (like the reference's static arrays). */
int rt_scene_builtin(uint32_t index, rt_scene *out);

/* First `n_spheres` spheres of `in` (the BASELINE "N-sphere" synthetic
 * scenes are prefixes of scene 1): counts become n, ceil(n/4), n+1; the
 * data pointers are shared. */
int rt_scene_prefix(const rt_scene *in, uint32_t n_spheres, rt_scene *out);

/* Camera basis + film for an orbit around scene->LookAt, exactly as
 * OnRender computes it (main.cpp:763-838, x87 fcos/fsin).  Image fields
 * of `out` are zeroed; the caller fills them. */
int rt_camera_setup(const rt_scene *scene, float distance_from_look_at, float x_angle, float y_height,
                    uint32_t width, uint32_t height, rt_camera_info *out);

/* Per-(pixel, frame) seed of the GPU's 'pixel' seed mode: the per-thread
 * mixer of main.cpp:668-675 applied to i = (k*H + y)*W + x. */
uint64_t rt_pixel_seed(uint32_t x, uint32_t y, uint32_t frame, uint32_t width, uint32_t height);

/* -------------------------------------------------------- device context */

typedef struct rt_device rt_device;

/* Replaces OnInit's allocation + WorkQueueCreate (main.cpp:658-665).  The
 * device runs the default kernels (every field of rt_device_options 0); the
 * library reads no environment variable that changes what it computes or
 * how (only the diagnostic RT_STATS / RT_WAVETIMES hooks, below). */
int rt_device_create(int hip_device, rt_device **out);
int rt_device_destroy(rt_device *dev);

/* Kernel and schedule choices of one device, fixed at creation.  Every
 * choice gives the same bits (each is parity-tested against the oracle); they
 * exist for A/B measurements and for the brute-force roofline (Cull and
 * Prefilter RT_OPT_OFF: every counted segment tests every sphere, as
 * main.cpp:399-430 does).  The reference's only run-time knobs are
 * render_params (base.h:157-161: ThreadCount, EnableSIMD, SceneIndex), which
 * rt_trace_desc carries.  Tri-state fields: RT_OPT_DEFAULT (0), RT_OPT_ON (1),
 * RT_OPT_OFF (-1); numeric fields: 0 = the default.  A zero-filled struct is
 * rt_device_create's behaviour. */
#define RT_OPT_DEFAULT 0
#define RT_OPT_ON 1
#define RT_OPT_OFF (-1)
typedef struct rt_device_options {
    uint32_t Size;               /* sizeof(rt_device_options), or 0                                  */
    int32_t Cull;                /* primary-ray cone cull and dead-tile fold (default on)            */
    int32_t Prefilter;           /* secondary-ray prefilter (default: per scene)                     */
    int32_t PrefilterRelative;   /* per-lane prefilter thresholds (default: per scene)               */
    int32_t Clusters;            /* cluster walk (default and ON: scenes of <= 128 groups, the       */
                                 /* largest a table is built for; beyond, ON is ignored)             */
    int32_t ClusterCount;        /* k-means top clusters K >= 2 (0: ~1.25 sqrt(n) or n / 8..17)      */
    int32_t SubClusterSpheres;   /* spheres per sub-cluster of two-level tables (0: 3, per-lane 4)   */
    int32_t SecondaryThreshold;  /* lanes a secondary round waits for (0: 24/40/48 by walk size)     */
    int32_t LanesPerPixel;       /* 1/2/4/8/16/32 sample chains per pixel (0: per launch)            */
    int32_t PixelsPerLane;       /* 1 never, 4 always (0: 4 for one-frame one-lane launches)         */
    int32_t OneWaveGroups;       /* one wave per workgroup, no LDS image (default on)                */
    int32_t SphereSourceLds;     /* four-wave kernels read spheres from LDS, not SMEM (default off)  */
    int32_t SceneInHbm;          /* four-wave kernels keep the scene out of LDS (default off)        */
    int32_t TablesInLds;         /* four-wave kernels' rsqrt / fold tables in LDS at P <= 8 (on)     */
    int32_t WalkAny;             /* the one-wave kernel picks its walk at run time (default off;     */
                                 /* MaxBounce == 0 and r^2 outside the short sqrt's range always do) */
    int32_t Interleave;          /* wave tiles interleaved over the block tile (default off)         */
    int32_t MergeRounds;         /* primary + secondary rays in every round (default: <= 2 groups)   */
    int32_t TileOrder;           /* heaviest-first order learned from earlier launches (default on)  */
    int32_t WaveOrder;           /* one-wave kernels order waves, not block tiles (default on)       */
    int32_t PixelSort;           /* a block tile's pixels dealt to its waves by cost (default on)    */
    int32_t PixelSegment;        /* pixels per dealt unit: 1, 2 or 4 (0: 1)                          */
    int32_t XcdGroup;            /* a block tile's waves on one XCD (default: launches at P <= 4)    */
    int32_t SplitFirstLaunch;    /* a key's first long launch measures costs first (default on)      */
    int32_t HeadSamples;         /* samples per lane of that split's head (0: 8)                     */
    int32_t SplitParts;          /* launches of the split, 1..8 (0: 2)                               */
    int32_t SplitGrowth;         /* each leading part this many times the previous (0: 3)            */
    int32_t OrderLaunches;       /* re-sorts per key before the order is kept (0: 4; -1: none)       */
    int32_t EncodePass;          /* RGBA8 by a coalesced pass after multi-frame launches (default on) */
    int32_t DirectionTable;      /* member entries chosen by the direction table (default: launches  */
                                 /* of at most 8 lanes per pixel; ON: 16 too; OFF: no table built)   */
} rt_device_options;

/* rt_device_create with options (NULL: the defaults).  RT_EINVAL for a value
 * out of range or a Size this library does not know. */
int rt_device_create_ex(int hip_device, const rt_device_options *options, rt_device **out);
/* The options the device was created with (as given, defaults left 0). */
int rt_device_get_options(rt_device *dev, rt_device_options *out);

/* x86 rsqrtss reproduction table (2 x 1024 f32): makes
 * v3::NormalizeFast (x64_math.h:246-257) bit-exact on the GPU. Required. */
int rt_set_rsqrt_table(rt_device *dev, const float table[2048]);

/* The built-in table: rsqrtss as captured on an Intel host (the parity
 * target; tests/golden/rsqrt_lut_intel.bin). */
int rt_rsqrt_table_builtin(float table_out[2048]);

/* Captures this host CPU's own rsqrtss into a table (x86 only).  Returns
 * RT_EINVAL when the host's rsqrtss is not representable by a parity +
 * 10-bit table (checked on a sample of inputs). */
int rt_rsqrt_table_capture_host(float table_out[2048]);

/* Uploads Scenes[SceneIndex] (read by RenderTile at main.cpp:370) into
 * HBM: SIMDSpheres/Materials for the SIMD rules, ScalarSpheres for the
 * scalar rules.  The scene is copied; the caller keeps ownership.  The
 * default one-wave kernels read every scene from HBM through the caches; the
 * four-wave kernels (rt_device_options OneWaveGroups off) also stage scenes of up to 656 spheres (164
 * groups) in each block's LDS.  Up to RT_MAX_SPHERES.
 * RT_EINVAL for a scene with no spheres (every built-in scene has some) or
 * more than RT_MAX_SPHERES. */
#define RT_MAX_SPHERES 16384u
int rt_scene_upload(rt_device *dev, const rt_scene *scene);

/* --------------------------------------------------------------- tracing */

#define RT_SEED_PIXEL 1u        /* per-(pixel, frame) PCG seed (GPU parity mode) */
#define RT_FLAG_ACCUM_ZERO 1u   /* PreviousImage treated as all-zero (not read) */
#define RT_FLAG_SRGB_POW 2u     /* RGBA8 through LinearToSRGB's exact-pow branch (main.cpp:320-321, '#if 0'
                                   in the reference) instead of its sqrt one; PreviousImage is unaffected */

typedef struct rt_trace_desc {
    uint32_t Width, Height;   /* full image (CurrentImage.Width/Height)          */
    uint32_t PreviousRayCount;/* frames already folded into PreviousImage (main.cpp:7) */
    uint32_t Frames;          /* progressive frames (samples/pixel) to fold now  */
    uint32_t MaxBounce;       /* the reference literal is 5 (main.cpp:387)       */
    uint32_t EnableSIMD;      /* 1 RenderTile rules, 0 RenderTileScalar rules    */
    uint32_t SeedMode;        /* RT_SEED_PIXEL                                   */
    uint32_t BandRows;        /* row-band height, a multiple of 8 (bench: 8)     */
    uint32_t BandCount;       /* bands are dealt round-robin over BandCount GPUs */
    uint32_t BandIndex;       /* this GPU's residue                              */
    uint32_t Flags;           /* RT_FLAG_*                                       */
} rt_trace_desc;

/* Number of image rows owned by band residue `band_index` (the compact
 * per-GPU framebuffer height). */
uint32_t rt_band_local_rows(uint32_t height, uint32_t band_rows, uint32_t band_count, uint32_t band_index);

/* Replaces WorkQueueStart(RenderTile|RenderTileScalar, TilesX*TilesY, N)
 * (main.cpp:851-856) for `Frames` consecutive frames: traces every pixel
 * of this GPU's bands, folds each frame into the running mean and stores
 * the sRGB RGBA8 of the last one.  cam->CurrentImage.Data and
 * cam->PreviousImage.Data are DEVICE pointers to compact band-local images
 * (rt_band_local_rows x Width).  `d_rays` (device u64) is incremented by
 * the bounce segments traced (RaysCastInThread, main.cpp:390).
 * Asynchronous on `stream` (hipStream_t; NULL = the HIP null stream): the
 * host never waits.  The first launch for a new camera / scene / geometry on
 * this device runs the primary-ray cull pass; its live-tile count stays on
 * the device (the trace grid covers every tile and blocks past the count
 * exit) until it has reached the host asynchronously, after which launches
 * of the same key size their grids exactly.  Launches of one device are meant
 * for one stream: when the stream changes between launches, the call first
 * waits for the device (host-side), as it does when it grows its buffers for
 * a larger geometry than any before.  PreviousRayCount + Frames must fit a u32. */
int rt_trace(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc,
             uint64_t *d_rays, void *stream);

/* The reference hands its workers 32 x 32 tiles: WorkQueueStart(RenderTile, TilesX*TilesY, ..)
 * gives each a WorkEntry, RenderTile turns it into TileX = Tile % TilesX, TileY = Tile / TilesX
 * and clips the tile to the image (main.cpp:9, 362-368, 851-856). */
#define RT_TILE_SIZE 32u   /* TileSize, main.cpp:9 */
/* TilesX*TilesY of a width x height image as OnRender forms them (ceil division);
 * *out_tiles_x (optional) = TilesX.  0 for an empty or oversized (> 65536) image. */
uint32_t rt_tile_count(uint32_t width, uint32_t height, uint32_t *out_tiles_x);

/* rt_trace over the listed tiles only: the caller's own tile queue, part of a frame, more
 * samples for some tiles than for others, or the one tile that holds a pixel in question.
 * tiles: HOST array of n_tiles WorkEntry values, Tile = TileY*TilesX + TileX with
 * TilesX = ceil(Width/32), each tile clipped to the image as main.cpp:362-368 does.  Any order.
 *  - Every pixel of a listed tile receives exactly the running mean and RGBA8 that rt_trace with
 *    the same desc writes for it (a pixel's seeds, samples and fold never depend on what else
 *    a launch traces).  No byte of any other pixel of CurrentImage or PreviousImage is written.
 *  - Both images are the full Width x Height device images, as for rt_trace with one band.
 *    BandCount must be 0 or 1 and BandIndex 0 (RT_EINVAL otherwise); BandRows is accepted as for
 *    rt_trace; cam->TilesX is not read (rt_trace does not read it either).
 *  - *d_rays grows by the bounce segments of the listed tiles' pixels only, traced ones and those
 *    counted analytically (dead tiles).  A list naming every tile gives rt_trace's bits and count.
 *  - PreviousRayCount is per call, as for rt_trace: frame k's seeds and weights depend on
 *    PreviousRayCount + k only, so a caller whose tiles carry different sample counts keeps one
 *    count per tile and lists together the tiles that share one (or hands every tile's own
 *    count to rt_trace_tile_work, below, in one call).
 *  - RT_EINVAL, before anything is enqueued: tiles == NULL with n_tiles > 0, an index >=
 *    rt_tile_count(Width, Height), an index named twice (the reference's queue would fold that
 *    tile twice; the library refuses rather than guess), and everything rt_trace refuses.
 *    n_tiles == 0 or Frames == 0: RT_OK, nothing enqueued.
 *  - The host array is consumed before the call returns: free or overwrite it at once.
 *  - The selection is part of the launch key (camera, scene, geometry, lanes per pixel, list --
 *    compared by content): the same list again reuses the cull masks, tile order and pixel
 *    permutation; a different list is a new key and pays a cull pass, the first-launch split
 *    and a fresh order.  Only the last key is kept.
 *  - With rt_device_options LanesPerPixel left at its default, the lanes per pixel follow the
 *    listed tiles' (clipped) pixel count per CU, not the frame's: a small window runs at 16 lanes
 *    per pixel, as a small rank share does.
 *  - Asynchronous on `stream` exactly like rt_trace; the host waits where rt_trace would (stream
 *    switch, buffer growth) and in one more place: a new list is uploaded from one of two pinned
 *    staging slots the library owns, and the call waits for a slot's previous upload (two new
 *    lists earlier) if that copy has not finished yet. */
int rt_trace_tiles(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc,
                   const uint32_t *tiles, uint32_t n_tiles, uint64_t *d_rays, void *stream);

/* one entry of a caller's tile queue: the reference's WorkEntry plus the tile's own counts */
typedef struct rt_tile_work {
    uint32_t Tile;             /* TileY*TilesX + TileX, as rt_trace_tiles                     */
    uint32_t PreviousRayCount; /* frames already folded into this tile's pixels               */
    uint32_t Frames;           /* frames to fold into them now; 0: the entry is dropped       */
} rt_tile_work;

/* rt_trace_tiles with a (PreviousRayCount, Frames) pair per tile, in one launch: the dispatch of an
 * adaptive or progressive sampler whose tiles sit at different sample counts.  Nothing in RenderTile
 * couples a tile's frame count to another's (main.cpp:362-368, 484-487); the host keeps one count per
 * tile.  work: HOST array of n_work entries, any order.  rt_trace_tiles' contract holds, except:
 *  - Every pixel of an entry's tile receives exactly the running mean and RGBA8 that rt_trace writes
 *    for it when desc->PreviousRayCount / Frames are replaced by the entry's values.  No byte of any
 *    other pixel of either image is written, the tiles of entries with Frames == 0 included.
 *    desc->PreviousRayCount and desc->Frames are not read.
 *  - *d_rays grows by the listed tiles' segments, each tile contributing its own frames, traced or
 *    counted analytically (dead tiles).
 *  - RT_FLAG_ACCUM_ZERO and RT_FLAG_SRGB_POW apply to the whole call; an entry with
 *    PreviousRayCount == 0 does not read its pixels' mean, as rt_trace does not.
 *  - RT_EINVAL, before anything is enqueued or any key state changes: what rt_trace_tiles refuses
 *    (work == NULL with n_work > 0, an index out of range, an index listed twice, bands), and an
 *    entry whose PreviousRayCount + Frames does not fit a u32.  A tile listed twice is refused even
 *    when one of its entries has Frames == 0: duplicates are refused before such entries are dropped.
 *    n_work == 0, or every entry at Frames == 0: RT_OK, nothing enqueued.
 *  - The counts are no part of the launch key.  The key holds the list of tiles with Frames > 0
 *    (compared by content) and nothing of their counts: the same tiles with other counts reuse the
 *    cull masks, the tile order and the pixel permutation (CullPassRan 0), and the key is the same
 *    whether the list came from rt_trace_tiles or from here.
 *  - The per-tile table (two words per tile of the image) is uploaded on every call with mixed counts,
 *    from one of two pinned staging slots the library owns, like a new list's bitmap; the host array
 *    is consumed before the call returns.  The call may wait where rt_trace_tiles may wait and for a
 *    table slot's previous upload (two such calls earlier), nothing else.  rt_device_reserve also
 *    sizes the table and its staging.
 *  - When every kept entry has the same pair, the call IS rt_trace_tiles with that pair: the same
 *    path and kernels, the first-launch split and the 4-pixels-per-lane shape at Frames == 1 included
 *    (rt_trace_last_tile_counts 0).
 *  - Mixed counts (rt_trace_last_tile_counts 1): the first-launch split does not apply (SplitHeadFrames 0; a
 *    per-tile split is not built).  With LanesPerPixel at its default the lanes follow the listed
 *    pixel count per CU, as for rt_trace_tiles, and never exceed the LARGEST Frames of the list; at
 *    a largest Frames of 1 the launch takes the 4-pixels-per-lane shape.  The trace kernels are the
 *    launch's usual ones compiled to take each block tile's pair from the table; the four-wave
 *    kernels (OneWaveGroups off) exist so for a scene in the LDS image read through the scalar cache
 *    only -- with SphereSourceLds or SceneInHbm on, or a scene beyond the LDS image, a mixed launch of
 *    such a device runs the one-wave run-time kernel (OneWaveGroups 1, Walk 0 in rt_trace_info; the
 *    wave-ranked order makes it another key than the device's uniform launches of that list). */
int rt_trace_tile_work(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc,
                       const rt_tile_work *work, uint32_t n_work, uint64_t *d_rays, void *stream);

/* How far the RGB bytes of one 32x32 reference tile (clipped to the image) moved. Alpha is not looked at. */
typedef struct rt_tile_delta {
    uint32_t Changed;    /* pixels with R, G or B different                       (<= 1024)        */
    uint32_t MaxDelta;   /* largest |new - old| over the tile's R, G, B bytes     (<= 255)         */
    uint32_t SumDelta;   /* sum of |new - old| over R, G, B of every pixel        (<= 783,360)     */
    uint32_t SumSquares; /* sum of (new - old)^2 over the same                    (<= 199,756,800) */
} rt_tile_delta;         /* 16 B */

/* rt_trace_tile_work that also tells, per listed tile, how far this call moved the tile's displayed
 * pixels: the decision half of an adaptive sampler (which tiles are still noisy, how many frames they
 * want next), computed on the device by the pass that stores the RGBA8 bytes, 16 B per tile instead of
 * an image copied to the host.  rt_trace_tile_work's whole contract holds -- the bits of both images,
 * the ray count, what is refused, the launch key, the routing of uniform and mixed pairs,
 * rt_trace_last_tile_counts, where the call may wait -- with one addition:
 *  - d_delta: DEVICE array of rt_tile_count(Width, Height) entries, 16-byte aligned, indexed by Tile.
 *    For every kept entry (Frames > 0), d_delta[Tile] receives the statistics of that tile's pixels
 *    (clipped to the image) between "old", what CurrentImage held at the pixel before this call in
 *    stream order, and "new", the RGBA8 this call stores there (RT_FLAG_SRGB_POW honoured).  The
 *    pixels of dead (folded) block tiles are included: the same pass encodes them.
 *  - Entries of tiles not listed, or listed with Frames == 0, are not written.  Nothing needs zeroing
 *    beforehand.  Written asynchronously on `stream`, like the images.
 *  - The caller owns the meaning of "old".  The library keeps no frame of its own: on a tile's first
 *    round "old" is whatever the caller put into CurrentImage (a cleared image, the last frame shown,
 *    uninitialised memory), and the first round's statistics measure the distance from that, not any
 *    error.  Statistics are comparable from the second round of a tile on, where "old" is what the
 *    previous round stored.
 *  - d_delta == NULL or not 16-byte aligned: RT_EINVAL, before anything is enqueued or any key state
 *    changes.  n_work == 0, or every entry at Frames == 0: RT_OK, nothing enqueued, nothing written.
 *  - The statistics are no part of the launch key: the same tiles through rt_trace_tile_work,
 *    rt_trace_tiles and this call share one key (CullPassRan 0 on the second of them).
 *  - RGBA8 is stored by the closing pass at every launch shape (also where rt_trace_tile_work's
 *    kernels would store it themselves: one frame, or rt_device_options EncodePass off); the bytes
 *    are the same.  No buffer, staging or wait beyond rt_trace_tile_work's; rt_device_reserve covers it.
 * The statistics are integers with no summation order: a given (old, new) pair of images has one result. */
int rt_trace_tile_work_delta(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc,
                             const rt_tile_work *work, uint32_t n_work, rt_tile_delta *d_delta,
                             uint64_t *d_rays, void *stream);

/* The same statistics between two RGBA8 images (DEVICE pointers, width x height u32 each), for every
 * tile of the image: d_delta[Tile] for all rt_tile_count(width, height) tiles.  For a host that keeps
 * two frames, as rt_on_render does.  Needs no rt_device and traces nothing; enqueued on `stream`
 * (NULL: the null stream) of the current HIP device.  RT_EINVAL for a NULL pointer, a d_delta that is
 * not 16-byte aligned, or an image for which rt_tile_count is 0. */
int rt_tile_delta_rgba8(const uint32_t *d_old, const uint32_t *d_new, uint32_t width, uint32_t height,
                        rt_tile_delta *d_delta, void *stream);

/* one entry per tile of the image (rt_tile_count(Width, Height) entries, indexed by Tile), DEVICE memory */
typedef struct rt_tile_counts {
    uint32_t PreviousRayCount; /* frames already folded into this tile's pixels                   */
    uint32_t Frames;           /* frames the tile wants folded by the next launch; 0: it rests    */
} rt_tile_counts;              /* 8 B */

/* rt_trace_tile_work_delta whose per-tile pairs live on the device: the refinement loop of an adaptive
 * sampler enqueued on one stream with no host wait.  The host names the tiles that MAY be traced; the
 * device table says, when the launch runs, how many frames each of them folds -- none, for a tile that
 * rests.  rt_trace_tile_work_delta's contract holds with these differences:
 *  - tiles: HOST array, the superset of tiles the call may trace.  Validated and keyed exactly as
 *    rt_trace_tiles does it -- the same refusals, the same key -- so the key depends on nothing the
 *    device holds: the same list again gives CullPassRan 0 whatever the table has become, tiles that came
 *    to rest included, and the key is shared with rt_trace_tiles and with a mixed rt_trace_tile_work call
 *    over the same tiles on this device.
 *  - d_counts: DEVICE table of rt_tile_count(Width, Height) entries.  A listed tile takes its pair from
 *    d_counts[Tile] at the moment the launch runs in stream order (write it on `stream` before the call:
 *    rt_tile_counts_step below, a copy, the caller's own kernel).  The host never reads the table.
 *    Entries of unlisted tiles are ignored, whatever they hold.
 *  - A listed tile folds min(Frames, max_frames) frames from its PreviousRayCount; where PreviousRayCount
 *    plus that many does not fit a u32 it folds 0 (the device cannot refuse an entry as the host does).
 *  - A listed tile that folds 0 frames rests: no byte of either image is written for it, its d_delta
 *    entry is not written, and it adds nothing to *d_rays or SegmentsFolded -- whether its block tiles
 *    are live or dead.  With every listed tile at rest the call is RT_OK and writes nothing (launches are
 *    still enqueued: the host does not know).  TilesSelected and TilesTraced count the listed tiles'
 *    block tiles, resting ones included.
 *  - max_frames, an upper bound of any entry's Frames, takes the place of "the LARGEST Frames of the
 *    list" in the launch shape: the lanes per pixel never exceed it, and max_frames == 1 gives the
 *    4-pixels-per-lane shape.  Keep it fixed over a loop: the shape is part of the key.
 *    desc->PreviousRayCount and desc->Frames are not read.
 *  - The call always routes as rt_trace_tile_work with mixed pairs does: no first-launch split, the
 *    four-wave kernels only where that call has them, rt_trace_last_tile_counts 1, SegmentsFolded summed
 *    on the device.
 *  - d_delta: DEVICE, 16-byte aligned, as for rt_trace_tile_work_delta (entries of the tiles that folded
 *    a frame are written), or NULL: no statistics, and RGBA8 is stored as rt_trace_tile_work stores it.
 *  - RT_EINVAL, before anything is enqueued or any key state changes: d_counts == NULL, max_frames == 0,
 *    d_delta neither NULL nor 16-byte aligned, and everything rt_trace_tiles refuses.  n_tiles == 0: RT_OK,
 *    nothing enqueued.
 *  - No pinned staging is used for the table: one small pass on `stream` copies the listed tiles' pairs,
 *    clamped as above, into the library's own table.  The host waits only where rt_trace_tiles may wait
 *    (a NEW list's bitmap upload); rt_device_reserve covers the call. */
int rt_trace_tile_counts(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc,
                         const uint32_t *tiles, uint32_t n_tiles, const rt_tile_counts *d_counts,
                         uint32_t max_frames, rt_tile_delta *d_delta, uint64_t *d_rays, void *stream);

/* The library's per-tile stopping rule, run on the device between two rt_trace_tile_counts calls. */
typedef struct rt_tile_rule {
    uint32_t Size;            /* sizeof(rt_tile_rule)                                             */
    uint32_t MaxRoundFrames;  /* >= 1: the max_frames given to rt_trace_tile_counts               */
    uint32_t MaxTileFrames;   /* >= 1: a tile rests once PreviousRayCount reaches it              */
    uint32_t RestMaxDelta;    /* a tile rests when its round's MaxDelta <= this ...               */
    uint32_t RestSumSquares;  /* ... and SumSquares <= this (0xFFFFFFFF: not looked at)           */
} rt_tile_rule;
typedef struct rt_tile_step_summary {
    uint64_t NextFrames;      /* frames the next round folds, over all tiles                      */
    uint32_t ActiveTiles;     /* tiles the next round traces                                      */
    uint32_t RestedNow;       /* tiles this step put to rest                                      */
} rt_tile_step_summary;       /* 16 B */

/* Advances a device table by the round rt_trace_tile_counts(.., rule->MaxRoundFrames, d_delta, ..) just
 * traced and decides each tile's next one.  Like rt_tile_delta_rgba8 it needs no rt_device and is
 * enqueued on `stream` of the current HIP device.  For every tile of the width x height image, with f the
 * frames its entry folded in that round (min(Frames, MaxRoundFrames), or 0 where the sum with
 * PreviousRayCount does not fit a u32):
 *  - f == 0: the entry is left as it is (a resting tile stays at rest until the caller wakes it).
 *  - else done = PreviousRayCount + f, and the tile rests when done >= MaxTileFrames, or when
 *    PreviousRayCount != 0 and its d_delta entry has MaxDelta <= RestMaxDelta and SumSquares <=
 *    RestSumSquares (a tile's first round never rests on its statistics: they measure the distance from
 *    whatever the caller had in CurrentImage).  The entry becomes {done, 0} at rest, else
 *    {done, min(done, MaxRoundFrames, MaxTileFrames - done)}: as many frames again as the tile has.
 *  - d_summary (DEVICE, or NULL): the sum of the new Frames of the entries this step advanced, how many
 *    of them are > 0, and how many tiles it put to rest -- what the next round will do (entries left as
 *    they are fold nothing then either).  Written, never accumulated: nothing needs zeroing, no atomics,
 *    one value for a given input.  Copy its 16 B back asynchronously to learn when to stop.
 * Tiles the trace call did not list must hold Frames == 0 (their d_delta entries were not written).
 * RT_EINVAL for a NULL d_counts, d_delta or rule, a wrong Size, a zero MaxRoundFrames or MaxTileFrames, a
 * d_delta that is not 16-byte aligned, or an image for which rt_tile_count is 0.  A caller's own kernel
 * may write the table instead: this is the library's rule, not the only one. */
int rt_tile_counts_step(rt_tile_counts *d_counts, const rt_tile_delta *d_delta, uint32_t width, uint32_t height,
                        const rt_tile_rule *rule, rt_tile_step_summary *d_summary, void *stream);

/* ------------------------------------------------- what a pixel sees: the first hit */

#define RT_HIT_MISS   0xFFFFFFFFu   /* rt_first_hit.Key of a pixel whose primary ray hits nothing      */
#define RT_HIT_INSIDE 0x80000000u   /* bit 31 of Key: the reference's InsideSphere flag of the winner  */
#define RT_HIT_PIXEL_CENTRE 1u      /* flags: Jx = Jy = 0, no RNG draw                                  */

typedef struct rt_first_hit {       /* 8 B per pixel */
    uint32_t Key;                   /* MaterialIndex (4*group + lane == index into ScalarSpheres), | RT_HIT_INSIDE; or RT_HIT_MISS */
    float    T;                     /* MinT of the first segment (main.cpp:413-429); 1e30f (F32Max) on a miss */
} rt_first_hit;

typedef struct rt_first_hit_planes {
    uint32_t      Size;             /* sizeof(rt_first_hit_planes) */
    rt_first_hit *Hit;              /* DEVICE, Width*Height entries, 8-byte aligned, or NULL  */
    float        *Normal;           /* DEVICE, Width*Height v4 f32, 16-byte aligned, or NULL  */
    float        *Albedo;           /* DEVICE, Width*Height v4 f32, 16-byte aligned, or NULL  */
} rt_first_hit_planes;

/* The first segment of every pixel's path as a pass of its own: which sphere the primary ray hits, how
 * far away, with which normal and which surface colour -- for picking, for a denoiser's or a stopping
 * rule's guide images, and for naming the sphere behind a pixel in question.  New; the reference keeps
 * these values inside RenderTile's first loop iteration (main.cpp:375-444).
 *  - The ray is the primary ray of frame k = desc->PreviousRayCount of rt_trace with the same cam, Width
 *    and Height: the seed rt_pixel_seed(x, y, k, Width, Height), two RandomFloat draws, the film point
 *    and Normalize of main.cpp:375-385 -- the trace kernel's own function.  With RT_HIT_PIXEL_CENTRE in
 *    `flags` both jitters are exactly 0.0f and no RNG is touched; every later operation is the same
 *    sequence.  desc->Frames, MaxBounce, Flags and the image fields of cam are not read.
 *  - The hit is the reference's first loop iteration under the rule set desc->EnableSIMD selects, sphere
 *    loop and hit select: the SIMD rules' per-class minima, first-equal-lane select and sticky inside
 *    flag (main.cpp:399-444), or the scalar rules' "later sphere wins a tie" and non-sticky flag
 *    (main.cpp:541-578).  The same device functions as the trace kernel's first segment, so the same bits.
 *  - Hit[y * Width + x] = {MaterialIndex | inside << 31, MinT} of the winner.  Normal = Normalize(D * MinT
 *    - C), negated when the inside flag is set, as the shading step forms HitNormal (main.cpp:423-429,
 *    452-457), with w = 0 -- the reference's Normalize, so the zero vector where the squared length, the winner's
 *    r^2, is <= 1e-4 (x64_math.h:234-245).  Albedo = the winner's Material.Color.xyz with w = 1.  A miss writes
 *    {RT_HIT_MISS, 1e30f} and zeros to the other two planes (Albedo.w = 0 marks it).
 *  - tiles == NULL with n_tiles == 0 selects every tile of the image.  Otherwise tiles is a HOST list of
 *    reference tiles validated exactly as rt_trace_tiles validates its list (the same refusals, the same
 *    clipping), consumed before the call returns.  Only the pixels of listed tiles are written, in each
 *    non-NULL plane: no byte of any other pixel, and nothing at all in a NULL plane.  A non-NULL list with
 *    n_tiles == 0 returns RT_OK with nothing enqueued.
 *  - RT_EINVAL, before anything is enqueued or changed: a NULL dev, cam, desc or out; a wrong Size; all
 *    three planes NULL; a misaligned plane; a flag bit other than RT_HIT_PIXEL_CENTRE; SeedMode other than
 *    RT_SEED_PIXEL; BandCount not 0 or 1, or BandIndex != 0; an image for which rt_tile_count is 0; no
 *    uploaded scene; tiles == NULL with n_tiles > 0, a tile index out of range or named twice.  The rsqrt
 *    table is not required: the pass never calls NormalizeFast.
 *  - No effect on tracing: the pass takes no d_rays and counts nothing; it neither reads nor creates nor
 *    replaces the device's launch key, cull masks, tile order, costs or pixel permutation (it culls inside
 *    its kernel, per 8x8 pixel tile, and keeps nothing); rt_trace_last_info and rt_trace_last_tile_counts
 *    report after the call what they reported before it, and the next rt_trace of an unchanged key has
 *    CullPassRan == 0.
 *  - Asynchronous on `stream` under the stream rule of rt_trace (one stream per device; a switch waits for
 *    the device); rt_scene_upload waits for this pass as it waits for trace launches.  A tile list is
 *    uploaded through a bitmap and pinned staging of the pass's own; rt_device_reserve covers them for its
 *    width x local_rows, and the call waits only where rt_trace_tiles may wait. */
int rt_trace_first_hit(rt_device *dev, const rt_camera_info *cam, const rt_trace_desc *desc,
                       const uint32_t *tiles, uint32_t n_tiles, uint32_t flags,
                       const rt_first_hit_planes *out, void *stream);

/* ------------------------------------------------- a filter over the first-hit planes */

#define RT_DENOISE_DEMODULATE 1u   /* divide by the first hit's albedo before, multiply back after */
#define RT_DENOISE_SRGB_POW   2u   /* Rgba8 through the exact-pow branch, as RT_FLAG_SRGB_POW        */
#define RT_DENOISE_MAX_ITERATIONS 8u

typedef struct rt_denoise_desc {
    uint32_t Size;                 /* sizeof(rt_denoise_desc)                                        */
    uint32_t Width, Height;        /* rt_tile_count(Width, Height) != 0                              */
    uint32_t Iterations;           /* 1..8 passes; pass i (from 0) samples at step 2^i               */
    uint32_t Flags;
    uint32_t NormalPower;          /* 0: no normal stop; k in 1..8: max(0, Np.Nq)^(2^k)              */
    float    SigmaDepth;           /* 0: no depth stop; else relative to the centre's T; finite, >0  */
    float    SigmaColor;           /* 0: no colour stop; else luminance width of pass 0, halved per pass */
    const float        *Mean;      /* DEVICE v4 f32, Width*Height, 16-byte aligned (PreviousImage)   */
    const rt_first_hit *Hit;       /* DEVICE, 8-byte aligned, required                               */
    const float        *Normal;    /* DEVICE v4 f32, required when NormalPower != 0, else may be NULL */
    const float        *Albedo;    /* DEVICE v4 f32, required with RT_DENOISE_DEMODULATE             */
    float              *Out;       /* DEVICE v4 f32, required                                        */
    float              *Scratch;   /* DEVICE v4 f32, required when Iterations >= 2                   */
    uint32_t           *Rgba8;     /* DEVICE or NULL: ColorFromV4(LinearToSRGB(Out))                 */
} rt_denoise_desc;

/* An edge-avoiding a-trous filter of a running mean (rt_trace's PreviousImage) guided by rt_trace_first_hit's
 * planes of the same frame.  New; the reference has no filter.  Like rt_encode_rgba8 and rt_tile_delta_rgba8 the
 * pass needs no rt_device, keeps no state, allocates nothing and does not wait on the host: one kernel launch
 * per pass on `stream` (NULL: the null stream) of the current HIP device, alternating between Scratch and Out so
 * that the last pass lands in Out (Iterations == 1: Mean -> Out, Scratch is never touched).  The inputs are only
 * read; no byte outside Out, Scratch (when used) and Rgba8 (when given) is written.
 *
 * The result is defined operation by operation; every operation is one IEEE f32 operation (no contraction,
 * IEEE division, denormals kept), so it is one set of bits (tests/denoise_ref.py restates it in numpy):
 *    K = {1/16, 1/4, 3/8, 1/4, 1/16};  lum(c) = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z;
 *    pos(v) = v > 0 ? v : 0 (NaN gives 0);  ic0 = 1.0f / SigmaColor, once on the host;
 *    pass i: s = 1 << i, ic = ic0 * (float)s.  I_0 = Mean; with RT_DENOISE_DEMODULATE I_0.ch = Mean.ch / a.ch,
 *    a.ch = Albedo.ch > 0.01f ? Albedo.ch : 0.01f where Albedo.w == 1 and a = 1 elsewhere (a miss).
 *  - Centre p = (x, y): kp = Hit[p].Key, tp = Hit[p].T, lp = lum(I_i[p]); rz = 1.0f / (SigmaDepth * tp), formed
 *    only when SigmaDepth > 0 and kp != RT_HIT_MISS.
 *  - acc = (+0, +0, +0), ws = +0.  Taps dy = -2..2 (outer), dx = -2..2 (inner) at q = (x + dx*s, y + dy*s); a
 *    tap outside the image is skipped.  w = K[dy+2] * K[dx+2]; the centre tap keeps that w.  Any other tap:
 *      Hit[q].Key != kp (the whole word, RT_HIT_INSIDE included): skipped.
 *      kp != RT_HIT_MISS and NormalPower = k > 0: d = pos((Np.x*Nq.x + Np.y*Nq.y) + Np.z*Nq.z), k times d = d*d,
 *        w = w*d.
 *      kp != RT_HIT_MISS and SigmaDepth > 0: w = w * pos(1.0f - fabsf(tp - Hit[q].T) * rz).
 *      SigmaColor > 0, hits and misses alike: w = w * pos(1.0f - fabsf(lp - lum(I_i[q])) * ic).
 *    A tap whose w is not > 0 is skipped (so an infinite or NaN neighbour never enters a pixel it does not
 *    belong to); otherwise acc.ch = acc.ch + w * I_i[q].ch per channel and ws = ws + w.
 *  - I_{i+1}[p].ch = acc.ch / ws (the centre gives ws >= 9/64); I_{i+1}[p].w = Mean[p].w.
 *  - After the last pass the demodulated variant multiplies back, Out.ch = I_n.ch * a.ch, and Rgba8[p] is the
 *    RGBA8 of Out.xyz as rt_trace and rt_encode_rgba8 encode it (RT_DENOISE_SRGB_POW: the exact-pow branch).
 * The falloffs are tents, not exponentials: no transcendental, so one result.
 *
 * RT_EINVAL, with an rt_last_error text and before anything is enqueued: a NULL desc or a wrong Size; a size
 * for which rt_tile_count is 0; Iterations outside 1..8; an unknown flag bit; NormalPower > 8; a sigma that is
 * negative, NaN or infinite; a required pointer that is NULL; a misaligned plane (Mean, Normal, Albedo, Out,
 * Scratch 16 bytes, Hit 8, Rgba8 4); two of Mean, Out and Scratch that are the same pointer. */
int rt_denoise(const rt_denoise_desc *desc, void *stream);
/* Fills *out with Size, Width = Height = 0, Flags = 0, every pointer NULL and the library's defaults:
 * Iterations = 3 (steps 1, 2, 4: a 29 x 29 footprint), NormalPower = 2 (max(0, Np.Nq)^4), SigmaDepth = 0.25f
 * (a tap's weight reaches 0 where its depth differs by a quarter of the centre's), SigmaColor = 0.5f (a tap's
 * weight reaches 0 at a luminance difference of 0.5 in pass 0, 0.25 in pass 1, 0.125 in pass 2: the built-in
 * scenes are mirrors and glass, whose reflections a filter without a colour stop blurs into a larger error
 * than the noise it removes).  Chosen on the CPU restatement over 4-spp frames of the three built-in scenes
 * against their 1024-spp means (DESIGN.md has the table).  RT_EINVAL for NULL. */
int rt_denoise_defaults(rt_denoise_desc *out);

/* ------------------------------------------------- the running mean across a camera move */

#define RT_REPROJECT_SRGB_POW 2u   /* Rgba8 through the exact-pow branch, as RT_FLAG_SRGB_POW */

typedef struct rt_reproject_desc {
    uint32_t Size;                 /* sizeof(rt_reproject_desc)                                       */
    uint32_t Width, Height;        /* rt_tile_count(Width, Height) != 0                               */
    uint32_t Frames;               /* >= 1: frames folded into Mean (traced from PreviousRayCount 0)   */
    uint32_t MaxHistory;           /* >= Frames: cap of a pixel's history length                      */
    uint32_t Flags;                /* RT_REPROJECT_SRGB_POW or 0                                      */
    float    DepthTolerance;       /* 0: no depth test; else relative to the distance; finite, > 0    */
    const rt_camera_info *Camera;          /* HOST: the camera of Mean and Hit                        */
    const rt_camera_info *PreviousCamera;  /* HOST: the camera of the history planes                  */
    const float        *Mean;      /* DEVICE v4 f32, Width*Height, 16-byte aligned: the fresh mean    */
    const rt_first_hit *Hit;       /* DEVICE, 8-byte aligned: rt_trace_first_hit, RT_HIT_PIXEL_CENTRE, at Camera */
    const float        *History;       /* DEVICE v4 f32: the previous call's Out      | all three NULL: */
    const rt_first_hit *HistoryHit;    /* DEVICE: the previous call's Hit             | no history, a   */
    const uint32_t     *HistoryCount;  /* DEVICE u32, 4-byte aligned: its OutCount    | loop's first frame */
    float              *Out;       /* DEVICE v4 f32, required                                         */
    uint32_t           *OutCount;  /* DEVICE u32, required: frames behind each pixel of Out           */
    uint32_t           *Rgba8;     /* DEVICE or NULL: ColorFromV4(LinearToSRGB(Out))                  */
} rt_reproject_desc;

/* Carries an accumulated frame across a camera move.  New; the reference's OnRender drops its running mean on
 * every move (main.cpp:791-806).  For each pixel of the new frame the pass finds where the surface point the
 * pixel sees lay in the previous frame, gathers the accumulated colour there from the pixels that saw the same
 * sphere at a consistent distance, and folds the fresh mean into it; a pixel with no such history starts again
 * from the fresh mean.  A miss never takes history, and what a mirror shows does not follow its surface:
 * MaxHistory bounds how long either error can live.  Like rt_denoise the pass needs no rt_device, keeps no state,
 * allocates nothing and does not wait on the host: one kernel launch on `stream` (NULL: the null stream) of the
 * current HIP device.  The cameras are HOST structs as rt_camera_setup makes them, consumed before the call
 * returns; only CameraPosition, CameraX, CameraY, FilmCenter, FilmW and FilmH are read, and CameraX and CameraY
 * are taken to be unit vectors orthogonal to FilmCenter - CameraPosition.  The inputs are only read; no byte
 * outside Out, OutCount and Rgba8 (when given) is written.  The loop: rt_trace at PreviousRayCount 0 into Mean,
 * rt_trace_first_hit with RT_HIT_PIXEL_CENTRE into Hit, rt_reproject, optionally rt_denoise of Out for display, then
 * Out, Hit, OutCount become History, HistoryHit, HistoryCount and the camera PreviousCamera.
 *
 * The result is defined operation by operation; every operation is one IEEE f32 operation (no contraction, IEEE
 * division and square root, denormals kept), so it is one set of bits (tests/reproject_ref.py restates it in numpy):
 *    dot3(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z;  primes mark PreviousCamera's fields.
 *  - Host, once: fv.c = FilmCenter'.c - CameraPosition'.c; ff = dot3(fv, fv); Wf = (float)Width, Hf = (float)Height;
 *    hw = Wf * 0.5f, hh = Hf * 0.5f.
 *  - Pixel p = (x, y): kp = Hit[p].Key, tp = Hit[p].T.
 *  1 Fresh: with History == NULL or kp == RT_HIT_MISS the pixel is fresh: Out.ch = Mean.ch, OutCount = Frames.
 *  2 Direction, the pixel-centre primary ray of rt_trace_first_hit: fx = -1.0f + ((float)x * 2.0f) / Wf, fy
 *    likewise; kx = (fx * FilmW) * 0.5f, ky = (fy * FilmH) * 0.5f; P.c = (FilmCenter.c + kx * CameraX.c) + ky *
 *    CameraY.c; D = Normalize(P - CameraPosition), the reference's Normalize (x64_math.h:234-245): v.c /
 *    sqrtf(dot3(v, v)), the zero vector where dot3(v, v) <= 1e-4f.
 *  3 Point: X.c = CameraPosition.c + D.c * tp; V.c = X.c - CameraPosition'.c.
 *  4 Projection: u = dot3(V, CameraX'), v = dot3(V, CameraY'), d = dot3(V, fv); qx = (u / d) * ff;
 *    sx = (((qx * 2.0f) / FilmW') + 1.0f) * hw; sy likewise from v, FilmH' and hh (a pixel's centre sits at its
 *    integer coordinate: the reference's jitter is in [-0.5, 0.5)).  te = sqrtf(dot3(V, V)), lim = DepthTolerance * te.
 *  5 Range: the pixel is fresh unless d > 0 && sx >= -1.0f && sx < Wf && sy >= -1.0f && sy < Hf (a NaN fails).
 *    x0 = floorf(sx), ax = sx - x0; y0 = floorf(sy), ay = sy - y0.
 *  6 Taps q = (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), in that order, w = wx * wy with wx = 1.0f - ax
 *    at x0 and ax at x0 + 1, wy alike.  acc = (+0, +0, +0), ws = +0, n = 0xFFFFFFFF.  A tap is skipped when it is
 *    outside the image; when w is not > 0; when HistoryCount[q] == 0; when HistoryHit[q].Key != kp (the whole word,
 *    RT_HIT_INSIDE included); when a channel of History[q].xyz is not finite (a NaN would live in the history for
 *    ever); and, with DepthTolerance > 0, when !(fabsf(te - HistoryHit[q].T) <= lim) (the far side of the same
 *    sphere).  A tap that is kept: acc.ch = acc.ch + w * History[q].ch, ws = ws + w, n = min(n, HistoryCount[q]).
 *  7 Fold: no tap kept: the pixel is fresh.  Else n = min(n, MaxHistory), H.ch = acc.ch / ws, a = (float)Frames /
 *    ((float)n + (float)Frames), Out.ch = H.ch + (Mean.ch - H.ch) * a, OutCount = min(n + Frames, MaxHistory) (the
 *    sum formed without wrapping).
 *  8 Out.w = Mean[p].w; Rgba8[p], when given, is the RGBA8 of Out.xyz as rt_trace and rt_encode_rgba8 encode it
 *    (RT_REPROJECT_SRGB_POW: the exact-pow branch).
 *
 * RT_EINVAL, with an rt_last_error text and before anything is enqueued: a NULL desc or a wrong Size; a size for
 * which rt_tile_count is 0; Frames == 0 or MaxHistory < Frames; an unknown flag bit; a DepthTolerance that is
 * negative, NaN or infinite; a NULL Camera, PreviousCamera, Mean, Hit, Out or OutCount; History, HistoryHit and
 * HistoryCount not all NULL or all non-NULL; a misaligned plane (Mean, History, Out 16 bytes, Hit, HistoryHit 8,
 * HistoryCount, OutCount, Rgba8 4); Out equal to Mean or History, OutCount equal to HistoryCount (the pass gathers
 * from its neighbours: it does not run in place). */
int rt_reproject(const rt_reproject_desc *desc, void *stream);
/* Fills *out with Size, Width = Height = 0, Frames = 1, Flags = 0, every pointer NULL and the library's defaults:
 * MaxHistory = 8 (the built-in scenes are mirrors and glass: over a long orbit a longer history carries more stale
 * reflection than it removes noise) and DepthTolerance = 0.1f (within 0.001 of no depth test on the three scenes'
 * mean, and still a guard against the far side of a sphere).  Chosen on the CPU restatement over orbit steps of
 * 1/16 rad at 1 fresh spp on the three built-in scenes against 256-frame means (DESIGN.md has the tables).
 * RT_EINVAL for NULL. */
int rt_reproject_defaults(rt_reproject_desc *out);

/* ------------------------------------------------- ... with the history clamped to the fresh neighbourhood */

typedef struct rt_reproject_clip_desc {
    uint32_t Size;               /* sizeof(rt_reproject_clip_desc)                                    */
    uint32_t Radius;             /* 1..3: the window is (2*Radius+1)^2 pixels of Mean                 */
    float    Gamma;              /* finite, > 0: half-width of the band in standard deviations        */
    rt_reproject_desc Reproject; /* everything rt_reproject takes, Size included                      */
} rt_reproject_clip_desc;

/* rt_reproject with variance clipping, as temporal anti-aliasing uses it.  What a mirror or a glass sphere shows
 * does not follow its surface, so the history rt_reproject gathers there is a reflection seen from another place.
 * This call clamps the gathered history colour, per channel, to mean +- Gamma standard deviations of the FRESH
 * frame's pixels of the same sphere in a (2*Radius+1)^2 window around the pixel, and then folds as rt_reproject
 * does: a stale reflection falls outside the band and is pulled in, the history of a diffuse surface lies inside
 * it and is untouched.  It needs no knowledge of the material.  Everything rt_reproject's comment says of the call
 * (no rt_device, no state, one launch on `stream`, HOST cameras, inputs only read, not in place) holds; the call
 * reads no plane rt_reproject does not read.
 *
 * The result is rt_reproject's steps 1 to 8 on desc->Reproject with one step between "H.ch = acc.ch / ws" and the
 * fold of step 7, for a pixel that kept at least one tap; every operation is one IEEE f32 operation, as there
 * (tests/reproject_clip_ref.py restates it in numpy):
 *  7a Window, R = Radius: taps dy = -R..R (outer), dx = -R..R (inner), at q = (x + dx, y + dy) of the fresh planes
 *     Mean and Hit.  A tap is skipped when it is outside the image; when Hit[q].Key != kp (the whole word,
 *     RT_HIT_INSIDE included); when a channel of Mean[q].xyz is not finite.  The centre takes part under the same
 *     rules: only the finiteness rule can drop it.
 *  7b Sums: s1 = s2 = (+0, +0, +0), nf = +0.  A tap that is kept, c = Mean[q]: s1.ch = s1.ch + c.ch,
 *     s2.ch = s2.ch + c.ch * c.ch, nf = nf + 1.0f.
 *  7c Band, where nf > 0: m.ch = s1.ch / nf, v.ch = pos(s2.ch / nf - m.ch * m.ch) with rt_denoise's pos
 *     (x > 0 ? x : 0: a NaN gives 0), sd.ch = sqrtf(v.ch), lo.ch = m.ch - Gamma * sd.ch, hi.ch = m.ch + Gamma * sd.ch.
 *  7d Clamp, by comparisons: if (H.ch < lo.ch) H.ch = lo.ch; if (H.ch > hi.ch) H.ch = hi.ch; a NaN bound clamps
 *     nothing.  nf == 0: no clamp.  (Squares that overflow, channels beyond 1.8e19: where m.ch * m.ch is still
 *     finite, sd = inf and the band is (-inf, +inf); where it overflows too, v = pos(inf - inf) = 0 and the band is
 *     the point m.  With finite taps and a finite Gamma no bound is a NaN.)
 *  A pixel alone in its window (no neighbour of its sphere) has sd = 0, so its history becomes its fresh value:
 *  this is intended, one sample says nothing about what is plausible beside it.
 * OutCount, Out.w, the fresh cases, Rgba8 and RT_REPROJECT_SRGB_POW are exactly rt_reproject's; OutCount does not
 * depend on the clamp.  With Reproject.History == NULL the call writes what rt_reproject writes.
 *
 * RT_EINVAL, with an rt_last_error text and before anything is enqueued: a NULL desc or a wrong Size; Radius
 * outside 1..3; a Gamma that is NaN, infinite or not > 0; and everything rt_reproject refuses for Reproject, its
 * Size included, with rt_reproject's texts. */
int rt_reproject_clip(const rt_reproject_clip_desc *desc, void *stream);
/* Fills *out with Size, Reproject as rt_reproject_defaults fills it, and the library's defaults Radius = 1 and
 * Gamma = 0.5f: the lowest three-scene mean of moves 13..24 of a 24-move orbit after the default rt_denoise, over
 * Radius 1..3 x Gamma 0.5, 1, 2 on the CPU restatement, since the filtered frame is what a loop shows (DESIGN.md
 * has the tables, and where a scene is worse than under rt_reproject).  A caller that shows the carried frame
 * unfiltered does better with Radius = 2.  RT_EINVAL for NULL. */
int rt_reproject_clip_defaults(rt_reproject_clip_desc *out);

/* What the last rt_trace on `dev` launched.  Host-side bookkeeping, except
 * that TilesTraced and SegmentsFolded need the cull pass's totals: when the
 * last launch's key is new and they have not reached the host yet, this call
 * waits for them (the only blocking part).  The reference counts every bounce segment, misses
 * included (RaysCastInThread, main.cpp:390); segments of pixels whose every
 * sample provably misses (no primary ray of their tile can reach a sphere,
 * no sky term) are counted analytically and folded by a pixel kernel rather
 * than traced: SegmentsFolded of the launch's ray count are such segments. */
typedef struct rt_trace_info {
    uint64_t SegmentsFolded;  /* dead-tile segments counted, not traced      */
    uint32_t LanesPerPixel;   /* P of the launch (sample chains per pixel)   */
    uint32_t TilesTotal;      /* block tiles of the band geometry            */
    uint32_t TilesTraced;     /* live tiles launched on the trace kernel     */
    uint32_t CullPassRan;     /* 1: this launch ran the primary-ray cull pass */
    uint32_t OrderedLaunches; /* heaviest-first re-sorts done for this key   */
    uint32_t ClusteredWalk;   /* 1: secondary rays used the cluster walk     */
    uint32_t GroupsPerRuleSet;/* sphere groups of the rule set traced        */
    uint32_t SplitHeadFrames; /* > 0: a key's first launch ran as two trace
                                 launches, these frames first in the cull
                                 pass's order (measuring tile costs), the rest
                                 heaviest-first; the same bits as one launch  */
    uint32_t OneWaveGroups;   /* 1: one wave per workgroup (no LDS image)    */
    uint32_t Walk;            /* the host's routing of the secondary walk
                                 (one-wave launches; else 0): 0 run-time
                                 dispatch, 1 per-group loops, 2/3/4 cluster
                                 walk with 1/2/4 mask words, 5/6/7 the same
                                 with per-lane thresholds.  1-7 run a kernel
                                 compiled for that walk alone, which also
                                 takes launch facts at compile time; a launch
                                 without one of them is routed to 0, the
                                 run-time kernel, which tests them:
                                 MaxBounce >= 1 (MaxBounce == 0 -> 0), every
                                 r^2 in the short square root's range (a scene
                                 outside it -> 0), WalkAny off (on -> 0).
                                 Walk kernels exist for the launch shapes
                                 PixelsPerLane 4 and LanesPerPixel 4, 8, 16
                                 with the primary cull: at LanesPerPixel 1, 2
                                 or 32, or with Cull off, a routing of 1-7
                                 still runs the run-time kernel, which
                                 dispatches that same walk                    */
    uint32_t PixelsPerLane;   /* 4: each lane traced 4 pixels in turn (one-lane-
                                 per-pixel launches of one frame), else 1     */
    uint32_t PixelsSorted;    /* 1: the block tiles' pixels were dealt to their
                                 waves by the previous launch's costs (P >= 4;
                                 PixelSort off disables)                      */
    uint32_t BufferGrowths;   /* launch-buffer (re)allocations on this device
                                 so far (tile lists, cull masks): constant
                                 across launches that rt_device_reserve covers */
    uint32_t TilesSelected;   /* block tiles inside the tiles rt_trace_tiles listed
                                 (== TilesTotal after rt_trace).  TilesTotal stays
                                 the geometry's block tiles; TilesTraced counts the
                                 live tiles among the selected, SegmentsFolded the
                                 dead selected tiles' segments only             */
} rt_trace_info;
int rt_trace_last_info(rt_device *dev, rt_trace_info *out);
/* *out = 1 when the last launch on `dev` took per-tile counts (rt_trace_tile_work with mixed pairs, rt_trace_tile_counts),
 * 0 otherwise (rt_trace, rt_trace_tiles, a work list of one pair).  A query of its own: rt_trace_info keeps
 * the layout and the last field its callers know.  Host-side bookkeeping, never waits.  After such a
 * launch rt_trace_last_info's SegmentsFolded is summed on the device -- each dead block tile's in-image
 * pixels times its own tile's frames -- and that call waits for the sum as it does for the cull totals. */
int rt_trace_last_tile_counts(rt_device *dev, uint32_t *out);
/* *out = 1 when the last launch's kernel chose its member entries by the direction table
 * (rt_scene_direction_table; rt_trace_info.Walk is then 2 as for the cluster walk it replaces), else 0.
 * A query of its own, as rt_trace_last_tile_counts is.  Host-side bookkeeping, never waits. */
int rt_trace_last_direction_table(rt_device *dev, uint32_t *out);

/* Pre-sizes the device's launch buffers (tile order / cost / live lists, the
 * cull pass's masks and counters) for bands of up to `width` x `local_rows`
 * pixels under every lanes-per-pixel shape rt_trace may pick, so that no later
 * rt_trace of such a band allocates or waits for the device (growing a buffer
 * otherwise synchronises the launch's stream).  Successive calls keep the
 * largest tile and pixel counts over the geometries asked for (not the largest
 * width times the largest height).  Masks are sized for the current scene;
 * rt_scene_upload re-applies the reservation for a larger one (if that fails,
 * the upload still succeeds and the reservation is dropped: later launches
 * grow their buffers as they need).  Also sizes what rt_trace_tiles needs for
 * a width x local_rows image (the selection bitmap and its pinned staging) and
 * what rt_trace_tile_work needs beyond that (the per-tile table and its staging),
 * and rt_trace_first_hit's own bitmap and staging.
 * Waits for the device.  (New; the reference's arena is sized once in OnInit,
 * main.cpp:658.) */
int rt_device_reserve(rt_device *dev, uint32_t width, uint32_t local_rows);

/* ColorFromV4(LinearToSRGB(v)) (main.cpp:312-346, the store at :490) over a
 * device-resident running mean: n_pixels v4 f32 -> RGBA8, both DEVICE
 * pointers, enqueued on `stream` (NULL: the null stream).  flags: 0 or
 * RT_FLAG_SRGB_POW.  rt_trace already stores the RGBA8 of every frame it
 * folds; this re-encodes a gathered or saved accumulation without tracing. */
int rt_encode_rgba8(const float *d_accum_v4, uint32_t *d_rgba8, uint64_t n_pixels, uint32_t flags, void *stream);

/* Multi-GPU gather helper: scatters `band_count` compact band images
 * (device, `elem_bytes` per pixel; rank r's image starts at byte
 * r * rank_stride_bytes of `d_compact`, as an RCCL gather of padded
 * per-rank buffers lays them out) into the full image `d_dst` (device). */
int rt_assemble_bands(const void *d_compact, uint64_t rank_stride_bytes, void *d_dst, uint32_t width,
                      uint32_t height, uint32_t elem_bytes, uint32_t band_rows, uint32_t band_count,
                      void *stream);

int rt_device_synchronize(rt_device *dev);

/* ------------------------------------------- several GPUs, one host process */

/* Replaces the reference's thread-pool tiler (WorkQueueCreate/WorkQueueStart,
 * main.cpp:658-665, 851-856; wasm/wasm.cpp:651-678) with N GPUs driven from
 * one host thread: the frame is dealt in interleaved BandRows-row bands,
 * band b -> device b mod N, each device traces its bands on its
 * own stream, and the band images are gathered to devices[0] over xGMI --
 * RCCL grouped send/recv (ncclCommInitAll over the N devices) or, where RCCL
 * cannot be used (a device listed twice, no librccl), peer copies
 * (hipMemcpyPeerAsync) -- then scattered into the full frame.  Samples are
 * never split across devices (the running-mean fold is order dependent,
 * main.cpp:484-487), so the gathered frame is bit-identical to one device's. */
typedef struct rt_multi rt_multi;

#define RT_MULTI_AUTO 0u  /* RCCL when the devices are distinct and RCCL initialises, else peer copies */
#define RT_MULTI_RCCL 1u  /* RCCL only (rt_multi_create fails if it cannot be used) */
#define RT_MULTI_PEER 2u  /* peer copies only */
#define RT_MULTI_MAX_DEVICES 16u

int rt_multi_create(const int *hip_devices, uint32_t count, uint32_t transport, rt_multi **out);
/* rt_multi_create whose devices take `options` (rt_device_create_ex; NULL: the defaults). */
int rt_multi_create_ex(const int *hip_devices, uint32_t count, uint32_t transport, const rt_device_options *options,
                       rt_multi **out);
int rt_multi_destroy(rt_multi *m);
/* rt_set_rsqrt_table / rt_scene_upload on every device. */
int rt_multi_set_rsqrt_table(rt_multi *m, const float table[2048]);
int rt_multi_scene_upload(rt_multi *m, const rt_scene *scene);

/* rt_trace over the N devices.  The running mean stays resident on the
 * devices (each keeps its own bands'): desc->PreviousRayCount frames are
 * already folded there by earlier calls of the same geometry, or
 * RT_FLAG_ACCUM_ZERO (or PreviousRayCount 0) starts a new mean.
 *   cam->CurrentImage.Data : DEVICE pointer on devices[0], the full
 *                            Width x Height RGBA8 frame (written).
 *   cam->PreviousImage.Data: NULL, or a DEVICE pointer on devices[0] that
 *                            receives the full-frame v4 f32 running mean.
 *   desc->BandRows         : band height, a multiple of 8 (0 = 8);
 *                            desc->BandCount / BandIndex must be 0.
 *   d_rays                 : DEVICE u64 on devices[0], incremented by the
 *                            segments every device traced.
 * Everything the caller sees (frame, mean, d_rays) is written after prior
 * work on `stream` (a stream of devices[0]; NULL = the null stream), and work
 * enqueued on `stream` afterwards sees the gathered frame.  The traces read
 * nothing of the caller's and do not wait for that prior work: each device
 * alternates between two band-image slots, so call k's gather overlaps call
 * k+1's traces.  A continuation's PreviousRayCount must equal the count the
 * resident means were left at (RT_EINVAL otherwise): after a call with
 * PreviousRayCount P and Frames F that is P + F -- also for a restart with
 * RT_FLAG_ACCUM_ZERO and P > 0, whose frames were folded with the weights of
 * P, P + 1, ... (main.cpp:484-487), as rt_trace does.  A failed call drops
 * the resident means.  Every entry point that switches devices restores the
 * caller's current HIP device before it returns. */
int rt_multi_trace(rt_multi *m, const rt_camera_info *cam, const rt_trace_desc *desc, uint64_t *d_rays,
                   void *stream);
int rt_multi_synchronize(rt_multi *m);

typedef struct rt_multi_info {
    uint32_t DeviceCount;
    uint32_t Transport;      /* RT_MULTI_RCCL or RT_MULTI_PEER */
    uint32_t BandRows;       /* of the last trace */
    uint32_t MaxLocalRows;   /* rows of the largest device share */
    uint64_t SegmentsFolded; /* dead-tile segments counted, not traced (last trace, all devices;
                                may wait for each device's cull totals, as rt_trace_last_info) */
} rt_multi_info;
int rt_multi_get_info(rt_multi *m, rt_multi_info *out);

/* Each device's trace time (ms, HIP events around its rt_trace on its own
 * stream) of the last rt_multi_trace call, devices[i] -> ms_out[i]; count >=
 * the device count.  Waits for those traces to finish. */
int rt_multi_last_trace_ms(rt_multi *m, float *ms_out, uint32_t count);

/* The last call's gather time (ms, HIP events on devices[0]'s gather stream):
 * from the moment every device's trace has finished to the frame (and mean)
 * assembled -- the band transfer (RCCL or peer copies) plus the scatter. */
int rt_multi_last_gather_ms(rt_multi *m, float *ms_out);

/* rt_trace_last_info of devices[index] for the last call (RT_EINVAL when that
 * device traced nothing); may wait for its cull totals. */
int rt_multi_shard_info(rt_multi *m, uint32_t index, rt_trace_info *out);

/* Pre-sizes every device's band images and launch buffers (rt_device_reserve)
 * and devices[0]'s gather staging for frames up to width x height in
 * band_rows-row bands (0 = 8), so no rt_multi_trace of that geometry
 * allocates; RT_MULTI_RESERVE_MEAN also sizes the staging of the gathered
 * running mean (cam->PreviousImage).  Waits for the devices.  A reservation
 * that grows the devices' resident running means discards them: the next
 * call must restart the mean (PreviousRayCount 0 or RT_FLAG_ACCUM_ZERO), a
 * continuation is RT_EINVAL. */
#define RT_MULTI_RESERVE_MEAN 1u
int rt_multi_reserve(rt_multi *m, uint32_t width, uint32_t height, uint32_t band_rows, uint32_t flags);

/* Frames folded into the devices' resident running means, i.e. the
 * PreviousRayCount a continuation must name; 0 when no mean is resident
 * (none traced yet, a failed call, a geometry change, or a reservation that
 * grew the means). */
int rt_multi_resident_frames(rt_multi *m, uint64_t *out);

/* ----------------------------------- several GPUs, one process per GPU (RCCL) */

/* The band gather for one-process-per-GPU launches (torch.distributed.run /
 * mpirun): every rank traces its band residue with rt_trace (BandCount =
 * nranks, BandIndex = rank) and rt_comm_gather_bands brings the compact band
 * images to rank 0 over RCCL and scatters them into the full frame.  Rank 0
 * makes the id (rt_comm_unique_id) and the launcher shares its
 * RT_COMM_ID_BYTES bytes with every rank before rt_comm_create (which blocks
 * until all ranks have joined).  RT_ENODEV when librccl cannot be loaded or
 * RCCL refuses the communicator (e.g. two ranks on one GPU). */
typedef struct rt_comm rt_comm;
#define RT_COMM_ID_BYTES 128u
int rt_comm_unique_id(void *id_out);
int rt_comm_create(int hip_device, const void *id, uint32_t nranks, uint32_t rank, rt_comm **out);
int rt_comm_destroy(rt_comm *c);
/* d_local: this rank's compact band image (rt_band_local_rows(height,
 * band_rows, nranks, rank) x width x elem_bytes, device); d_full: rank 0's
 * full frame (width x height x elem_bytes, device; ignored elsewhere).
 * Enqueued on `stream` (NULL = the null stream) on every rank. */
int rt_comm_gather_bands(rt_comm *c, const void *d_local, void *d_full, uint32_t width, uint32_t height,
                         uint32_t elem_bytes, uint32_t band_rows, void *stream);

/* Scheduling counters accumulated over trace launches when the library is the
 * diagnostic build (`make -C simd-ray-tracer_amd variant NAME=stats
 * KFLAGS=-DRTK_STATS`, loaded via RT_TRACE_LIB) and the process runs with
 * RT_STATS=1: [0] primary wave-iterations, [1] primary lane-segments,
 * [2] secondary wave-iterations, [3] secondary lane-segments, [4] sphere
 * groups tested by primary iterations after culling, [5] secondary groups
 * (exact loop) where some lane passed the distance test, [6]/[7] secondary
 * iterations with < 16 lanes and their lanes, [8] secondary iterations with
 * no sample left to start, [9]-[15] wave-resident s_memtime cycles in
 * primary iterations, secondary iterations, the owner fold, block init,
 * mask load, barrier, and post-barrier setup, [16] prefiltered secondary
 * wave-iterations, [17]/[18] (wave, group) pairs the prefilter flagged, with
 * and without flags on the sphere a diffuse ray just left, [19]/[20] the same
 * per sphere pair, [21] lane-level flagged pairs (clustered loop: [17] member
 * pairs tested, [19] pairs rechecked, [21] clusters entered); [22]-[24] lanes of
 * primary rounds blocked by the sample ring, waiting for a secondary round,
 * and done; [25, 32) reserved.
 * Returns 1 when enabled, 0 when not (out zeroed), < 0 on error. */
int rt_debug_stats(rt_device *dev, uint64_t out[32], int reset);

/* With RT_WAVETIMES=1: {start, end} s_memrealtime (100 MHz) of every wave of
 * the last trace launch, wave id = block tile * 4 + w (dead tiles are not written).
 * Returns the number of waves copied (0 when disabled), < 0 on error. */
int64_t rt_debug_wave_times(rt_device *dev, uint64_t *out, uint64_t max_waves);

/* The cull pass's primary masks of the last culled launch geometry, one bit
 * per sphere pair (bit p: spheres 2p and 2p + 1, i.e. half p & 1 of group
 * p >> 1): word ((tile * 4 + wave) * n_words + w), n_words = ceil(2 groups / 64).
 * Returns the number of words copied (0 when no cull pass ran), < 0 on error.
 * After rt_trace_tiles the words of block tiles outside the listed tiles are
 * unspecified (the cull pass leaves such a tile before it writes any).
 * Test hook: tests/test_gpu_parity.py checks them against a CPU restatement. */
int64_t rt_debug_masks(rt_device *dev, uint64_t *out, uint64_t max_words);

/* Host-side view of what rt_scene_upload derives for one rule set (no GPU
 * needed): per sphere slot s = 4*group + lane, the r^2 the exact test uses
 * and the secondary-ray prefilter threshold r2p (any ray whose
 * origin lies on a scene sphere and |D|^2 is within 2^-16 of 1 that passes
 * the exact test d < r^2 (d <= r^2 for the scalar rules) has prefilter
 * estimate e < r2p).  *out_flags: bit 0 = the scene-wide threshold pays
 * for this scene, bit 1 = candidate sqrt in the short sequence's range, bit 2
 * = per-lane thresholds instead (where bit 0 is clear): r2p then holds r^2
 * (-inf: never hit) and a lane skips a sphere when e >= RN(cc 2^-15 + r2p),
 * cc its computed |C|^2.
 * Arrays may be NULL to query the count. */
int rt_scene_prefilter(const rt_scene *scene, uint32_t enable_simd, float *out_r2, float *out_r2p, uint32_t capacity,
                       uint32_t *out_count, uint32_t *out_flags);
/* The own-sphere rule's per-slot word (test/inspection hook; DESIGN.md §3, "the sphere a ray
 * leaves"): out_rho[s] is word 3 of sphere s's record, r_s^2 where a lane may prove that the ray it
 * continues from sphere s cannot accept s again, +inf where nothing is proven (no scene-wide
 * cluster table, a sphere outside it, a radius outside [16.1 eps, 16]).  A lane with C = RN(S - O),
 * cc = fma |C|^2 and T = fma C.D leaves s out of its own member flags when
 * |RN(rho - cc (1 - 5 2^-18))| < RN(-T 1.9e-4).  out_rho may be NULL to query the count. */
int rt_scene_own_sphere(const rt_scene *scene, uint32_t enable_simd, float *out_rho, uint32_t capacity,
                        uint32_t *out_count);
/* The packed sphere-group records rt_scene_upload builds for one rule set, as
 * the device reads them (layout: rt_kernel.h, "HBM layout of an uploaded
 * scene").  *out_f4 = float4 rows; out_rows (optional, 6 words) = rows per
 * group, then the row index of x, y, z, r*r and the prefilter threshold.  out
 * may be NULL to query the size.  Test/inspection hook. */
int rt_scene_groups(const rt_scene *scene, uint32_t enable_simd, float *out, uint32_t capacity_f4, uint32_t *out_f4,
                    uint32_t *out_rows);
/* The clustered secondary-ray prefilter table rt_scene_upload builds for one
 * rule set (layout: rt_kernel.h, kClEntryF4 = 4 float4 rows per entry;
 * cluster-pair entries first).  *out_f4 = float4 rows, *out_cpairs = cluster
 * pairs (0: the scene uses the per-group prefilter loop).  out may be NULL to
 * query the size.  Test/inspection hook: the kernel's skip proof is checked
 * against it on the CPU (tests/test_prefilter_bound.py). */
int rt_scene_clusters(const rt_scene *scene, uint32_t enable_simd, float *out, uint32_t capacity_f4,
                      uint32_t *out_f4, uint32_t *out_cpairs);
/* The expanded form of a scene-wide table (test/inspection hook; DESIGN.md §3, "the expanded
 * prefilter"): the same entries in the same layout, with centres S' = RN(S - c0), near-line
 * thresholds t' = t - |S'|^2 + G and behind thresholds lowered by the error of the expanded T; mask
 * rows, ranges and slots are those of rt_scene_clusters.  A lane with O' = RN(O - c0) skips on
 *   fma(-T, T, A) >= t',  T = fma(S'x, Dx, fma(S'y, Dy, fma(S'z, Dz, -O'.D))),
 *                         A = fma(S'x, -2O'x, fma(S'y, -2O'y, fma(S'z, -2O'z, |O'|^2))),
 * and on T < b'.  *out_f4 = float4 rows (0: the scene has no scene-wide table), out_c0 = c0 (3 floats),
 * *out_in_use = 1 where the table is proven and useful for the scene, so that the walk-specialised
 * kernels run on it; 0: every launch walks the rt_scene_clusters table with the run-time kernel
 * (rt_trace_info.Walk = 0).  out may be NULL to query the size. */
int rt_scene_clusters_expanded(const rt_scene *scene, uint32_t enable_simd, float *out, uint32_t capacity_f4,
                               uint32_t *out_f4, float *out_c0, uint32_t *out_in_use);
/* The table's levels (test/inspection hook): *out_levels = 1 (cluster-pair
 * entries index member entries), 2 (tables of two or more pair-mask words: the
 * *out_cpairs top entries index *out_sub_pairs sub-cluster pair entries, which
 * index the member entries) or 0 (no table). */
int rt_scene_cluster_layout(const rt_scene *scene, uint32_t enable_simd, uint32_t *out_levels,
                            uint32_t *out_sub_pairs);
/* The direction table of a one-word scene-wide table whose expanded form is in use (test/inspection hook;
 * DESIGN.md §3, "the direction table"): Rows rows, one per sphere slot, of CellsPerRow masks of MaskBits
 * bits (32 up to 32 sphere pairs, else 64), row-major.  Bit p of row j, cell c is set when a ray with
 * |D|^2 within 2^-16 of 1 and rt_direction_cell(D) == c whose origin lies within 1.008 r_j of sphere j's
 * centre can be accepted by the exact test on sphere 2p or 2p + 1; the bit of j's own pair is always
 * set, and a cell no such direction reaches is all-ones.  A secondary round of the walk-specialised
 * one-wave kernels then tests only the member entries of the union of its lanes' masks.  *out_bytes = the
 * table's size (0: the scene has none; info is then all 0); out may be NULL to query the size. */
typedef struct rt_direction_table_info {
    uint32_t CellsPerEdge; /* n: a face of the direction grid is n x n cells        */
    uint32_t MaskBits;     /* 32 or 64                                              */
    uint32_t Rows;         /* sphere slots: 4 x groups                              */
    uint32_t CellsPerRow;  /* 6 n^2                                                 */
} rt_direction_table_info;
int rt_scene_direction_table(const rt_scene *scene, uint32_t enable_simd, void *out, uint64_t capacity_bytes,
                             uint64_t *out_bytes, rt_direction_table_info *info);
/* The member entries that walk reads: entry p = the sphere pair {2p, 2p + 1} in the layout and with the
 * values of the rt_scene_clusters_expanded member entries (4 float4 rows each; a sphere outside the
 * table: threshold -inf, no bit).  *out_f4 = float4 rows (0: none). */
int rt_scene_direction_members(const rt_scene *scene, uint32_t enable_simd, float *out, uint32_t capacity_f4,
                               uint32_t *out_f4);
/* The cell of direction D, bit for bit the kernel's own function (IEEE compares, one FMA, floor and clamp
 * per axis): face = the largest component by magnitude and its sign, the other two components index the
 * face's n x n grid as they are. */
uint32_t rt_direction_cell(float dx, float dy, float dz);
/* The union step of that walk, alone (test/inspection hook): one wave of 64 lanes runs the kernels' own union
 * function with only the lanes of `lanes` enabled (bit l = lane l; 0 is refused: a round has at least one
 * lane) and returns the OR of their words.  words: one mask per lane, 64 uint32 for mask_bits = 32, or 64
 * pairs {low, high} for mask_bits = 64; out_union = {low, high} (high = 0 at 32 bits).  The union enables
 * every lane while it reduces, so each lane, enabled or not, also writes canary_in[l] to a register of its
 * own before the union and stores it to canary_out[l] after it: canary_out == canary_in shows that the
 * reduction wrote no register that belongs to a lane outside `lanes`. */
int rt_direction_union(rt_device *dev, const uint32_t *words, uint32_t mask_bits, uint64_t lanes,
                       const uint32_t *canary_in, uint32_t out_union[2], uint32_t *canary_out);
const char *rt_last_error(void);

/* ----------------------------------------------- OnInit / OnRender driver */

/* OnInit (main.cpp:645-679): window defaults, built-in scenes, device 0. */
int rt_on_init(rt_init_params *params);
/* OnInit on `count` devices: with more than one, rt_on_render drives them
 * through rt_multi (bands dealt over the devices, the running mean resident
 * on each, the frame gathered to hip_devices[0]). */
int rt_on_init_devices(rt_init_params *params, const int *hip_devices, uint32_t count);

/* Input state for the orbit camera (the reference polls IsDown(key) at
 * main.cpp:732-761).  Bits: */
#define RT_KEY_FORWARD 0x01u  /* W / ArrowUp    */
#define RT_KEY_BACK 0x02u     /* S / ArrowDown  */
#define RT_KEY_RIGHT 0x04u    /* D / ArrowRight */
#define RT_KEY_LEFT 0x08u     /* A / ArrowLeft  */
#define RT_KEY_UP 0x10u       /* Space          */
#define RT_KEY_DOWN 0x20u     /* C / LeftControl*/
#define RT_KEY_RESET 0x40u    /* R              */

/* OnRender (main.cpp:705-859) with the accumulation resident in HBM: one
 * progressive frame per call, one-frame output lag, reset on
 * move/resize/scene change/R.  `image` is a HOST RGBA8 image.  Returns 1
 * when `image` received a completed frame, 0 when not (previous frame
 * still running), negative on error. */
int rt_on_render(const rt_image *image, rt_render_params params, uint32_t keys,
                 uint64_t *out_total_rays_cast, double *out_time_elapsed_ms);

/* Blocks until the in-flight frame (if any) has completed
 * (WorkQueueWaitUntilCompletion, base.h:175). */
int rt_on_render_wait(void);
int rt_on_shutdown(void);

/* Opt-in fast hand-out.  By default rt_on_render copies a completed frame
 * into `image` through a pinned staging buffer the library owns (one DMA,
 * then one host copy; the reference's CopyImage, main.cpp:688-697).  A caller
 * that renders into the same host buffer every frame (the platform's image,
 * wasm/wasm.cpp:179) may register it: the library page-locks the `bytes` at
 * `data`, and frames for an image whose Data is `data` then arrive by one DMA
 * straight into it.  The caller must keep the buffer allocated until
 * rt_on_render_unregister_image or rt_on_shutdown, which unlock it.  A second
 * registration replaces the first.  Returns RT_OK, RT_EINVAL (not initialised,
 * NULL, 0 bytes) or RT_EIO (the driver refused to page-lock it). */
int rt_on_render_register_image(void *data, uint64_t bytes);
int rt_on_render_unregister_image(void);

/* Where rt_on_render's time goes (cumulative since init or the last reset).
 * A frame is handed out by rt_on_render after the next frame is launched, so
 * the copy runs beside that frame's trace. */
typedef struct rt_on_render_profile {
    uint64_t Calls;          /* rt_on_render calls                                   */
    uint64_t FramesLaunched; /* frames started (trace + its copies to the host)      */
    uint64_t FramesCopied;   /* completed frames handed to the caller's image        */
    double CallMs;           /* host time inside rt_on_render                         */
    double HostCopyMs;       /* of which: frame -> caller image (CopyImage: DMA [+ host copy]) */
    double HostWaitMs;       /* of which: waiting for an in-flight frame (reset/move) */
    double GpuFrameMs;       /* sum of completed frames' launch -> done GPU time      */
    uint64_t FrameAllocations; /* frame-buffer (re)allocations by rt_on_init /
                                  rt_on_render_reserve / a resize beyond them      */
} rt_on_render_profile;
int rt_on_render_get_profile(rt_on_render_profile *out, int reset);

/* Sizes the frame driver's device frames (running mean + two RGBA8 frames)
 * and the trace's launch buffers for images up to width x height, so a later
 * resize within that size frees and allocates nothing: it re-uses them, as
 * the reference re-Pushes its images into the arena OnInit sized (main.cpp:
 * 658, 798-804).  rt_on_init reserves its 1280x720 window (main.cpp:649-650).
 * Keeps the current frames on one device; on several devices (rt_on_init_devices)
 * the call restarts the running mean at the next rt_on_render, as a resize does,
 * since growing the devices' resident means drops them.  New. */
int rt_on_render_reserve(uint32_t width, uint32_t height);

/* ----------------------------------------------------------- output path */

/* The RGBA8 frame (RT_FORMAT_R8G8B8A8_U32, host memory) written as a binary
 * PPM (P6, RGB) or an 8-bit RGBA PNG (stored deflate blocks), in place of
 * the reference's WebGL texture upload of Image.Data (wasm/wasm.cpp:216-218).
 * RT_IMAGE_FLIP_Y writes image row Height-1 first: the texture's row 0 is the
 * bottom of the window, so that is the on-screen orientation.
 * Returns RT_OK, RT_EINVAL (bad image / format / path) or RT_EIO. */
#define RT_IMAGE_FLIP_Y 1u
int rt_image_write_ppm(const rt_image *image, const char *path, uint32_t flags);
int rt_image_write_png(const rt_image *image, const char *path, uint32_t flags);

/* FNV-1a 64 of `nbytes` host bytes (offset basis 0xcbf29ce484222325, prime
 * 0x100000001b3): the frame checksum the committed fixtures hold
 * (tests/golden, *.json), so a caller can check a rendered frame -- RGBA8 or
 * the v4 running mean copied to the host -- against a golden without the
 * checker.  New; the reference has no frame checksum. */
uint64_t rt_frame_hash(const void *data, uint64_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* RT_TRACE_H */
