/*
 * horayzon_hip.h -- C ABI of libhorayzon_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the ray-casting core of HORAYZON.  Each entry point
 * names the reference interface it replaces (paths relative to the reference
 * tree).  The reference exposes C++-linkage functions to Cython
 * (horizon.pyx:13-27, shadow.pyx:8-15); a maintainer binds these C symbols
 * instead (see INTEGRATION.md for the Cython / ctypes stubs).
 *
 * Conventions
 *   - plain pointers and sizes only; every array is caller-owned and is never
 *     retained after the call returns (the reference keeps raw pointers in
 *     CppTerrain, shadow_comp.cpp:332-346; this library copies to HBM).
 *   - every data pointer may be HOST memory (NumPy) or DEVICE memory (HBM) of
 *     the selected GPU; the library detects which (hipPointerGetAttributes).
 *   - every function returns 0 on success and a non-zero status otherwise;
 *     hz_last_error() returns the message (thread local).  The reference
 *     returns void and only prints (horizon_comp.cpp:74-76).
 *   - units and meaning of the scalar arguments are exactly the reference's
 *     (degrees, kilometres, ... as in horizon_comp.h:8-20, shadow_comp.h:22-38).
 */
#ifndef HORAYZON_HIP_H
#define HORAYZON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HZ_OK 0
#define HZ_ERR_ARG 1      /* invalid argument                                  */
#define HZ_ERR_HIP 2      /* HIP runtime failure (message has the HIP error)   */
#define HZ_ERR_NODEV 3    /* no usable gfx950 device                           */
#define HZ_ERR_DEPTH 4    /* BVH deeper than the traversal stack               */
#define HZ_ERR_BOUND 5    /* a bounded device loop reached its iteration limit */

/* Optional controls; pass NULL for the reference's behaviour on device 0.     */
typedef struct hz_opts {
    int32_t device;        /* HIP device ordinal                               */
    int32_t verbose;       /* 1: print the reference's stdout report           */
    int32_t row_begin;     /* inner-domain row slab [row_begin, row_end) to compute.  {0, 0} (a zeroed struct) = the   */
    int32_t row_end;       /*   whole inner domain; row_end == -1 = dim_in_0 (explicit sentinel); every other pair    */
                           /*   must satisfy 0 <= row_begin <= row_end <= dim_in_0, else HZ_ERR_ARG (negative or        */
                           /*   out-of-range slabs are rejected, not clamped).  row_begin == row_end (> 0) is an empty  */
                           /*   slab: the call succeeds and computes nothing (a rank without rows)                      */
    int32_t top_nodes;     /* > 0: stage that many top-of-tree BVH nodes in LDS (guess_constant;   */
                           /*   measured 2 % slower than L1 reads, so <= 0 means none)            */
    int32_t regroup;       /* wave regroup threshold in lanes (<= 0: default)  */
                           /*   | leaf-vote bias << 8 | 0x10000: the threshold  */
                           /*   is absolute ("regroup_rule" of hz_debug_set)    */
    int32_t count_work;    /* 1: also count BVH nodes / triangle tests (slow)  */
    int32_t no_hit_cache;  /* 0 (default): rays expected to be blocked first walk the subtree  */
                           /*   that blocked the cell's previous ray; 1: always start at the root */
    float  *svf;           /* optional fused sky view factor out, f32[y][x]    */
    const float *vec_tilt; /* tilted normals f32[y][x][3] for svf              */
    int32_t skip_hori;     /* 1: hori_buffer may be NULL, only svf (and the    */
                           /*   maps of hz_topo_out, _ex calls) are written    */
    int32_t chunk_rows;    /* rows per launch when hori is host memory or skipped (chunks are      */
                           /*   double buffered and copied out while the next one is traced);      */
                           /*   <= 0: as many rows as fit 4 GiB                                     */
    int32_t level_stack;   /* 1: use the one-entry-per-tree-level traversal stack from the start (cannot overflow, +10 % */
                           /*   VALU); 0: the fast discipline first, the other one only for launches whose stack overflowed; */
                           /*   < 0 (tests): the fast discipline with -level_stack entries                                 */
    int32_t hori_is_slab;  /* 0: hori_buffer (and svf) address inner-domain row 0 (reference layout, [dim_in_0][..]); */
                           /*   1: they address row_begin, i.e. hold only the slab [row_end - row_begin][dim_in_1].. */
                           /*   -- the form for resident HBM slab buffers (the caller never forms an address        */
                           /*   outside its allocation).  For the inputs see inputs_are_slab                         */
    int32_t no_near_skip;  /* 1: do not compute / use the near-field certificates (hz_near.hip): every ray starts at   */
                           /*   parameter 0.  Results are the same either way; the default (0) is faster and is only   */
                           /*   active for a DEM mesh that IS a height field over the world (x, y) plane (checked by   */
                           /*   the scene build, hz_stats.height_field); -1 (tests): certificates even if it is not    */
    int32_t verify_near;   /* N >= 1: check the near-field certificates while computing; disagreeing hit decisions are   */
                           /*   counted in hz_stats.near_violations (must stay 0), the rays checked in near_verified.    */
                           /*   With count_work: the counting instantiation traces one of every N shortened rays (N       */
                           /*   rounded up to a power of two; 1: every one) a second time over its full length.  Without: */
                           /*   the production launch is untouched and a second, counting launch re-traces EVERY          */
                           /*   shortened ray of one of every N 8 x 8 blocks of cells, next to it on a stream of its own --  */
                           /*   N = 256 monitors real inputs for 2 - 3 % of the run time (profiles/r04/)                  */
    int32_t inputs_are_slab; /* 0: vec_norm, vec_north, mask (and opts.vec_tilt) address inner-domain row 0 (reference   */
                           /*   layout; only the slab's rows are read or uploaded); 1: they address row_begin, i.e. the */
                           /*   caller holds only its slab [row_end - row_begin][dim_in_1] of each -- the form for a    */
                           /*   rank of a row-sharded job                                                                */
    int32_t no_host_pin;   /* 0 (default): a HOST hori_buffer is page-locked chunk by chunk on a helper thread while the   */
                           /*   first chunks are traced (hipHostRegister, released before the call returns), so that the  */
                           /*   device-to-host copies are DMA instead of staged pageable copies; 1: leave it pageable     */
    int32_t left_min;      /* leftover cells (hz_horizon.hip): an 8 x 8 block of cells ends when at most this many of its  */
                           /*   cells are unfinished; they are finished 64 at a time by follow-up launches, which hand     */
                           /*   over again.  Byte l = the threshold of level l (0 = production launch; a zero byte: that   */
                           /*   level runs to its end); 0: the default; < 0: off.  Results do not depend on it             */
    int32_t persist_grid;  /* 0 (default): persistent waves -- a launch has as many workgroups as are resident at once and */
                           /*   every wave pulls 8 x 8 blocks from its XCD's queue; < 0: one 16 x 16 tile per workgroup;   */
                           /*   n > 0 (tests): persistent with n workgroups, so that small grids run the block loop too    */
    int32_t left_cap_test; /* tests: > 0 caps every region of the leftover records at this many (rounded up to 64), so       */
                           /*   that the out-of-room path runs on small grids                                               */
    int32_t left_tune;     /* tuning of the follow-up launches (0: defaults): byte 0 = their compaction threshold in lanes   */
                           /*   (opts.regroup of those launches), byte 1 = 1 + log2 of the width of the azimuths-left        */
                           /*   classes their cells are sorted into (1: one class per azimuth)                               */
} hz_opts;

/* Run-time self report (the quantities the reference prints,                  */
/* horizon_comp.cpp:225-227, 805-810, 816-818).                                */
typedef struct hz_stats {
    uint64_t num_rays;     /* occlusion queries, counted as the reference does */
    uint64_t num_cells;    /* cells with mask == 1 in the computed slab        */
    uint64_t guard_events; /* searches stopped where the reference never ends  */
    uint64_t nodes_visited;/* only with count_work                             */
    uint64_t tris_tested;  /* only with count_work                             */
    double t_bvh_s;        /* "BVH build time"                                 */
    double t_h2d_s;        /* host -> HBM copies                               */
    double t_kernel_s;     /* "Ray tracing time" (traversal kernels only)      */
    double t_d2h_s;        /* HBM -> host copies                               */
    double t_total_s;      /* "Total run time"                                 */
    int32_t bvh_height;
    int32_t elev_num;
    uint64_t scene_bytes;  /* HBM bytes of vertices + LBVH                     */
    uint64_t wave_node_iters; /* count_work: wave-level executions of the node  */
    uint64_t wave_leaf_iters; /*   step / leaf step / ray refill section (SIMT  */
    uint64_t wave_refills;    /*   efficiency = lane count / (64 x wave count)) */
    double t_svf_s;        /* the horizon reductions: the kernel that writes opts.svf and / or the  */
                           /*   hz_topo_out maps of the _ex calls (one launch per horizon chunk)      */
    uint64_t stack_fallbacks; /* launches after which blocks (or the whole launch) were repeated with the one-entry-per- */
                              /*   level stack because a ray ran out of entries of the fast one                          */
    uint64_t rays_shortened;  /* count_work: rays that started beyond the cell's neighbourhood (near-field certificate) */
    uint64_t near_violations; /* count_work + verify_near: shortened rays whose full-length re-trace disagreed (0)      */
    double t_near_s;       /* certificate pre-pass (hz_near.hip)                */
    uint64_t stack_redo_blocks; /* 8 x 8 blocks repeated one by one after such an overflow (few: deep trees overflow in    */
                               /*   a few places; many overflows repeat the launch and switch the scene for good)        */
    uint64_t guard_cells;  /* cells with at least one guard event (the reference's search would not terminate there,     */
                           /*   horizon_comp.cpp:474-488)                                                                 */
    int32_t height_field;  /* 1: the scene's DEM mesh is a height field over the world (x, y) plane                      */
    int32_t near_used;     /* 1: the near-field certificates were active in this call                                    */
    uint64_t near_verified;/* opts.verify_near: shortened rays that were traced a second time over their full length     */
    double t_left_s;       /* leftover launches: part of t_kernel_s spent finishing the cells that blocks of the production   */
    uint64_t left_cells;   /*   launch handed over when <= opts.left_min of their 64 cells were unfinished (hz_horizon.hip)   */
    uint64_t left_again;   /* hand-overs by the leftover launches themselves (levels >= 1)                                    */
    uint64_t scratch_bytes;/* HBM scratch this call used besides the scene and the caller's buffers: near-field certificates, */
                           /*   leftover records, the horizon chunk buffers of a host / skipped hori_buffer                   */
    uint64_t left_redo_groups; /* groups of 64 leftover cells computed again with the one-entry-per-level stack after a ray of */
                           /*   theirs ran out of entries of the fast one (counted in stack_redo_blocks as well)               */
} hz_stats;

const char *hz_last_error(void);
/* sizeof(hz_opts), sizeof(hz_stats) as compiled: lets a binding verify its mirror */
int hz_abi_struct_sizes(int *opts_bytes, int *stats_bytes);
/* ABI revision.  6 (round 6): opts.left_min, persist_grid, left_cap_test, left_tune and hz_stats.left_again, scratch_bytes, left_redo_groups appended.  5 (round 5): hz_stats.t_left_s, left_cells appended.  4 (round 4): hz_stats.near_verified appended; opts.verify_near is a sampling period (1 = every ray, as   */
/* before).  3 (round 3): {row_begin > 0, row_end = 0} is rejected (was "to the end": use row_end = -1); opts.regroup <= 0 */
/* means the default threshold (was: 0 = ray compaction off; 64 | bias << 8 still disables the early exit in effect)     */
int hz_abi_version(void);
int hz_device_count(int *count);
/* name[0..cap) <- device name, *cu <- compute units, *hbm_bytes <- total HBM  */
int hz_device_info(int device, char *name, int cap, int *cu, uint64_t *hbm_bytes);

/* ------------------------------------------------------------------------- */
/* Scene = vertices + flat LBVH, resident in HBM as ONE contiguous blob        */
/* (so that a multi-GPU job can broadcast it with a single collective).        */
/* Replaces initializeDevice/initializeScene, horizon_comp.cpp:74-231,         */
/* shadow_comp.cpp:171-298 (Embree rtcNewScene ... rtcCommitScene).            */
/* ------------------------------------------------------------------------- */
typedef struct hz_scene hz_scene;

int hz_scene_create(const float *vert_grid, int dem_dim_0, int dem_dim_1,
                    const char *geom_type,
                    const float *vert_simp, int num_vert_simp,
                    const int32_t *tri_ind_simp, int num_tri_simp,
                    int device, hz_scene **scene, hz_stats *stats);
/* the blob: position independent, valid on any gfx950 device                  */
int hz_scene_blob(const hz_scene *scene, void **device_ptr, size_t *nbytes);
/* the vertex array inside the blob (f32[dem_dim_0 * dem_dim_1][3], the caller's vert_grid without padding): lets a   */
/* rank that received the blob derive per-cell inputs of its slab on the device without the host arrays               */
int hz_scene_vertices(const hz_scene *scene, const float **device_ptr, int *dem_dim_0, int *dem_dim_1,
                      int *height_field);
/* wrap a blob that already sits in HBM of `device` (e.g. received by an RCCL  */
/* broadcast into caller-owned memory); the scene does not own the memory      */
int hz_scene_adopt(void *device_ptr, size_t nbytes, int device, hz_scene **scene);
int hz_scene_destroy(hz_scene *scene);

/* ------------------------------------------------------------------------- */
/* Horizon                                                                     */
/* ------------------------------------------------------------------------- */

/* One-shot call; argument list mirrors horizon_gridded_comp                   */
/* (horizon_comp.h:8-20, horizon_comp.cpp:629-822).  Builds the scene,         */
/* computes, releases (the reference also rebuilds per call, :813-814).        */
int hz_horizon_gridded(const float *vert_grid, int dem_dim_0, int dem_dim_1,
                       const float *vec_norm, const float *vec_north,
                       int offset_0, int offset_1,
                       float *hori_buffer, int dim_in_0, int dim_in_1,
                       int azim_num, float dist_search, float hori_acc,
                       const char *ray_algorithm, const char *geom_type,
                       const float *vert_simp, int num_vert_simp,
                       const int32_t *tri_ind_simp, int num_tri_simp,
                       float elev_ang_low_lim, const uint8_t *mask,
                       float hori_fill, float ray_org_elev,
                       const hz_opts *opts, hz_stats *stats);

/* Same computation on an existing scene (persistent BVH; additive API).       */
int hz_horizon_gridded_scene(const hz_scene *scene,
                             const float *vec_norm, const float *vec_north,
                             int offset_0, int offset_1,
                             float *hori_buffer, int dim_in_0, int dim_in_1,
                             int azim_num, float dist_search, float hori_acc,
                             const char *ray_algorithm,
                             float elev_ang_low_lim, const uint8_t *mask,
                             float hori_fill, float ray_org_elev,
                             const hz_opts *opts, hz_stats *stats);

/* Further reductions of the horizon computed in the same call (the _ex forms below).  Each map follows every   */
/* rule opts->svf follows: host or device memory; only the row slab is written (other rows are left untouched);  */
/* with opts->hori_is_slab it addresses row_begin; opts->vec_tilt (opts->inputs_are_slab) supplies the tilt.     */
/* Every horizon chunk gets ONE reduction launch that writes all requested maps, opts->svf included, and          */
/* opts->skip_hori is valid as soon as any of svf / vsf / openness is requested.                                 */
typedef struct hz_topo_out {
    int32_t size;          /* sizeof(hz_topo_out); other values -> HZ_ERR_ARG (room to grow without a new revision)  */
    float  *vsf;           /* optional visible sky fraction f32[y][x] (_visible_sky_fraction_cy, topo_param.pyx:499-543); */
                           /*   needs opts->vec_tilt and azim_num >= 2                                                */
    float  *openness;      /* optional positive topographic openness f32[y][x] [radian] (_topographic_openness_cy,   */
                           /*   :577-603); needs neither vec_tilt nor two azimuths                                     */
} hz_topo_out;

/* hz_horizon_gridded / hz_horizon_gridded_scene plus the maps of `topo`.  topo == NULL, or both of its pointers */
/* NULL: exactly the call without _ex.                                                                           */
int hz_horizon_gridded_ex(const float *vert_grid, int dem_dim_0, int dem_dim_1,
                          const float *vec_norm, const float *vec_north,
                          int offset_0, int offset_1,
                          float *hori_buffer, int dim_in_0, int dim_in_1,
                          int azim_num, float dist_search, float hori_acc,
                          const char *ray_algorithm, const char *geom_type,
                          const float *vert_simp, int num_vert_simp,
                          const int32_t *tri_ind_simp, int num_tri_simp,
                          float elev_ang_low_lim, const uint8_t *mask,
                          float hori_fill, float ray_org_elev,
                          const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats);
int hz_horizon_gridded_scene_ex(const hz_scene *scene,
                                const float *vec_norm, const float *vec_north,
                                int offset_0, int offset_1,
                                float *hori_buffer, int dim_in_0, int dim_in_1,
                                int azim_num, float dist_search, float hori_acc,
                                const char *ray_algorithm,
                                float elev_ang_low_lim, const uint8_t *mask,
                                float hori_fill, float ray_org_elev,
                                const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats);

/* ------------------------------------------------------------------------- */
/* The azimuth-major layout (additive): planes f32[azim_num][y][x] next to hori f32[y][x][azim_num].            */
/* planes[k][y][x] and hori[y][x][k] hold the same 32-bit word, NaN payloads and hori_fill included: the         */
/* functions below move words and decide nothing numerically, so every result obtained through planes is         */
/* bit-identical to the one obtained through the cell-major layout.  It is the layout a stored horizon is read   */
/* back in (hz_horizon_terrain_initialise_planes): a wave that looks one azimuth up reads consecutive words.    */
/* ------------------------------------------------------------------------- */
/* The _ex forms with `hori_planes` f32[azim_num][rows][dim_in_1] in place of hori_buffer (host or device        */
/* memory); the cell-major horizon is never written.  Each chunk of rows is traced into the bounded chunk buffer */
/* of opts->skip_hori, reduced as the _ex forms reduce it (topo, opts->svf), and transposed into its rows of     */
/* every plane; a host hori_planes receives it through a second chunk buffer and one strided copy.  Row slabs    */
/* mean what they mean for hori_buffer: rows = dim_in_0 and the planes address inner-domain row 0, or, with      */
/* opts->hori_is_slab, rows = row_end - row_begin and they address row_begin; rows outside the slab are left     */
/* untouched.  opts->skip_hori is HZ_ERR_ARG here.  stats->scratch_bytes includes the chunk buffers.             */
int hz_horizon_gridded_planes(const float *vert_grid, int dem_dim_0, int dem_dim_1,
                              const float *vec_norm, const float *vec_north,
                              int offset_0, int offset_1,
                              float *hori_planes, int dim_in_0, int dim_in_1,
                              int azim_num, float dist_search, float hori_acc,
                              const char *ray_algorithm, const char *geom_type,
                              const float *vert_simp, int num_vert_simp,
                              const int32_t *tri_ind_simp, int num_tri_simp,
                              float elev_ang_low_lim, const uint8_t *mask,
                              float hori_fill, float ray_org_elev,
                              const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats);
int hz_horizon_gridded_scene_planes(const hz_scene *scene,
                                    const float *vec_norm, const float *vec_north,
                                    int offset_0, int offset_1,
                                    float *hori_planes, int dim_in_0, int dim_in_1,
                                    int azim_num, float dist_search, float hori_acc,
                                    const char *ray_algorithm,
                                    float elev_ang_low_lim, const uint8_t *mask,
                                    float hori_fill, float ray_org_elev,
                                    const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats);
/* hori f32[len_0][len_1][len_2] <-> planes f32[len_2][len_0][len_1], a tiled transpose on the device.  Each     */
/* pointer may be host or device memory; a host side is staged in chunks of at most 256 MiB, never as a second   */
/* full copy on the device.  All lengths >= 1.                                                                   */
int hz_hori_to_planes(const float *hori, int len_0, int len_1, int len_2, float *planes, int device);
int hz_hori_from_planes(const float *planes, int len_0, int len_1, int len_2, float *hori, int device);
/* hz_topo_params with the horizon given as planes f32[len_2][len_0][len_1] (host or device): chunk by chunk    */
/* the rows go back into a bounded cell-major buffer and through the reduction launch of hz_topo_params, so each */
/* map is bit-identical to hz_topo_params' (and to the single-output functions').                               */
int hz_topo_params_planes(const float *azim, const float *planes, const float *vec_tilt, int len_0, int len_1, int len_2,
                          float *svf, float *vsf, float *openness, int device);

/* ------------------------------------------------------------------------- */
/* The 16-bit horizon code (additive; DESIGN.md section 4, clause 15): half the bytes of the float32 horizon.     */
/* All arithmetic is float64, every operation rounded on its own, rint rounds half to even:                      */
/*   HALF_PI = 1.5707963267948966, SCALE = 32767.0 / HALF_PI, STEP = HALF_PI / 32767.0                           */
/*   encode(v): NaN -> 0xFFFF; else (uint16)(rint(fmin(fmax((double)v, -HALF_PI), HALF_PI) * SCALE) + 32767.0)    */
/*   decode(q): 0xFFFF -> the quiet NaN 0x7FC00000; else (float)((double)((int)q - 32767) * STEP)                */
/* +-0 encodes to 32767 and decodes to +0.0f; +-inf and finite values outside [-pi/2, pi/2] (a hori_fill, say)    */
/* clamp to the ends; encode(decode(q)) == q for every q; |decode(encode(v)) - v| <= STEP / 2 + 2^-24 rad in      */
/* range.  The code is elementwise: planes_q[k][y][x] and hori_q[y][x][k] hold the same 16-bit word.              */
/* ------------------------------------------------------------------------- */
/* dst[i] = encode(src[i]) / decode(src[i]), i < n.  Either side may be host or device memory, in any mix, aligned */
/* to its element type (a view at an odd element is fine); a host side is staged in bounded chunks                */
/* ("q16_chunk" elements).  n == 0 succeeds.                                                                      */
int hz_hori_quantise(const float *src, size_t n, uint16_t *dst, int device);
int hz_hori_dequantise(const uint16_t *src, size_t n, float *dst, int device);
/* hz_topo_params / hz_topo_params_planes on codes (clause 17): planes = 0: hori_q is          */
/* u16[len_0][len_1][len_2], planes = 1: u16[len_2][len_0][len_1].  Every pointer is host or device memory, hori_q  */
/* aligned to 2 bytes (a view at an odd element is fine); any non-empty subset of svf / vsf / openness.  A code is  */
/* decoded to float32 first and the float kernels' operation sequence runs on that float32: each map is, word for   */
/* word, the map hz_topo_params returns on decode(hori_q); 0xFFFF behaves as a NaN horizon does (svf and vsf take   */
/* the tilted plane's own horizon and stay numbers, openness becomes NaN).  No float32 copy of the horizon is made: */
/* cell-major codes are read by the tiled kernel, planes of codes -- one lane per cell, coalesced as they lie -- by */
/* the direct kernel; host planes are staged in row slabs ("planes_chunk").  Checks and messages as hz_topo_params, */
/* plus "planes must be 0 or 1" and "an array is not aligned to its element type".                                  */
int hz_topo_params_q16(const float *azim, const uint16_t *hori_q, int planes, const float *vec_tilt,
                       int len_0, int len_1, int len_2,
                       float *svf, float *vsf, float *openness, int device);
/* hz_horizon_gridded_planes / _scene_planes with `hori_q` in place of hori_planes (host or device memory):       */
/* planes = 0: u16[rows][dim_in_1][azim_num], planes = 1: u16[azim_num][rows][dim_in_1].  Each chunk of rows is    */
/* traced into the bounded float32 chunk buffer, reduced there -- opts->svf and topo come from the unquantised     */
/* chunk and are bit-identical to the float call's maps -- and then encoded (planes = 1: and transposed) into its  */
/* place: hori_q == encode(what the float call of the same layout writes), word for word.  A device hori_q is      */
/* written in place; a host hori_q goes through one more chunk buffer of half the size and one copy.  Row slabs,   */
/* hori_is_slab, inputs_are_slab and chunk_rows mean what they mean for hori_planes; rows outside the slab are     */
/* left untouched.  opts->skip_hori is HZ_ERR_ARG.  stats->scratch_bytes includes the chunk buffers; t_d2h_s       */
/* includes the chunk copies of a host hori_q.                                                                     */
int hz_horizon_gridded_q16(const float *vert_grid, int dem_dim_0, int dem_dim_1,
                           const float *vec_norm, const float *vec_north,
                           int offset_0, int offset_1,
                           uint16_t *hori_q, int planes, int dim_in_0, int dim_in_1,
                           int azim_num, float dist_search, float hori_acc,
                           const char *ray_algorithm, const char *geom_type,
                           const float *vert_simp, int num_vert_simp,
                           const int32_t *tri_ind_simp, int num_tri_simp,
                           float elev_ang_low_lim, const uint8_t *mask,
                           float hori_fill, float ray_org_elev,
                           const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats);
int hz_horizon_gridded_scene_q16(const hz_scene *scene,
                                 const float *vec_norm, const float *vec_north,
                                 int offset_0, int offset_1,
                                 uint16_t *hori_q, int planes, int dim_in_0, int dim_in_1,
                                 int azim_num, float dist_search, float hori_acc,
                                 const char *ray_algorithm,
                                 float elev_ang_low_lim, const uint8_t *mask,
                                 float hori_fill, float ray_org_elev,
                                 const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats);

/* ------------------------------------------------------------------------- */
/* The distance to the horizon of a gridded horizon (additive; DESIGN.md section 4, clause 16).  The reference    */
/* has it only for locations (the *_hori_dist variants, horizon_comp.cpp:519-612); the meaning is theirs: the      */
/* closest hit of the last ray that hit.  Per cell with mask == 1, azimuth a and horizon value h (float32; a code  */
/* is decoded first):  j = max{ i : elev_ang[i] <= h } in the ascending table of hz_horizon_tables (-1: none),      */
/* k = max(j - 5, 0); the ray of table entry k and azimuth a, direction and origin as the gridded horizon forms    */
/* them; the distance [metre] is the minimum t over all triangles (DEM mesh and outer TIN) accepted with           */
/* tfar = dist_search.  NaN where that ray hits nothing, where h is NaN and where mask != 1.  A nearer, lower      */
/* ridge that also rises above h - hori_acc is what is reported.                                                    */
/* hori_kind: HZ_HORI_PLANES and HZ_HORI_U16 or'ed -- f32[rows][dim_in_1][azim_num] (0), f32[azim_num][rows]        */
/* [dim_in_1] (1), and the same two of 16-bit codes (2, 3).  `dist` is float32 in the layout of `hori`.  Both may  */
/* be host or device memory; rows, row slabs (only the slab is read and written), opts->hori_is_slab (for hori     */
/* AND dist), inputs_are_slab and chunk_rows mean what they mean for hz_horizon_gridded_planes.  Two device        */
/* arrays are one launch; a host side moves through a bounded device buffer chunk by chunk.  hz_stats: num_rays    */
/* (distance rays), num_cells, t_kernel_s, t_h2d_s, t_d2h_s, t_total_s, scratch_bytes.                              */
/* ------------------------------------------------------------------------- */
#define HZ_HORI_F32 0
#define HZ_HORI_PLANES 1
#define HZ_HORI_U16 2
int hz_horizon_distance(const float *vert_grid, int dem_dim_0, int dem_dim_1,
                        const void *hori, int hori_kind, float *dist,
                        const float *vec_norm, const float *vec_north,
                        int offset_0, int offset_1, int dim_in_0, int dim_in_1,
                        int azim_num, float dist_search, float hori_acc,
                        const char *geom_type,
                        const float *vert_simp, int num_vert_simp,
                        const int32_t *tri_ind_simp, int num_tri_simp,
                        float elev_ang_low_lim, const uint8_t *mask, float ray_org_elev,
                        const hz_opts *opts, hz_stats *stats);
int hz_horizon_distance_scene(const hz_scene *scene,
                              const void *hori, int hori_kind, float *dist,
                              const float *vec_norm, const float *vec_north,
                              int offset_0, int offset_1, int dim_in_0, int dim_in_1,
                              int azim_num, float dist_search, float hori_acc,
                              float elev_ang_low_lim, const uint8_t *mask, float ray_org_elev,
                              const hz_opts *opts, hz_stats *stats);
/* The gridded horizon of any kind (hz_horizon_gridded_ex / _planes / _q16 by hori_kind) PLUS its distances in      */
/* dist_buffer f32, cell-major or planes as hori_kind says.  Inside the chunk loop the distance kernel runs on the   */
/* float32 chunk after it was traced and reduced and before it is laid out or encoded, so dist_buffer equals         */
/* hz_horizon_distance on the float32 horizon of the call, word for word -- for 16-bit codes too -- and `hori` and    */
/* the maps are those of the call without distances.  opts->skip_hori is HZ_ERR_ARG.  hz_stats: num_rays and          */
/* t_kernel_s include the distance rays and their kernel, t_d2h_s the copies of a host dist_buffer.                  */
int hz_horizon_gridded_dist(const float *vert_grid, int dem_dim_0, int dem_dim_1,
                            const float *vec_norm, const float *vec_north,
                            int offset_0, int offset_1,
                            void *hori, int hori_kind, float *dist_buffer,
                            int dim_in_0, int dim_in_1,
                            int azim_num, float dist_search, float hori_acc,
                            const char *ray_algorithm, const char *geom_type,
                            const float *vert_simp, int num_vert_simp,
                            const int32_t *tri_ind_simp, int num_tri_simp,
                            float elev_ang_low_lim, const uint8_t *mask,
                            float hori_fill, float ray_org_elev,
                            const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats);
int hz_horizon_gridded_scene_dist(const hz_scene *scene,
                                  const float *vec_norm, const float *vec_north,
                                  int offset_0, int offset_1,
                                  void *hori, int hori_kind, float *dist_buffer,
                                  int dim_in_0, int dim_in_1,
                                  int azim_num, float dist_search, float hori_acc,
                                  const char *ray_algorithm,
                                  float elev_ang_low_lim, const uint8_t *mask,
                                  float hori_fill, float ray_org_elev,
                                  const hz_opts *opts, const hz_topo_out *topo, hz_stats *stats);

/* Horizon (and optionally distance to the horizon) for arbitrary locations; argument list     */
/* mirrors horizon_locations_comp (horizon_comp.h:22-34, horizon_comp.cpp:828-1094).           */
/* coords f32[num_loc][3], vec_norm / vec_north f32[num_loc][3], ray_org_elev f32[num_loc],    */
/* hori_buffer f32[num_loc][azim_num]; hori_dist_buffer f32[num_loc][azim_num] is only written */
/* when hori_dist_out != 0 (may be NULL otherwise).  Locations whose normal never meets the    */
/* mesh keep the caller's values (the reference pre-fills NaN, horizon.pyx:331-341).           */
int hz_horizon_locations(const float *vert_grid, int dem_dim_0, int dem_dim_1,
                         const float *coords, const float *vec_norm, const float *vec_north,
                         float *hori_buffer, float *hori_dist_buffer, int num_loc,
                         int azim_num, float dist_search, float hori_acc,
                         const char *ray_algorithm, const char *geom_type,
                         float elev_ang_low_lim, const float *ray_org_elev, int hori_dist_out,
                         const hz_opts *opts, hz_stats *stats);
int hz_horizon_locations_scene(const hz_scene *scene,
                               const float *coords, const float *vec_norm, const float *vec_north,
                               float *hori_buffer, float *hori_dist_buffer, int num_loc,
                               int azim_num, float dist_search, float hori_acc,
                               const char *ray_algorithm, float elev_ang_low_lim,
                               const float *ray_org_elev, int hori_dist_out,
                               const hz_opts *opts, hz_stats *stats);

/* Trig tables exactly as horizon_comp.cpp:711-731 builds them (host side;     */
/* exported so tests can compare them bit for bit with the oracle).            */
/* Returns elev_num through *elev_num; arrays may be NULL to query the size.   */
int hz_horizon_tables(int azim_num, float hori_acc, float elev_ang_low_lim,
                      float *azim_sin, float *azim_cos, int elev_cap,
                      float *elev_ang, float *elev_sin, float *elev_cos,
                      int *elev_num);

/* Sky view factor from a horizon array: _sky_view_factor_cy,                  */
/* topo_param.pyx:412-460.                                                     */
int hz_sky_view_factor(const float *azim, const float *hori, const float *vec_tilt,
                       int len_0, int len_1, int len_2, float *svf, int device);
/* _visible_sky_fraction_cy (topo_param.pyx:499-543) and _topographic_openness_cy (:577-603):   */
/* the other two reductions of the same horizon array.                                          */
int hz_visible_sky_fraction(const float *azim, const float *hori, const float *vec_tilt,
                            int len_0, int len_1, int len_2, float *vsf, int device);
int hz_topographic_openness(const float *azim, const float *hori, int len_0, int len_1, int len_2,
                            float *top, int device);
/* All three reductions of a materialised horizon array in one pass over it: any of svf / vsf / openness may be    */
/* NULL, not all; vec_tilt is needed (and read) only for svf / vsf, which also need len_2 >= 2.  Each map is         */
/* bit-identical to the single-output function's.                                                                   */
int hz_topo_params(const float *azim, const float *hori, const float *vec_tilt, int len_0, int len_1, int len_2,
                   float *svf, float *vsf, float *openness, int device);

/* Test hooks for the hand-written build primitives (stable radix sort of uint32 pairs by key,   */
/* exclusive prefix sum); host arrays, in place / in -> out.  Not needed by a binding.            */
int hz_debug_sort_pairs(uint32_t *keys, uint32_t *vals, size_t n, int device);
int hz_debug_exclusive_scan(const uint32_t *in, uint32_t *out, size_t n, int device);
/* Test hooks for the device build of the refraction math (hz_crmath.h, hz_horisun_refrac.h; hz_crmath_probe.hip): one thread */
/* per element, host arrays in and out; n == 0 succeeds without a launch and writes nothing.  Not needed by a binding.        */
/* `which`: 0 hz_crm_acosf, 1 hz_crm_tanf, 2 hz_crm_cosf, 3 hz_crm_sinf, 4 hz_crm_powf(x, y), 5 horisun_deg2rad_f,             */
/* 6 horisun_rad2deg_f, 7 horisun_atmos_refrac(x, (double)y).                                                                  */
/* hz_debug_crmath_eval: out[i] = f(x[i], y[i]); y may be NULL (then 0) for the one-argument functions.                        */
/* hz_debug_crmath_range: out[i] = f(the float with the bit pattern first_bits + i * stride (uint32 arithmetic), y) -- a sweep */
/* uploads nothing.  hz_debug_refrac_factor: the per-cell float64 pressure / temperature factor of the refraction formula     */
/* from elevation[n] [m], by the kernel Terrain and HorizonTerrain.refraction run.                                            */
int hz_debug_crmath_eval(int which, const float *x, const float *y, float *out, size_t n, int device);
int hz_debug_crmath_range(int which, uint32_t first_bits, uint32_t stride, size_t n, float y, float *out, int device);
int hz_debug_refrac_factor(const float *elevation, size_t n, double *out_f64, int device);
/* Machine calibration for the roofline (bench.py, untimed section).  hz_debug_valu_peak: chains of      */
/* independent v_fma_f32 (packed = 1: v_pk_fma_f32) at 8 waves per SIMD, `waves_per_simd` rounds of      */
/* 3.5 ms (the name is historical: it only sets the length of the run; long pure-FMA runs are power-     */
/* limited) -> wave-level VALU instructions per second and SIMD, the engine clock [GHz], the SIMD count. */
/* hz_debug_copy_peak: float4 device-to-device copy of `bytes` -> read + write GB/s.                     */
int hz_debug_valu_peak(int device, int packed, int waves_per_simd, double *winst_per_s_per_simd,
                       double *clock_ghz, int *simds);
int hz_debug_copy_peak(int device, size_t bytes, double *gbs);
/* issue rate of one VALU instruction kind (selector list: hz_bench.hip) in cycles per wave64 instruction per SIMD */
int hz_debug_inst_rate(int device, int op, double *cycles_per_inst);
/* test knobs (process wide; results never depend on them): "shadow_fast_cap" = entries of the shadow kernel's fast stack (< 0: */
/* the default; small values make the in-kernel retry with the level stack the common case), "topo_wide" = 1: the reductions    */
/* over the azimuth axis use the one-lane-per-cell fallback kernel, "accum_chunk" = sun positions per chunk of                   */
/* hz_terrain_accumulate and hz_terrain_sw_dir_cor_coarse (<= 0: the default, from the scratch budget), "coarse_tile" = cells   */
/* of the LDS tile of hz_terrain_sw_dir_cor_coarse's reduction (<= 0 or above the default: the default; blocks wider than the  */
/* tile take the kernel without LDS), "horisun_chunk" = sun positions per launch of hz_horizon_terrain_run (<= 0: the default), */
/* "horisun_coarse_route" / "horisun_coarse_tile": see hz_horizon_terrain_sw_dir_cor_coarse (< 0: the default),                 */
/* "planes_chunk" = cells per staging chunk of hz_hori_to_planes / _from_planes / hz_topo_params_planes (<= 0: the default),   */
/* "topo_planes_direct" = 1: hz_topo_params_planes reduces float32 planes with the direct one-lane-per-cell kernel that planes */
/* of codes always take, not by transposing row slabs back (0 or < 0: the default; the maps are the same words either way),   */
/* "q16_chunk" = elements per staging chunk of hz_hori_quantise / hz_hori_dequantise (<= 0: the default),                        */
/* "leaf_lend" = 0: the horizon kernel's fast stack runs without leaf lending (1 or < 0: the default, with it)                  */
/* "flat_refill" = 0: guess_constant's refill runs the search state machine's if-chain (1 or < 0: the default, the branch-free */
/* pass; it belongs to the instantiations with leaf lending, so "leaf_lend" = 0 switches it off too),                           */
/* "regroup_rule" = 0: the horizon kernel's ray-compaction threshold is absolute -- a wave leaves the traversal loop when fewer */
/* than min(regroup, lanes that entered with a ray) still traverse, regroup 36 by default -- (1 or < 0: the default, the         */
/* threshold scales with the lanes that entered, regroup 44 by default; bit 16 of hz_opts.regroup forces 0 for one call),       */
/* "regroup_round" = 0 ... 63: the rounding addend of that scaled threshold, (regroup * lanes + round) >> 6 (< 0: the default),  */
/* "horidist_traversal" = 0: the distance kernel of hz_horizon_distance runs hz_closest's slot order (1 or < 0: the default,   */
/* the children of a node front to back), "horidist_block_w" = 16, 32, 64: cells per row of a wave's block in                  */
/* hz_horizon_distance (8 or < 0: the default, 8 x 8 cells),                                                                    */
/* "panorama_traversal" = 0: the kernel of hz_terrain_panorama runs hz_closest's slot order (1 or < 0: the default, the children */
/* of a node front to back), "panorama_budget" = n > 0: bytes of staged output per chunk of hz_terrain_panorama (<= 0: 256 MiB)  */
int hz_debug_set(const char *key, int value);

/* ------------------------------------------------------------------------- */
/* Steps next to the path: slope and input preparation */
/* ------------------------------------------------------------------------- */

/* _slope_plane_meth_cy / _slope_vector_meth_cy, topo_param.pyx:84-225, :284-372.               */
/* x, y, z f32[len_0][len_1]; rot_mat f32[len_0][len_1][3][3] or NULL; vec_tilt f32[..][3]      */
/* (border cells NaN).                                                                          */
int hz_slope_plane_meth(const float *x, const float *y, const float *z, int len_0, int len_1,
                        const float *rot_mat, int output_rot, float *vec_tilt, int device);
int hz_slope_vector_meth(const float *x, const float *y, const float *z, int len_0, int len_1,
                         const float *rot_mat, int output_rot, float *vec_tilt, int device);
/* ellps: 0 "sphere", 1 "GRS80", 2 "WGS84".                                                     */
/* _lonlat2ecef_1d, transform.pyx:60-103: lon, lat f64[n] [degree], h f32[n] -> f64[n] x 3      */
int hz_lonlat2ecef(const double *lon, const double *lat, const float *h, size_t n, int ellps,
                   double *x_ecef, double *y_ecef, double *z_ecef, int device);
/* -- NOT a row of the scope table (SURVEY.md section 8(f)4 names transform.pyx:60-103, 152-189, 231-261 only; section 2   */
/*    lists coordinate transforms as out of scope): the two Swiss-grid routines below were added in round 2, are kept   */
/*    because the reference's swissALTI3D examples feed the path through them, and are not part of any parity claim.    */
/* _wgs2swiss_1d, transform.pyx:306-345: lon, lat f64[n] [degree], h_wgs f32[n] -> LV95 e, n f64[n] [m], */
/* h_ch f32[n]; _swiss2wgs_1d, transform.pyx:390-432: the inverse (swisstopo's approximate formulas)  */
int hz_wgs2swiss(const double *lon, const double *lat, const float *h_wgs, size_t n,
                 double *e, double *n_out, float *h_ch, int device);
int hz_swiss2wgs(const double *e, const double *n_in, const float *h_ch, size_t n,
                 double *lon, double *lat, float *h_wgs, int device);
/* _ecef2enu_1d with TransformerEcef2enu(lon_or, lat_or, ellps), transform.pyx:152-189, 438-487 */
int hz_ecef2enu(const double *x_ecef, const double *y_ecef, const double *z_ecef, size_t n,
                double lon_or, double lat_or, int ellps, float *x_enu, float *y_enu, float *z_enu,
                int device);
/* _ecef2enu_vector_1d, transform.pyx:231-261: f32[n][3] -> f32[n][3]                           */
int hz_ecef2enu_vector(const float *vec_ecef, size_t n, double lon_or, double lat_or, int ellps,
                       float *vec_enu, int device);
/* _surf_norm_1d, direction.pyx:48-70                                                           */
int hz_surf_norm(const double *lon, const double *lat, size_t n, float *vec_norm_ecef, int device);
/* _north_dir_1d, direction.pyx:125-178                                                         */
int hz_north_dir(const double *x_ecef, const double *y_ecef, const double *z_ecef,
                 const float *vec_norm_ecef, size_t n, int ellps, float *vec_north_ecef, int device);

/* rearrange_pad_buffer / pad_buffer, auxiliary.py:49-95, :99-133: coordinate planes x, y, z f32[num_vertices]  */
/* (row-major DEM) -> the interleaved xyz vertex buffer `vert_grid` every entry point above takes, with the    */
/* reference's zero padding.  hz_vert_grid_len gives the padded length in floats.  With device pointers the     */
/* whole chain lon/lat/elevation -> ENU -> vert_grid -> scene -> horizon / SVF / shadow never leaves HBM.       */
size_t hz_vert_grid_len(size_t num_vertices);
int hz_pack_vertices(const float *x, const float *y, const float *z, size_t num_vertices, float *vert_grid,
                     size_t vert_grid_len, int device);

/* ------------------------------------------------------------------------- */
/* Shadow: handle API mirroring class CppTerrain (shadow_comp.h:4-39)          */
/* ------------------------------------------------------------------------- */
typedef struct hz_terrain hz_terrain;

/* CppTerrain::CppTerrain, shadow_comp.cpp:304-308 */
int hz_terrain_create(int device, hz_terrain **terrain);
/* CppTerrain::initialise, shadow_comp.cpp:318-380 (argument order as there)   */
int hz_terrain_initialise(hz_terrain *terrain, const float *vert_grid,
                          int dem_dim_0, int dem_dim_1, int offset_0, int offset_1,
                          const float *vec_tilt, const float *vec_norm,
                          int dim_in_0, int dim_in_1,
                          const float *surf_enl_fac, const float *elevation,
                          const uint8_t *mask, const char *geom_type,
                          float sw_dir_cor_fill, float ang_max, int refrac_cor,
                          hz_stats *stats);
/* additive: initialise on an existing scene (scene must outlive the terrain)  */
int hz_terrain_initialise_scene(hz_terrain *terrain, const hz_scene *scene,
                                int offset_0, int offset_1,
                                const float *vec_tilt, const float *vec_norm,
                                int dim_in_0, int dim_in_1,
                                const float *surf_enl_fac, const float *elevation,
                                const uint8_t *mask,
                                float sw_dir_cor_fill, float ang_max, int refrac_cor);
/* CppTerrain::shadow, shadow_comp.cpp:386-491: u8[y][x], 0/1/2/3              */
int hz_terrain_shadow(hz_terrain *terrain, const float *sun_position,
                      uint8_t *shadow_buffer, hz_stats *stats);
/* CppTerrain::sw_dir_cor, shadow_comp.cpp:495-605: f32[y][x]                  */
int hz_terrain_sw_dir_cor(hz_terrain *terrain, const float *sun_position,
                          float *sw_dir_cor_buffer, hz_stats *stats);
/* additive batch forms: num_sun positions f32[num_sun][3] ->                  */
/* buffers [num_sun][y][x]; all positions in ONE launch (grid.y = position)    */
int hz_terrain_shadow_batch(hz_terrain *terrain, const float *sun_positions,
                            int num_sun, uint8_t *shadow_buffers, hz_stats *stats);
int hz_terrain_sw_dir_cor_batch(hz_terrain *terrain, const float *sun_positions,
                                int num_sun, float *sw_dir_cor_buffers, hz_stats *stats);
/* additive: weighted sums over num_sun >= 1 positions without a map per position. For unmasked  */
/* cells, sw_dir_cor_sum[c] = (float)(sum over s ascending of (double)w[s] * sw_dir_cor_s[c]) and  */
/* sunlit_sum[c] = (float)(sum of (double)w[s] * [shadow_s[c] == 0]), float64 accumulators rounded */
/* once; masked cells get sw_dir_cor_fill in both. weights f32[num_sun] (NULL = ones); an output   */
/* NULL = not wanted (at least one). Positions, weights and outputs f32[y][x] may be host or       */
/* device pointers. One ray per (cell, position) with dot_ts > 0 if sunlit_sum is wanted, else    */
/* with dot_ts > dot_prod_min; device scratch (hz_stats.scratch_bytes) does not grow with num_sun  */
int hz_terrain_accumulate(hz_terrain *terrain, const float *sun_positions, const float *weights, int num_sun,
                          float *sw_dir_cor_sum, float *sunlit_sum, hz_stats *stats);
/* additive: per sun position, means over blocks of pixel_per_gc_0 x pixel_per_gc_1 cells of the inner domain (each >= 1 and  */
/* a divisor of dim_in_0 / dim_in_1; gy = dim_in_0 / pixel_per_gc_0, gx = dim_in_1 / pixel_per_gc_1), without a map per        */
/* position. For position s and coarse cell (I, J), B = the cells (i, j), I * P0 <= i < (I + 1) * P0, J * P1 <= j < (J + 1)    */
/* * P1, with mask[i][j] == 1, and n = |B|:                                                                                     */
/*   f_cor[s][I][J] = (float)(SUM / (double)n), SUM a float64 accumulator that starts at 0.0 and takes                          */
/*     (double)sw_dir_cor_s[i][j] -- bit for bit what hz_terrain_sw_dir_cor writes for position s -- one cell at a time over B, */
/*     i ascending and within a row j ascending (the order is part of the contract: a float64 sum of float32 values is not      */
/*     exact in general; the library is built with -ffp-contract=off);                                                          */
/*   sunlit_frac[s][I][J] = (float)((double)n_lit / (double)n), n_lit = the cells of B for which hz_terrain_shadow gives 0;    */
/*   n == 0: both are sw_dir_cor_fill.                                                                                          */
/* f_cor, sunlit_frac f32[num_sun][gy][gx]; NULL = not wanted (at least one; they must differ). Positions and outputs may be    */
/* host or device pointers. Rays as in hz_terrain_accumulate: one per (cell, position) with dot_ts > 0 if sunlit_frac is        */
/* wanted (it serves both outputs), else with dot_ts > dot_prod_min; device memory besides the outputs                          */
/* (hz_stats.scratch_bytes) does not grow with num_sun                                                                          */
int hz_terrain_sw_dir_cor_coarse(hz_terrain *terrain, const float *sun_positions, int num_sun,
                                 int pixel_per_gc_0, int pixel_per_gc_1,
                                 float *f_cor, float *sunlit_frac, hz_stats *stats);
/* additive: line-of-sight maps from observer points (DESIGN.md section 4 clause 18). observers f32[num_obs][3] are points of   */
/* the scene's ENU frame (the frame of sun_position), num_obs >= 1.  For observer P and inner cell c, everything float32, every */
/* multiply, add and divide rounded on its own, associated as in hz_terrain_shadow's set-up, in this order:                      */
/*   mask[c] != 1 -> 3;  T = v + norm * target_elev (v = the DEM vertex of c), d = P - T, mag = sqrtf((dx dx + dy dy) + dz dz);  */
/*   a limit is given and mag > max_dist -> 4 (no ray);  !(mag > 0) -> 0 (no ray);  u = d / mag;                                 */
/*   facing and !((tilt_x u_x + tilt_y u_y) + tilt_z u_z > 0) -> 1 (no ray: the surface faces away);                             */
/*   else one any-hit ray with origin T, direction u and tfar = mag: a hit -> 2, no hit -> 0.                                    */
/* Refraction is never applied (a Terrain initialised with refrac_cor gives the same codes).  visible u8[num_obs][y][x] takes   */
/* the codes, seen_count i32[y][x] the number of observers with code 0 for the cell (masked cells: -1), cells_seen              */
/* i64[num_obs] the number of cells with code 0 per observer; NULL = not wanted (at least one; they must differ).  Every        */
/* pointer may be host or device memory.  target_elev >= 0.005 [m]; max_dist [m]: <= 0, NaN or infinite = no limit.             */
/* stats->num_rays = rays traced.  hz_stats.scratch_bytes = device memory the call allocates besides the caller's buffers: the  */
/* staging of a host seen_count; it does not grow with num_obs.  Not counted there: the staging of a host visible / cells_seen  */
/* (num_obs * cells bytes, num_obs * 8 bytes) and the handle's own staging buffer for host observers, which hz_terrain_shadow   */
/* and the batch calls share: it is kept with the handle, 12 bytes per observer of one launch, at most 32768 * 12 bytes         */
int hz_terrain_viewshed(hz_terrain *terrain, const float *observers, int num_obs, float target_elev, float max_dist,
                        int facing, uint8_t *visible, int32_t *seen_count, int64_t *cells_seen, hz_stats *stats);
/* additive: the lowest target height in sight per observer and cell (DESIGN.md section 4 clause 19).  observers as in          */
/* hz_terrain_viewshed; heights f32[num_heights] is the caller's table H: 1 <= num_heights <= 65535, finite, strictly           */
/* increasing, H[0] >= 0.005 [m] (checked here; HZ_ERR_ARG otherwise); the kernel indexes it and does no arithmetic on it.      */
/* visible(k): T = v + norm * H[k], d = P - T, mag and u as in hz_terrain_viewshed; !(mag > 0) is visible without a ray; else   */
/* one any-hit ray (T, u, tfar = mag), no hit = visible.  No facing test; never refracted.  Per observer and cell, in order:    */
/*   mask[c] != 1 -> NaN;  a limit is given and mag(H[0]) > max_dist -> +inf (no ray);  !visible(n - 1) -> +inf;                 */
/*   n == 1 or visible(0) -> H[0];  else lo = 0, hi = n - 1, while hi - lo > 1: mid = (lo + hi) >> 1,                            */
/*   visible(mid) ? hi = mid : lo = mid;  the result is H[hi].                                                                   */
/* height f32[num_obs][y][x] takes the results, lowest f32[y][x] their minimum over the observers (+inf where no observer is   */
/* reached, NaN where masked), cells_reached i64[num_obs] the cells with a finite result per observer; NULL = not wanted (at   */
/* least one; they must differ).  Every pointer may be host or device memory (a device table is read back for its checks).     */
/* max_dist [m]: <= 0, NaN or infinite = no limit.  stats->num_rays = rays traced.  hz_stats.scratch_bytes = device memory the  */
/* call allocates besides the caller's buffers: a host table (4 bytes per entry) and the staging of a host lowest; it does not */
/* grow with num_obs.  Not counted: the staging of a host height / cells_reached and the handle's buffer for host observers.   */
int hz_terrain_sight_height(hz_terrain *terrain, const float *observers, int num_obs, const float *heights, int num_heights,
                            float max_dist, float *height, float *lowest, int64_t *cells_reached, hz_stats *stats);
/* additive: depth images of the scene from observer points (DESIGN.md section 4 clause 20).  observers f32[num_obs][3] as in   */
/* hz_terrain_viewshed.  An image has elev_num x azim_num pixels; the caller passes the four float32 tables                      */
/* azim_sin / azim_cos f32[azim_num] and elev_sin / elev_cos f32[elev_num] (float64 sin / cos of the angles, rounded once;      */
/* azimuth clockwise from north): the kernel does no trigonometry.  vec_north, vec_norm f32[num_obs][3]: the unit vectors of    */
/* each observer's frame, both or neither (both NULL: north = (0, 1, 0), norm = (0, 0, 1)).  All float32, every product and sum */
/* rounded on its own.  Per observer s and pixel (e, a):                                                                         */
/*   east = north x norm;  rx = elev_cos[e] * azim_sin[a], ry = elev_cos[e] * azim_cos[a], rz = elev_sin[e];                     */
/*   dir = (east * rx + north * ry) + norm * rz;  one closest-hit ray (observer, dir, tfar = max_dist);                          */
/*   dist[s][e][a] = the minimum t over all accepted triangles, NaN if there is none;  point[s][e][a][c] = obs[c] + dir[c] * t   */
/*   (NaN x 3 if there is none);  hits[s] = the pixels of observer s with a hit.  A minimum that is zero is written as +0.0     */
/*   (an observer on the surface is accepted with T = +0 and T = -0 by the triangles around it), and point uses that value.     */
/* dist f32[num_obs][elev_num][azim_num], point f32[num_obs][elev_num][azim_num][3], hits i64[num_obs]; NULL = not wanted (at    */
/* least one; they must differ); every element is written.  Every pointer may be host or device memory.  Never refracted; mask, */
/* vec_tilt and the inner-domain offsets play no part.  HZ_ERR_ARG for counts < 1, elev_num * azim_num > 2^30, max_dist not      */
/* finite or <= 0, no output, or exactly one of the two frame arrays.  stats->num_rays = num_obs * elev_num * azim_num.          */
/* Observers go in chunks: a host dist / point is staged on the device one chunk at a time, at most 256 MiB                      */
/* ("panorama_budget" of hz_debug_set) or one observer's images.  hz_stats.scratch_bytes = that staging, host tables and the     */
/* chunk's host observers and frames; it does not grow with num_obs.  Not counted: the staging of a host hits (8 bytes each).    */
int hz_terrain_panorama(hz_terrain *terrain, const float *observers, int num_obs,
                        const float *azim_sin, const float *azim_cos, int azim_num,
                        const float *elev_sin, const float *elev_cos, int elev_num,
                        const float *vec_north, const float *vec_norm,   /* both NULL: planar frame */
                        float max_dist, float *dist, float *point, int64_t *hits, hz_stats *stats);
/* additive: any-hit and closest-hit for rays the caller supplies (DESIGN.md section 4 clause 21).  origins f32[num_rays][3] in */
/* the scene's frame (as observers of hz_terrain_viewshed), 1 <= num_rays <= 2^31 - 64, and exactly one of                      */
/*   directions f32[num_rays][3]: unit vectors, used as given (not normalised); ray i = (origins[i], directions[i], tfar =      */
/*     max_dist), max_dist finite and > 0;                                                                                      */
/*   targets f32[num_rays][3]: d = target - origin, mag = sqrtf((dx dx + dy dy) + dz dz); !(mag > 0): no ray -- occluded 0,      */
/*     dist and point NaN, not counted; else ray i = (origins[i], d / mag, tfar = mag).  max_dist is not read.                  */
/* All float32, every product, sum, square root and quotient rounded on its own.  Per ray:                                      */
/*   occluded[i] = 1 if a triangle is accepted within the ray, else 0;  dist[i] = the minimum t over all accepted triangles,    */
/*   NaN if there is none (a minimum that is zero is written as +0.0);  point[i][c] = origin[c] + dir[c] * dist[i] (NaN x 3).   */
/* occluded u8[num_rays], dist f32[num_rays], point f32[num_rays][3]; NULL = not wanted (at least one; they must differ); every */
/* element is written.  occluded alone runs an any-hit kernel that stops at the first accepted triangle; it is the byte the     */
/* closest-hit kernel writes.  order 0: the rays are traced in the caller's order; 1: each chunk in an order computed on the   */
/* device (a radix sort of origin and direction codes) -- the results do not depend on it.  Every pointer may be host or        */
/* device memory.  Never refracted; mask, vec_tilt and the inner-domain offsets play no part.  HZ_ERR_ARG for num_rays out of   */
/* range, both or neither of directions and targets, max_dist not finite or <= 0 with directions, order not 0 or 1, no output.  */
/* stats->num_rays = the rays traced (num_rays minus the targets on their origin).  The rays go in chunks (a multiple of 64):   */
/* host inputs and host outputs are staged on the device one chunk at a time and order 1 sorts one chunk at a time, together    */
/* at most 256 MiB ("cast_budget" of hz_debug_set) or 64 rays' worth, plus the sort's histograms (about 2 bytes per ray of a  */
/* chunk).  hz_stats.scratch_bytes = that memory; it does not grow with num_rays.                                                */
/* hz_debug_set: "cast_fast_cap" = n entries of the any-hit kernel's fast stack (0: level stack only; < 0: the                  */
/* default), "cast_sort_only" = 1: order 1 stops after the sort and writes no output (timing).                                  */
int hz_terrain_cast(hz_terrain *terrain, const float *origins, const float *directions, const float *targets, int num_rays,
                    float max_dist, int order, uint8_t *occluded, float *dist, float *point, hz_stats *stats);
/* additive: 1 = later shadow / sw_dir_cor calls run the counting instantiation and also fill   */
/* hz_stats.nodes_visited / tris_tested / wave_*_iters (slower; for the roofline's B_trav)      */
int hz_terrain_count_work(hz_terrain *terrain, int on);
/* CppTerrain::~CppTerrain, shadow_comp.cpp:310-316 */
int hz_terrain_destroy(hz_terrain *terrain);

/* ------------------------------------------------------------------------- */
/* Shadow from a stored horizon (additive; no BVH, no ray): the handle API of hz_terrain with the look-up       */
/* "the sun's elevation against the horizon at the sun's azimuth" in place of the ray.  Per unmasked cell and    */
/* position p (no atmospheric refraction):                                                                      */
/*   float32, as hz_terrain: o = v + norm * 0.05f, s = unit(p - o), dot_ns = (n.s), dot_ts = (tilt.s), sums      */
/*     associated (x + y) + z; shadow = 1 where !(dot_ts > 0), sw_dir_cor = 0 where !(dot_ts > dot_prod_min);     */
/*   float64 from the float32 s, norm, north, every product and sum rounded on its own: E = north x norm,        */
/*     cn = s.north, ce = s.E, cu = s.norm (x, y, z order), phi = atan2(ce, cn) (+ 2 pi if < 0),                 */
/*     u = phi * (A / (2 pi)), k = floor(u), t = u - k, h = (1 - t) * hori[k mod A] + t * hori[(k + 1) mod A],   */
/*     alpha = asin(min(max(cu, -1), 1)); terrain-shaded iff alpha < h (a NaN h: lit).                           */
/*   shadow 0 / 1 / 2 / 3 and sw_dir_cor = (dot_ts / max(dot_ns, dot_prod_min)) * surf_enl_fac or 0 as           */
/*   hz_terrain_shadow / _sw_dir_cor with "terrain-shaded" for "the ray hit"; the sums as hz_terrain_accumulate. */
/* hori f32[dim_in_0][dim_in_1][azim_num] [rad] for the azimuths 2 pi k / azim_num (what hz_horizon_gridded      */
/* writes); azim_num >= 1.  A device pointer `hori` is BORROWED (the caller keeps it alive until the handle is   */
/* initialised again or destroyed); a host `hori` and every other input, host or device, is copied.             */
/* ------------------------------------------------------------------------- */
typedef struct hz_horizon_terrain hz_horizon_terrain;
typedef struct hz_horisun_out {
    int32_t size;            /* sizeof(hz_horisun_out) */
    uint8_t* shadow;         /* u8 [num_sun][y][x], optional */
    float*   sw_dir_cor;     /* f32[num_sun][y][x], optional */
    float*   sw_dir_cor_sum; /* f32[y][x], optional (weighted) */
    float*   sunlit_sum;     /* f32[y][x], optional (weighted) */
} hz_horisun_out;
int hz_horizon_terrain_create(int device, hz_horizon_terrain** t);
int hz_horizon_terrain_initialise(hz_horizon_terrain* t, const float* hori, int azim_num,
        const float* vert_grid, int dem_dim_0, int dem_dim_1, int offset_0, int offset_1,
        const float* vec_tilt, const float* vec_norm, const float* vec_north, int dim_in_0, int dim_in_1,
        const float* surf_enl_fac, const uint8_t* mask, float sw_dir_cor_fill, float ang_max, hz_stats* stats);
/* hz_horizon_terrain_initialise with the horizon given as planes f32[azim_num][dim_in_0][dim_in_1] (host:       */
/* copied; device: borrowed).  hz_horizon_terrain_run then reads hori[k mod A] as planes[k mod A][cell]; the     */
/* arithmetic, the chunking of positions, the sums and the outputs are the same, and so is every result.         */
int hz_horizon_terrain_initialise_planes(hz_horizon_terrain* t, const float* planes, int azim_num,
        const float* vert_grid, int dem_dim_0, int dem_dim_1, int offset_0, int offset_1,
        const float* vec_tilt, const float* vec_norm, const float* vec_north, int dim_in_0, int dim_in_1,
        const float* surf_enl_fac, const uint8_t* mask, float sw_dir_cor_fill, float ang_max, hz_stats* stats);
/* hz_horizon_terrain_initialise with the horizon given as 16-bit codes (clause 15): hori_q u16[dim_in_0][dim_in_1][azim_num]    */
/* (planes = 0) or u16[azim_num][dim_in_0][dim_in_1] (planes = 1); host: copied, device: borrowed.  Refraction is off afterwards. */
/* hz_horizon_terrain_run, _sun_times, _sw_dir_cor_coarse and _refraction then work on the handle unchanged: every kernel loads  */
/* the two codes, applies decode as written above (float64 product, rounded to float32), widens that float32 to float64 and       */
/* continues with clause 10, 13 or 14, so every output is, word for word, that of a handle initialised with the float32 array     */
/* decode(hori_q) of the same layout.  hz_horizon_terrain_sw_dir_cor_coarse always takes the two-pass route on such a handle:     */
/* hz_debug_set("horisun_coarse_route", 0) is ignored for it (the fused kernel has no form that reads codes).                    */
int hz_horizon_terrain_initialise_q16(hz_horizon_terrain* t, const uint16_t* hori_q, int azim_num, int planes,
        const float* vert_grid, int dem_dim_0, int dem_dim_1, int offset_0, int offset_1,
        const float* vec_tilt, const float* vec_norm, const float* vec_north, int dim_in_0, int dim_in_1,
        const float* surf_enl_fac, const uint8_t* mask, float sw_dir_cor_fill, float ang_max, hz_stats* stats);
/* Atmospheric refraction (DESIGN.md section 4 clause 13) on or off for every later call on the handle, both      */
/* layouts, hz_horizon_terrain_run and both routes of hz_horizon_terrain_sw_dir_cor_coarse.  elevation           */
/* f32[dim_in_0][dim_in_1] [m], host or device, copied: the orthometric elevation of the inner-domain cells,     */
/* hz_terrain_initialise's; NULL = off.  On: the float32 set-up above becomes hz_terrain's with refrac_cor = 1,  */
/* word for word -- elev_ang_true from the unrefracted dot_ns, Saemundsson's correction with the cell's          */
/* pressure / temperature factor (float64, 8 B per cell, kept until destroy, initialise or NULL), s turned about */
/* unit(s x norm) by it, dot_ns and dot_ts formed from the turned s', which also feeds the float64 look-up.  A   */
/* sun at the cell's zenith gives NaN dot products: self-shaded.  hz_horizon_terrain_initialise(_planes)         */
/* switches it off.  stats (may be NULL): t_h2d_s, t_total_s, num_cells.                                         */
int hz_horizon_terrain_refraction(hz_horizon_terrain* t, const float* elevation /* f32[dim_in_0*dim_in_1]; NULL = off */,
        hz_stats* stats /* may be NULL */);
/* Any subset of the four outputs (at least one; NULL = not wanted; host or device pointers, all different) from  */
/* one pass: positions go in chunks, one launch per chunk.  weights f32[num_sun], NULL = ones (the sums only).   */
/* stats (may be NULL): t_kernel_s, t_d2h_s, t_total_s, num_cells, scratch_bytes = device memory of the call      */
/* besides per-position maps staged for host outputs; it does not grow with num_sun                             */
int hz_horizon_terrain_run(hz_horizon_terrain* t, const float* sun_positions, const float* weights /* NULL = ones */,
        int num_sun, const hz_horisun_out* out, hz_stats* stats);
/* DESIGN.md section 4 clause 14: sunrise, sunset, sunshine duration and the number of sunlit spells per cell over a sun track.  */
/* sun_positions f32[num_sun][3], times f64[num_sun] (finite, strictly increasing, the caller's unit), num_sun >= 1.  For every   */
/* unmasked cell, in ascending s:                                                                                                 */
/*   set-up: the float32 set-up above (with hz_horizon_terrain_refraction on: the refracted one, steps 1 - 7 of clause 13 for     */
/*     every cell, without the early exit for back slopes) gives s, dot_ns, dot_ts;                                               */
/*   look-up, for EVERY position, also where dot_ts <= 0: h and alpha as above; d = alpha - h (float64; NaN for a NaN horizon),   */
/*     beta = asin(fmin(fmax((double)dot_ts, -1.0), 1.0)), g = fmin(d, beta) (IEEE fmin: a NaN d leaves beta) -- the sun's          */
/*     clearance over terrain and surface [rad];                                                                                  */
/*   lit = dot_ts > 0 && !(alpha < h): exactly "shadow gives 0" for that cell and position; g never decides it;                    */
/*   events: s = 0: if lit, open = rise = times[0], n = 1.  s >= 1 and lit != lit_prev: f = g_prev / (g_prev - g); if !(f >= 0 &&   */
/*     f <= 1) f = 0.5; tau = times[s-1] + f * (times[s] - times[s-1]), every operation float64 and rounded on its own; up:         */
/*     open = tau, if n == 0 rise = tau, n += 1; down: dur += tau - open, set = tau.  After the last position, if lit:             */
/*     dur += times[num_sun-1] - open, set = times[num_sun-1].                                                                    */
/*   sunrise = (float)rise, sunset = (float)set, duration = (float)dur (one rounding each), intervals = n.  Never lit: NaN, NaN,   */
/*   0.0f, 0.  Masked cells (mask != 1): sw_dir_cor_fill in the three float maps, -1 in intervals.                                 */
/* Both horizon layouts give the same words, and the position chunk ("horisun_chunk") changes none.  Any subset of the four        */
/* outputs f32 / i32 [dim_in_0][dim_in_1] (at least one; NULL = not wanted; all different); positions, times and outputs may be    */
/* host or device pointers.  Between the launches of a call the running state lives in 44 B per cell; a call of one chunk needs    */
/* none.  stats (may be NULL): t_kernel_s, t_d2h_s, t_total_s, num_cells, scratch_bytes = that state plus staging; it does not     */
/* grow with num_sun                                                                                                             */
typedef struct hz_suntimes_out {
    int32_t size;            /* sizeof(hz_suntimes_out) */
    float*   sunrise;        /* f32[y][x], optional */
    float*   sunset;         /* f32[y][x], optional */
    float*   duration;       /* f32[y][x], optional */
    int32_t* intervals;      /* i32[y][x], optional */
} hz_suntimes_out;
int hz_horizon_terrain_sun_times(hz_horizon_terrain* t, const float* sun_positions, const double* times,
        int num_sun, const hz_suntimes_out* out, hz_stats* stats);
/* DESIGN.md section 4 clause 12: hz_terrain_sw_dir_cor_coarse from the stored horizon.  For position s and coarse cell       */
/* (I, J), B = the cells (i, j), I * P0 <= i < (I + 1) * P0, J * P1 <= j < (J + 1) * P1, with mask[i][j] == 1, and n = |B|:     */
/*   f_cor[s][I][J] = (float)(SUM / (double)n), SUM a float64 accumulator that starts at 0.0 and takes (double)v one cell at a   */
/*     time over B, i ascending and within a row j ascending, v = bit for bit what hz_horizon_terrain_run writes into           */
/*     sw_dir_cor for that cell and position (a masked or unlit cell may contribute +0.0 instead of being skipped: the           */
/*     accumulator is never -0.0, so the add changes no bit);                                                                   */
/*   sunlit_frac[s][I][J] = (float)((double)n_lit / (double)n), n_lit = the cells of B whose shadow code is 0;                   */
/*   n == 0: both are sw_dir_cor_fill.  With hz_horizon_terrain_refraction on, v and the codes are the refracted sun's.          */
/* pixel_per_gc_0 / _1 >= 1 and divisors of dim_in_0 / dim_in_1; f_cor, sunlit_frac f32[num_sun][gy][gx], NULL = not wanted (at */
/* least one; they must differ); positions and outputs host or device pointers.  The look-up is evaluated for the cells with    */
/* dot_ts > 0 if sunlit_frac is wanted (it serves both outputs), else for dot_ts > dot_prod_min.  Both horizon layouts give the */
/* same words.  Positions go in chunks ("horisun_chunk").  Two routes, chosen by hz_debug_set("horisun_coarse_route", r):       */
/* r = 1, two passes per chunk: the look-up kernel of hz_horizon_terrain_run into scratch maps (5 B per cell and position of   */
/* the chunk), then hz_terrain_sw_dir_cor_coarse's reduction, which obeys "coarse_tile"; r = 0, one fused kernel per chunk, no  */
/* map per position; blocks wider than its LDS tile ("horisun_coarse_tile" cells, <= 0 or above the default of 4096: the         */
/* default) go the two-pass route.  r < 0 (the default): the route measured as the faster one for the layout, at present the     */
/* two-pass route for both.  stats as                                                                      */
/* hz_horizon_terrain_run; scratch_bytes = device memory besides the outputs and their staging, it does not grow with num_sun   */
int hz_horizon_terrain_sw_dir_cor_coarse(hz_horizon_terrain *t, const float *sun_positions, int num_sun,
                                         int pixel_per_gc_0, int pixel_per_gc_1,
                                         float *f_cor, float *sunlit_frac, hz_stats *stats);
int hz_horizon_terrain_destroy(hz_horizon_terrain* t);

/* ------------------------------------------------------------------------- */
/* Ocean masking: the `mask` argument of the entry points above, from a land-sea mask and the coastline        */
/* ------------------------------------------------------------------------- */
/* Contract, all float64, every operation rounded once: for a water cell c (mask_land[c] == 0) and a vertex p    */
/*   d2(c, p) = ((cx - px) * (cx - px) + (cy - py) * (cy - py)) + (cz - pz) * (cz - pz)                         */
/*   dist_chord[c] = sqrt(min over p of d2(c, p)), correctly rounded; land cells NaN; num_pts == 0: +inf         */
/*   mask_buffer[c] = dist_chord[c] > dist_thr; land cells 0                                                    */
/* x_ecef, y_ecef, z_ecef f64[len_0][len_1] [m], mask_land u8[len_0][len_1] (0 = water), pts_ecef                */
/* f64[num_pts][3] [m] (num_pts < 2^31; NULL allowed when 0); host or device pointers.  The vertices are indexed  */
/* on the device in every call (Morton sort, boxes over leaves of 8); the results do not depend on the index.   */
/* stats (may be NULL): t_bvh_s index build, t_kernel_s query, t_h2d_s, t_d2h_s, t_total_s, num_cells = water    */
/* cells queried, scratch_bytes = device memory of the index and its build.                                     */
/* coastline_distance, ocean_masking.py:163-212 (the k-d tree query for every water cell)                       */
int hz_coastline_distance(const double *x_ecef, const double *y_ecef, const double *z_ecef,
                          const uint8_t *mask_land, int len_0, int len_1,
                          const double *pts_ecef, size_t num_pts,
                          double *dist_chord, int device, hz_stats *stats);
/* coastline_buffer, ocean_masking.py:217-345, without its block pre-classification: every water cell is decided  */
/* exactly, by an any-hit query that ends at the first vertex within dist_thr                                    */
int hz_coastline_buffer(const double *x_ecef, const double *y_ecef, const double *z_ecef,
                        const uint8_t *mask_land, int len_0, int len_1,
                        const double *pts_ecef, size_t num_pts, double dist_thr,
                        uint8_t *mask_buffer, int device, hz_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* HORAYZON_HIP_H */
