/*
 * ptx.h -- C-ABI drop-in boundary of the MI355X path tracer (libptx.so).
 *
 * Replaces the WebGPU compute path behind the reference's Renderer class
 * (apps/frontend/src/graphics-core/Renderer_TEST.ts; GC/ below = graphics-core/):
 *
 *   ptx_create           <- new Renderer(adapter, device, canvas)          GC/Renderer_TEST.ts:83-126
 *   ptx_upload_scene     <- Initialize(world) -> CreateGPUResources         GC/Renderer_TEST.ts:141-163,445-460
 *                           (takes exactly SerializeWorldData's three u32 arrays, :267-420)
 *   ptx_set_frame        <- Update(): the 33-word uniform block             GC/Renderer_TEST.ts:165-206
 *   ptx_render           <- Render(): G-buffer -> Init -> Final dispatches  GC/Renderer_TEST.ts:208-261
 *                           (+ copyTextureToTexture Result->Scene, :223-231) or the
 *                           legacy brute-force TEST_MCPT dispatch            GC/Renderer.ts:580-647
 *   ptx_reset_accumulation <- texture re-creation on Initialize             GC/Renderer_TEST.ts:445-476
 *   ptx_destroy          <- DestroyGPUResources                             GC/Renderer_TEST.ts:462-476
 *   ptx_run_pass         <- ComputePass.Dispatch of one pass                GC/ComputePass.ts:66-78
 *   ptx_run_passes       <- a run of ComputePass.Dispatch calls (Render, :208-261)
 *   PTX_PASS_TEMPORAL / PTX_PASS_SPATIAL and ptx_halo_* <- the reuse passes the reference
 *                           only specifies (docs/theory/ReSTIR_Pipeline.md:259-462; no code)
 *   PTX_PIPELINE_RESTIR_GI <- BASELINE configs[4], ReSTIR GI: build-defined on the reference's
 *                           shading functions with memo.md:166-231's reconnection shift
 *
 * Conventions: every function returns 0 (PTX_OK) or a negative PTX_E* code and never
 * throws; ptx_last_error() holds the handle's last message.  Input arrays are borrowed
 * for the duration of the call only.  A handle is single-threaded and owns one HIP
 * stream on one device.  Multi-GPU: one handle per rank, each rendering the row band
 * [row_begin, row_end) of the full image with global pixel coordinates (RNG seeds and
 * camera rays use global (x, y), so output is independent of the band split).
 */
#ifndef PTX_H
#define PTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTX_ABI_VERSION 5

#define PTX_OK 0
#define PTX_E_INVALID (-1)  /* bad argument / state                  */
#define PTX_E_HIP (-2)      /* HIP runtime error                     */
#define PTX_E_SCENE (-3)    /* scene arrays inconsistent/unsupported */
#define PTX_E_NOMEM (-4)    /* allocation failure                    */
#define PTX_E_PENDING (-5)  /* ptx_present_poll: the present is still in flight (not an error) */

#define PTX_UNIFORM_WORDS 33
#define PTX_GBUFFER_WORDS 4     /* rgba32 texel: flags|inst|mat, prim, bary.x, bary.y */
#define PTX_RESERVOIR_WORDS 32  /* 128-byte Reservoir, SH/PT_1_InitPass.wgsl:145-185 */

/* pipelines */
#define PTX_PIPELINE_RESTIR 0  /* PT_01 G-buffer -> PT_1 Init -> PT_4 Final (Renderer_TEST) */
#define PTX_PIPELINE_MCPT 1    /* TEST_MCPT brute force (legacy Renderer)                 */
#define PTX_PIPELINE_RESTIR_REUSE 2 /* G-buffer -> Init -> temporal -> spatial -> Final: the
                                       build-defined reuse passes; wavefront
                                       kernels only                                        */
#define PTX_PIPELINE_RESTIR_GI 3    /* G-buffer -> GI init (direct light + 1-bounce indirect
                                       candidate) -> temporal -> spatial -> GI shade, on 64-byte
                                       GI reservoirs; passes keep their
                                       PTX_PASS_* ids (INIT, TEMPORAL, SPATIAL, FINAL)        */

/* passes for ptx_run_pass */
#define PTX_PASS_GBUFFER 0
#define PTX_PASS_INIT 1
#define PTX_PASS_FINAL 2
#define PTX_PASS_MCPT 3
#define PTX_PASS_TRACE 4  /* ptx_trace / ptx_trace_device / ptx_trace_queries (stats slot only) */
#define PTX_PASS_TEMPORAL 8  /* reuse: PT_1 reservoir <- previous frame's output (same pixel) */
#define PTX_PASS_SPATIAL 9   /* reuse: pairwise-MIS resampling over neighbours -> Final's input */
/* stats-only slots: every launch of the wavefront pipeline's kernels, by kind */
#define PTX_STAT_WAVE_TRACE 5  /* trace_queue launches (ray-segment traversal)      */
#define PTX_STAT_WAVE_LOGIC 6  /* start/step launches (shading, RIS, queue appends) */
#define PTX_STAT_FRAME 7       /* whole ptx_render frames of the wavefront ReSTIR path, which
                                  overlaps its passes: slots 0..2 then only get the per-part
                                  G-buffer launches, with PTX_FLAG_TIME_LAUNCHES          */
#define PTX_STAT_PASS_GROUP 10 /* ptx_run_passes calls of the wavefront kernels          */
#define PTX_STAT_FINAL_FUSED 11 /* count only (no time): PT_4 passes of the reuse pipeline that
                                   walked their replays inside their one logic launch
                                   (wfinal_one, or wfinal_replay behind a spatial pass that shaded),
                                   so none of their queries reached trace_queue */
#define PTX_STAT_DENOISE 12  /* launches of the denoiser's kernels (ms with PTX_FLAG_TIME_LAUNCHES) */
#define PTX_STAT_REFIT 13    /* launches of ptx_update_vertices' and ptx_skin_vertices' kernels (ms with
                                PTX_FLAG_TIME_LAUNCHES) */
#define PTX_STAT_BUILD 14    /* launches of ptx_build_blas' kernels, the library's sort as one, and of
                                ptx_rebuild_mesh's and ptx_blas_cost's (ms with PTX_FLAG_TIME_LAUNCHES) */

/* buffers for ptx_read_buffer / ptx_write_buffer / ptx_device_pointer */
#define PTX_BUF_GBUFFER 0    /* band_h * W * 4 u32   */
#define PTX_BUF_RESERVOIR 1  /* band_h * W * 32 u32 (GI pipeline: 16 u32) */
#define PTX_BUF_ACCUM 2      /* band_h * W * 4 f32 (Scene texture: accumulated radiance) */
#define PTX_BUF_COUNTERS 3   /* 32 u64: work counters [0..4] (PTX_FLAG_COUNT builds), diagnostics [8..) */
/* PTX_BUF_COUNTERS word 6, every build: pixels whose history a band could not reproject (past its
 * motion halo of reuse_radius rows; such a pixel has no temporal history); zeroed by ptx_reset_stats */
#define PTX_COUNTER_MOTION_CLIP 6
/* PTX_BUF_COUNTERS word 7, every build: pixels of ptx_denoise_bands' temporal mode with a history
 * candidate inside the image but outside the rows the band's state covers (not taken; see
 * ptx_denoise_bands); zeroed by ptx_reset_stats */
#define PTX_COUNTER_DENOISE_CLIP 7
/* PTX_BUF_COUNTERS word 18 (the next free one: 8..17 are diagnostics), every build: pixels of the
 * reuse pipeline whose spatial output carried no contribution when the spatial pass shaded them
 * itself (a spatial pass directly followed by PTX_PASS_FINAL in one ptx_render / ptx_run_passes
 * sequence), so PT_4 replayed their paths; zeroed by ptx_reset_stats */
#define PTX_COUNTER_REPLAY 18
/* PTX_BUF_COUNTERS word 19, every build: pixels of ptx_upsample_temporal_bands with a history candidate
 * inside the image but outside the rows the band's state covers (not taken; see
 * ptx_upsample_temporal_bands); zeroed by ptx_reset_stats */
#define PTX_COUNTER_UPSAMPLE_CLIP 19
#define PTX_BUF_RESERVOIR_HIST 4 /* band_h * W * 32 u32: spatial output = Final's input and the
                                    next frame's temporal history (reuse pipeline)           */
#define PTX_BUF_DIRECT 5     /* band_h * W * 4 f32: direct light of the GI init pass (GI pipeline) */
#define PTX_BUF_DENOISED 6   /* band_h * W * 4 f32: ptx_denoise's output (read-only; exists after the first call) */
#define PTX_BUF_FRAME_COLOR 7 /* band_h * W * 4 f32 {r, g, b, 1}: the radiance of the frame last rendered alone, what
                                 WriteColor mixed into the accumulation (PTX_FLAG_FRAME_COLOR handles; read-only;
                                 unspecified at pixels without a primary hit, which get the environment colour) */
#define PTX_BUF_DENOISE_HISTORY 8 /* band_h * W * 4 f32 {C.rgb, n}: the temporally integrated colour and the history
                                     length (0..255; 0 = no primary hit) of the last temporal ptx_denoise
                                     (read-only; exists after the first temporal call) */
#define PTX_BUF_UPSAMPLE_HISTORY 9 /* band_h * W * 4 f32 {H.rgb, n}: the colour ptx_upsample_temporal (or its band form)
                                      integrated and the number of own samples in it (0..255) after its last call on
                                      this (full-size) handle (read-only; exists after the first call) */

#define PTX_FLAG_COUNT_WORK 1u     /* count rays / AABB / triangle tests on device (slower)   */
#define PTX_FLAG_SIMPLE_KERNELS 2u   /* A/B: one thread per pixel, no ray exchange            */
#define PTX_FLAGS_RETIRED 12u      /* bits 4, 8: the persistent-lane / tiled-exchange A/B variants
                                      (round 1; both lost to the wavefront kernels, removed):
                                      ptx_create rejects them with PTX_E_INVALID               */
#define PTX_FLAG_TIME_LAUNCHES 16u   /* HIP events around every wavefront launch (stats slots
                                        PTX_STAT_WAVE_*); costs ~5% of frame time            */
#define PTX_FLAG_SINGLE_STREAM 32u   /* run the wavefront passes as one launch sequence (no
                                        two-stream overlap): isolated per-kernel timings     */
#define PTX_FLAG_ROW_CENSUS 64u    /* counting build (implies PTX_FLAG_COUNT_WORK) that also keeps the
                                        work per 8-row tile row of the band, for ptx_row_census;
                                        the totals of PTX_BUF_COUNTERS stay zero              */
#define PTX_FLAG_HALO_OVERLAP 128u /* band frames: the spatial pass of the interior rows runs while
                                        the halo is exchanged, the edge rows after it         */
#define PTX_FLAG_HALO_SKIP 256u    /* a band handle WITHOUT a communicator: ptx_render runs the band
                                        frame exactly as a rank does (pipelined, same launches)
                                        but skips the halo exchange -- the halo rows keep what
                                        they hold, so the edge rows are NOT the split frame's.
                                        Timing only (a band timed alone: bench.py calibration) */
#define PTX_FLAG_FRAME_COLOR 512u  /* keep PTX_BUF_FRAME_COLOR: every WriteColor also stores the frame's own
                                        radiance (one more band_h * W * 16 bytes, counted in device_bytes;
                                        written by the kernels that write the accumulation, in its order).
                                        Accumulation, reservoirs and G-buffer keep their bits.  Needed by
                                        ptx_denoise's temporal mode; any pipeline (TEST_MCPT included)  */
/* no variant flag: the wavefront pipeline (compacted ray queues, one trace round per
   path vertex) -- the default */

typedef struct ptx_config {
    uint32_t width, height;       /* full image size (uniform words 0,1 must match) */
    uint32_t row_begin, row_end;  /* band rendered by this handle; 0,0 = all rows    */
    int32_t device;               /* HIP device ordinal; -1 = current device        */
    uint32_t pipeline;            /* PTX_PIPELINE_*                                  */
    uint32_t flags;               /* PTX_FLAG_*                                      */
    /* reuse pipeline (0 = default): spatial neighbours lie in [-radius, radius]^2 (30),
     * `neighbors` per pixel (3, at most 16), history confidence capped at temporal_cap (20).
     * A band handle keeps min(radius, rows available) halo rows above and below its band. */
    uint32_t reuse_radius, reuse_neighbors, temporal_cap;
    uint32_t reserved[2];
} ptx_config;

typedef struct ptx_stats {
    uint64_t frames;              /* ptx_render calls since the last stats reset    */
    double kernel_ms_total[16];   /* summed device time per PTX_PASS_* / PTX_STAT_* slot */
    uint64_t kernel_launches[16]; /* launches per slot                              */
    uint32_t triangles, bvh_nodes, instances, max_bvh_depth;
    uint64_t device_bytes;        /* device memory held by the handle               */
} ptx_stats;

typedef struct ptx_handle ptx_handle;

int ptx_abi_version(void);
int ptx_create(const ptx_config *cfg, ptx_handle **out);
int ptx_upload_scene(ptx_handle *h, const uint32_t *scene, size_t n_scene, const uint32_t *geometry,
                     size_t n_geometry, const uint32_t *accel, size_t n_accel);
/* Edit instances, materials and lights in place: replace the handle's scene array with one of the
 * same layout (same length, same offsets and counts in the uniform set on the handle, same mesh
 * descriptors); geometry and accel stay.  The array is compared with the handle's, block by block
 * -- instances [0, 33 * n_inst), materials [off_mat, off_light), lights and their CDF
 * [off_light, n_scene) -- and *changed_out (NULL ok) receives the PTX_EDIT_* bits of the blocks
 * that differ; with none the call returns PTX_OK without waiting and without touching the GPU.
 * Otherwise it waits for the frames in flight, uploads the changed words, and
 *   PTX_EDIT_LIGHTS alone    keeps everything: PT_01 reads no light, so the kept G-buffer, the
 *                            surface records and every history stay;
 *   PTX_EDIT_MATERIALS       rebuilds the material table and the root records' transmission word,
 *                            drops the kept G-buffers, surface records and neighbour summaries;
 *   PTX_EDIT_INSTANCES       rebuilds the instance table and the cull bounds (an instance may
 *                            switch to another loaded mesh), the same drops, and ptx_upsample_temporal's
 *                            history (the temporal upsampler does not follow objects unless the
 *                            handle follows: ptx_upsample_follow; the temporal mode of ptx_denoise
 *                            does: below);
 *   a switched mesh          drops the reuse / GI history outright: its reservoirs name triangles and
 *                            sub-meshes of the instance's old mesh;
 *   INSTANCES or MATERIALS   the reuse / GI history serves the next frame only if its camera words
 *                            (uniform 4..22) are those of the frame that wrote it (the ordinary
 *                            same-pixel temporal pass); a moved camera renders that one frame
 *                            without history.  A LIGHTS-only edit never limits the history.
 * After an instance or material edit the G-buffers on the handle are the old tables': ptx_denoise,
 * ptx_upsample and their band and temporal forms are PTX_E_INVALID until a frame or a G-buffer pass
 * has run.  The accumulation is not reset: the caller restarts the frame index as on a camera move.  Band
 * handles and handles with a communicator: every band / rank makes the same call, nothing is exchanged.
 * Refused with scene, tables and histories untouched, so that the next frame is the unedited one (like
 * every error on a handle a refusal drops the kept G-buffers: that frame traces its primary rays
 * again): PTX_E_INVALID -- a null handle or array, no scene or no frame set, another n_scene, a
 * differing word outside the three blocks (the descriptors included); PTX_E_SCENE -- an instance whose
 * mesh word is not a loaded mesh.  A HIP error after the upload has begun leaves the handle without a
 * scene: ptx_upload_scene next. */
#define PTX_EDIT_INSTANCES 1u
#define PTX_EDIT_MATERIALS 2u
#define PTX_EDIT_LIGHTS    4u
int ptx_update_scene(ptx_handle *h, const uint32_t *scene, size_t n_scene, uint32_t *changed_out /* NULL ok */);
/* Deform a loaded mesh in place and refit its BLAS on the GPU: the topology -- index buffer, node order,
 * words 6 and 7 of every node, the sub-BLAS root offsets -- stays, every box follows the vertices.
 * `vertices` holds n_vertices records of 8 words, as the geometry array's (position, normal, uv); they
 * replace records [first_vertex, first_vertex + n_vertices) of mesh `mesh`'s vertex block in the
 * handle's copy of the geometry array and in the device's.  Then, for that mesh only and on the GPU:
 * its triangles are derived again (edge form and vertex / normal records, the expressions of the
 * upload), and its boxes are refitted by the rule of the BLAS builder (pathtracerdemo_amd/scene/bvh.py
 * refit_blas), in f64 rounded to f32 where written:
 *   per triangle   mn, mx = per-axis min / max of the three positions; half = (mx - mn) / 2;
 *                  c = f32(mn + half); h = f32(half + (|mn| + half) * 2^-24);
 *                  lo = f32(f64(c) - f64(h)), hi = f32(f64(c) + f64(h))
 *   a leaf         the per-axis min of lo and max of hi over its triangles
 *   an interior    the union of its two children's boxes
 * so unchanged vertices give the uploaded boxes bit for bit when the uploaded accel array was built by
 * that rule, and the 2^-24 widening keeps every grazing hit.  The host then reads the mesh's root
 * boxes back (32 bytes per sub-mesh, the only readback) and rebuilds the instance table, so the cull
 * boxes of the instances that name the mesh follow it.  Blocking: it waits for the frames in flight first.
 * Kept and dropped as by ptx_update_scene's PTX_EDIT_INSTANCES without a switched mesh: triangle numbers
 * and sub-meshes stay valid, so the reuse / GI history's reservoirs decode; the kept G-buffers, the
 * surface records and the neighbour summaries are dropped; ptx_denoise, ptx_upsample and their band
 * and temporal forms are PTX_E_INVALID until a frame or a G-buffer pass has run; the reuse / GI history
 * serves the next frame only if its camera words are those of the frame that wrote it; the history of
 * ptx_upsample_temporal is dropped, unless the handle follows: ptx_upsample_follow.  The temporal history of ptx_denoise stays and is looked up as for
 * an unchanged instance: it does not follow vertices, so a deformed surface keeps the history of the
 * pixels it covered -- unless the handle's last temporal call asked to follow them
 * (ptx_denoise_params.reserved[2], "Vertex motion" under ptx_denoise): then this call first saves the
 * mesh's triangle records as that call saw them.  The accumulation is not reset.  Band handles and handles with a communicator:
 * every band / rank makes the same call, nothing is exchanged.
 * Refused before the GPU is touched, the next frame being the unedited one: PTX_E_INVALID -- a null
 * handle, a null array with n_vertices > 0, no scene, no frame set or no layout, a range past the
 * mesh's vertex block (it ends at the next larger vertex offset among the descriptors, or at the index
 * block), a position word (0..2 of a record) that is not finite; PTX_E_SCENE -- `mesh` is not a loaded
 * mesh.  n_vertices == 0 is PTX_OK and does nothing.  A HIP error after the upload has begun leaves the
 * handle without a scene: ptx_upload_scene next.
 * The launches (one per triangle pass, one per tree height, one for the roots) count in stats slot
 * PTX_STAT_REFIT, with their time under PTX_FLAG_TIME_LAUNCHES.  Memory: 4 bytes per node pair and 24
 * per triangle of the largest mesh, allocated with the layout and counted in device_bytes. */
int ptx_update_vertices(ptx_handle *h, uint32_t mesh, uint32_t first_vertex, uint32_t n_vertices,
                        const uint32_t *vertices /* n_vertices * 8 words: the geometry array's vertex records */);
/* The accel array as the handle traces it now: the uploaded array with words 0..5 of every node
 * reachable from a sub-mesh root taken from the device's tables.  Before any ptx_update_vertices it is
 * the uploaded array bit for bit, after one the refit -- what a host without a refit of its own keeps
 * to serialise the scene.  Blocking; n_accel must be the uploaded length -- after a ptx_rebuild_mesh the
 * handle's current length (ptx_scene_sizes) -- (PTX_E_INVALID otherwise, and without a scene, a frame or a
 * layout). */
int ptx_read_accel(ptx_handle *h, uint32_t *accel_out, size_t n_accel);
/* Skinning and morph targets on the GPU.  ptx_set_skin binds the bind pose, the joint indices, the
 * weights and the morph deltas of a range of one mesh's vertices into device tables the handle owns
 * (48 bytes per vertex, 12 per vertex and target table, (256 * 12 + 8) * 4 for a call's palette and target
 * weights; counted in device_bytes).  One skin per mesh: a second call replaces it, n_vertices == 0
 * removes it (counts and pointers are not looked at then), ptx_upload_scene drops every skin.  The call
 * launches nothing and changes nothing a frame reads: every history and the kept G-buffers stay.
 * Refused before the GPU is touched: PTX_E_INVALID -- a null handle or descriptor, no scene, no frame
 * set or no layout, a range past the mesh's vertex block, n_joints outside 1..256, n_targets above 8, a
 * joint index >= n_joints, a weight, bind word or delta that is not finite, null joints or weights,
 * target_pos null with targets or non-null without, target_nrm non-null without targets, a non-zero
 * reserved word, a vertex block that does not begin on a 16-byte boundary of the geometry array (the
 * kernel stores 16 bytes at once; the scene compiler's blocks do); PTX_E_SCENE -- `mesh` is not loaded. */
typedef struct ptx_skin_desc {
    uint32_t mesh, first_vertex, n_vertices;  /* the bound range of the mesh's vertex block */
    uint32_t n_joints;                        /* 1..256 */
    uint32_t n_targets;                       /* 0..8 morph targets */
    uint32_t reserved[3];                     /* zero */
    const uint32_t *joints;      /* n_vertices * 4, each < n_joints */
    const float    *weights;     /* n_vertices * 4, finite */
    const float    *bind;        /* n_vertices * 6 {p.xyz, n.xyz}; NULL = words 0..5 of the handle's records now */
    const float    *target_pos;  /* n_targets * n_vertices * 3 position deltas; NULL iff n_targets == 0 */
    const float    *target_nrm;  /* same shape, normal deltas; NULL = normals are not morphed */
} ptx_skin_desc;
int ptx_set_skin(ptx_handle *h, const ptx_skin_desc *d);
/* Pose the skinned range of `mesh` and refit its BLAS.  `palette` holds n_joints affine matrices of 12
 * f32, three rows of four, row-major (M[4r + c]); `target_weights` n_targets f32.  Per bound vertex v,
 * everything in f32, every product and every sum rounded on its own (no fused multiply-add), in
 * exactly this order:
 *   q = p;  m = n                                   (bind position / normal of the vertex)
 *   for k = 0 .. n_targets-1:  q_c = q_c + tw[k] * dP[k][v][c]          (c = x, y, z)
 *                              m_c = m_c + tw[k] * dN[k][v][c]          (only with target_nrm)
 *   B[e]  = ((w0*M[j0][e] + w1*M[j1][e]) + w2*M[j2][e]) + w3*M[j3][e]   (e = 0..11)
 *   P'_r  = ((B[4r]*q.x + B[4r+1]*q.y) + B[4r+2]*q.z) + B[4r+3]         (r = 0..2)
 *   N_r   =  (B[4r]*m.x + B[4r+1]*m.y) + B[4r+2]*m.z
 *   l     = sqrt((N.x*N.x + N.y*N.y) + N.z*N.z);   n' = l > 0 ? N / l : N   (IEEE sqrt and divide)
 * P' and n' replace words 0..5 of the vertex's record in the device's geometry array; words 6 and 7
 * (uv) stay (pathtracerdemo_amd/scene/skin.py skin_vertices is the rule in numpy).  The normal uses the
 * blend's linear part: right for rotations and uniform scales; a non-uniformly scaled joint wants the
 * inverse transpose, which is deliberately not built.  Then the call is ptx_update_vertices from its
 * triangle pass onward: the same refit chain, root-box readback and instance table, the same things
 * kept and dropped, blocking; band handles and ranks each make the same call.  Launches count in
 * PTX_STAT_REFIT: the refit chain plus one.  The handle's host copy of the geometry array is brought up
 * to date from the device (one device-to-host copy per skinned mesh, the accel array's boxes with it)
 * only when a changed layout key in ptx_set_frame derives the layout again; ptx_read_vertices is how a
 * host reads the posed records.  A ptx_update_vertices over a skinned range is legal: it writes records,
 * the bind tables are separate, and the next ptx_skin_vertices overwrites the range.
 * Refused before the GPU is touched, the next frame being the unedited one: what ptx_update_vertices
 * refuses about handle and mesh; PTX_E_INVALID -- a mesh with no skin, a null or non-finite palette,
 * target_weights null or non-finite where targets exist or non-null where there are none, and the
 * overflow bound: with Wmax the largest per-vertex sum of |w|, Pmax the largest |bind word| and Dmax
 * the largest |delta| of the skin, m = max |palette| and T = sum |tw|, the call is refused unless
 * 4 * Wmax * m * (3 * (Pmax + T * Dmax) + 1), evaluated in double, is below 2^96.  Below it every P' is
 * finite by construction, so the kernel needs no flag and no state is ever partially applied. */
int ptx_skin_vertices(ptx_handle *h, uint32_t mesh, const float *palette /* n_joints * 12 */,
                      const float *target_weights /* n_targets; NULL iff n_targets == 0 */);
/* The device's current vertex records [first_vertex, first_vertex + n_vertices) of `mesh`, 8 words
 * each, into records_out.  Blocking; ptx_read_accel's preconditions (PTX_E_INVALID without a scene, a
 * frame or a layout, for a range past the mesh's vertex block and for a null array with n_vertices > 0;
 * PTX_E_SCENE for a mesh that is not loaded). */
int ptx_read_vertices(ptx_handle *h, uint32_t mesh, uint32_t first_vertex, uint32_t n_vertices, uint32_t *records_out);
/* Build a mesh's BLAS on the GPU: an LBVH (Morton codes, a radix sort, a binary radix tree) in the accel
 * array's serialisation -- 32-byte nodes, depth-first, left child = node + 1, leaves as contiguous ranges of a
 * reordered index buffer -- so that the result goes straight into the arrays of ptx_upload_scene, where the
 * host-side SAH builder's went (pathtracerdemo_amd/scene/bvh.py build_blas, js/bvh.js), and refit, skinning
 * and the followers work on it unchanged.  The tree is a pure function of the input
 * (pathtracerdemo_amd/scene/lbvh.py build_blas_lbvh is the same rule in numpy, bit for bit):
 *   inputs         positions (V x 3 f32), indices (3T u32), groups (n_groups x {first_tri, tri_count}: disjoint
 *                  contiguous triangle ranges in ascending order, tri_count >= 1; each gives one root), max_leaf
 *   per triangle   the builder's record, as under ptx_update_vertices: the centre c = f32(mn + half) per axis,
 *                  the box lo = f32(f64(c) - f64(h)), hi = f32(f64(c) + f64(h)); no contraction anywhere
 *   cell numbers   per group, cmin / cmax the per-axis min / max of its triangles' centres; per axis q = 0 where
 *                  cmax == cmin, else q = min(1023, (u32)floor(((f64(c) - f64(cmin)) * 1024.0) / (f64(cmax) -
 *                  f64(cmin)))), every operation rounded on its own in f64 (the sign of a zero in cmin never
 *                  reaches an output)
 *   order          the 30-bit code interleaves the bits of q.x, q.y, q.z, x highest: bit 3k+2 = x's bit k,
 *                  3k+1 = y's, 3k = z's.  A group's triangles are ordered by (code, position in the input index
 *                  buffer), ascending; the reordered index buffer holds their three indices in that order, each
 *                  group in its own range [first_tri, first_tri + tri_count)
 *   tree           with p the sorted position within the group, keys K_p = code_p * 2^32 + p (strictly
 *                  increasing).  node(a, b) covers positions a..b.  If b - a + 1 <= max_leaf it is a leaf: w6 =
 *                  first_tri + a (relative to the mesh's index buffer), w7 = 0xFFFF0000 | count.  Otherwise let
 *                  `bit` be the highest bit in which K_a and K_b differ and s the largest position in [a, b)
 *                  whose key has that bit clear: the children are node(a, s), stored at node + 1, and
 *                  node(s + 1, b), stored behind the whole left subtree; w6 = 8 * (the right child's index from
 *                  the root); w7 is the split axis -- for bit >= 32 with j = bit - 32: 0 if j % 3 == 2, 1 if
 *                  j % 3 == 1, 2 if j % 3 == 0; for bit < 32 (identical codes) 0.  (No consumer reads an
 *                  interior w7 beyond its upper 16 bits being zero.)
 *   boxes          words 0..5 by the refit's rule: a leaf is the per-axis min of lo and max of hi over its
 *                  triangles, an interior node the union of its children (a box word that is a zero may carry
 *                  either sign: min / max over a set holding both zeros is order-dependent)
 *   results        the roots packed in group order into nodes_out, group_nodes_out[g] nodes each; the reordered
 *                  index buffer (triangles in no group are legal: their words are copied through in place);
 *                  the largest depth over all groups (root = 0)
 *   max_leaf       0 = 10, else 1..64 (the device's packed leaf reference holds a count below 128 and a first
 *                  triangle up to 2^24 - 1: T above 2^24 is refused)
 * Blocking, on the handle's stream and device.  Needs no scene and no frame, and reads and writes nothing a
 * frame reads: scene, layout, histories, kept G-buffers and skins are untouched, and frames in flight are not
 * waited for beyond stream order.  Device memory lives for the call only (about 240 bytes per triangle, not
 * counted in device_bytes).  Launches count in stats slot PTX_STAT_BUILD -- the library's sort as one, one per
 * height of the tree in rounds of 24, about 32 for a mesh -- with their time under PTX_FLAG_TIME_LAUNCHES; the
 * host reads one word per group back (the roots' node counts) before the output.
 * Refused with a message before the GPU is touched, PTX_E_INVALID: a null handle, descriptor or array; T = 0
 * or above 2^24; a builder above 1 or a non-zero reserved word; max_leaf above 64; an index >= V; a position
 * that is not finite; groups that overlap, descend, are empty or reach past T; n_node_words below
 * 8 * sum(2 * tri_count - 1).
 *
 * reserved[0] selects the builder: PTX_BLAS_LBVH (0, the tree above) or PTX_BLAS_SAH (1).  PTX_BLAS_SAH builds
 * the host-side SAH builder's tree (pathtracerdemo_amd/scene/bvh.py build_blas: 32 bins, traversal cost 1,
 * triangle cost 1.25) with a STABLE partition in place of its pairwise swaps.  A split is chosen from bin
 * counts and bin boxes, functions of the set of triangles in a node, so every node word and the depth are
 * build_blas'; only the order of the triangles inside a leaf differs.  The tree is a pure function of the input
 * (pathtracerdemo_amd/scene/sah.py build_blas_sah is the same rule in numpy, bit for bit).  Everything is f64
 * from f32 inputs unless it says f32; every operation is rounded on its own, no contraction anywhere:
 *   per triangle   the record above: centre c and half-extent h in f32; tmin = f64(c) - f64(h) and tmax =
 *                  f64(c) + f64(h) stay unrounded f64 (the bin boxes use these, not the f32 lo / hi)
 *   node(lo, hi, depth)  covers positions [lo, hi) of the group's current order, count = hi - lo.  Its box
 *                  (words 0..5) is the f32 rounding of the per-axis min of tmin and max of tmax (= the min of lo
 *                  and the max of hi); cmin / cmax are the per-axis min / max of its centres, f32.  It is a leaf
 *                  if count <= max_leaf or depth >= 40
 *   the split      root_sa = 2 * ((d0*d1 + d1*d2) + d2*d0) on the f64 of the node's f32 box; best = 1.25 * count
 *                  with no axis chosen; then axis a = 0, 1, 2 in that order:
 *                    bin_w = (f64(cmax_a) - f64(cmin_a)) / 32; a triangle's bin is clip(floor((f64(c_a) -
 *                    f64(cmin_a)) / bin_w), 0, 31), or 0 when bin_w is not positive; a bin has a count and a
 *                    3-axis f64 box (min of tmin, max of tmax);
 *                    candidates i = 0..30 ascending: lc = the triangles in bins <= i, rc = count - lc; lp =
 *                    SA(union of bins 0..i) / root_sa if lc > 0 and root_sa > 0, else 0; rp likewise over bins
 *                    i+1..31 and rc; cost = 1.0 + 1.25 * (lp*lc + rp*rc); if cost < best (strict: the first
 *                    minimum wins) take axis a, best = cost, pos = f64(f32((f64(cmin_a) + bin_w) + i * bin_w))
 *                  with no axis chosen the node is a leaf
 *   partition      a triangle goes left iff f64(c_axis) < pos.  This compare and the bin number can disagree
 *                  about a triangle on a bin boundary: n_left is counted by the compare, never taken from the
 *                  bins.  If n_left is 0 or count the node is a leaf.  The order is stable: lefts keep their
 *                  relative order, then rights theirs
 *   children       node(lo, lo + n_left, depth + 1) at node + 1, node(lo + n_left, hi, depth + 1) behind the
 *                  whole left subtree.  Interior words: w6 = 8 * (the right child's index from the root), w7 =
 *                  axis.  Leaf words: w6 = the leaf's first position in the mesh's index buffer, w7 = 0xFFFF0000
 *                  | count
 *   final order    inside a leaf the triangles are in input order; leaves lie in depth-first order
 *   zeros          the sign of a zero never reaches a decision; a box word that is a zero may carry either sign
 * max_leaf means what it means to build_blas: a node of at most max_leaf triangles is never split.  A leaf may
 * be LARGER than max_leaf where the SAH prefers it or no split exists (identical centres); ptx_upload_scene
 * keeps refusing a leaf past its packed reference.  A leaf of more than 65 535 triangles cannot be serialised:
 * PTX_E_SCENE with a message, outputs unspecified.  Device memory lives for the call only: about 230 bytes per
 * triangle (36 per triangle for records and orders, 84 per node of up to 2 T - 1 for tables and output, 24 for
 * the two index buffers) and 12 per vertex; an arena that cannot be allocated is PTX_E_NOMEM before any launch.  Launches
 * count in PTX_STAT_BUILD: one per depth going down (the host reads two words back after each to size the
 * next; 41 bound the loop), one per depth coming up, and three more. */
#define PTX_BLAS_LBVH 0u
#define PTX_BLAS_SAH  1u
typedef struct ptx_blas_desc {
    const float    *positions;  uint32_t n_vertices;   /* V x 3 f32, finite */
    const uint32_t *indices;    uint32_t n_tris;       /* 3T, each < V */
    const uint32_t *groups;     uint32_t n_groups;     /* {first_tri, tri_count} pairs */
    uint32_t max_leaf;          uint32_t reserved[3];  /* [0]: PTX_BLAS_LBVH or PTX_BLAS_SAH; [1], [2]: zero */
} ptx_blas_desc;
int ptx_build_blas(ptx_handle *h, const ptx_blas_desc *d,
                   uint32_t *nodes_out, size_t n_node_words,   /* >= 8 * sum(2*tri_count - 1) */
                   uint32_t *indices_out,                       /* 3T */
                   uint32_t *group_nodes_out,                   /* n_groups: nodes per root, packed in order */
                   uint32_t *max_depth_out);
/* Rebuild a loaded mesh's BLAS in place.  A refit (ptx_update_vertices, ptx_skin_vertices) keeps the topology,
 * so a mesh posed far from the shape it was built for is traced through that shape's tree with inflated
 * boxes; this call builds the tree again from the shape the device holds now and puts it into the handle
 * without an upload (pathtracerdemo_amd/scene/world.py rebuild_mesh is the same rule in numpy):
 *   positions      words 0..2 of the mesh's vertex records on the device -- what the vertex calls left there,
 *                  finite by their own guarantees
 *   indices        the mesh's index block on the device (it ends at the next larger index offset among the
 *                  descriptors, or at the sub-root block)
 *   groups         one per sub-mesh root, from the handle's accel copy: first = the smallest w6 of the leaves
 *                  reachable from the root, end = the largest w6 + count (world.py mesh_groups)
 *   tree           ptx_build_blas' for `builder` (PTX_BLAS_LBVH or PTX_BLAS_SAH) and max_leaf (0 = 10, else
 *                  1..64), by the same kernels; a box word that is a zero may carry either sign, as there
 *   splice         the roots, concatenated in group order, replace the mesh's block of the accel array (from
 *                  offset blas + d[4] to the next larger block start or the array's end); later blocks shift and
 *                  word 4 of every descriptor whose block lay behind moves by the difference; the mesh's sub-root
 *                  words become the running sum of its roots' lengths (in words); its index block becomes the
 *                  reordered indices.  Vertex records, every other scene word and the uniform's offsets stay
 * Blocking.  The call waits for frames in flight, brings the handle's host copies up to date with the device
 * (posed vertex blocks, refitted boxes), validates, builds on the handle's stream, reads nodes and indices
 * back as ptx_build_blas does, validates the tree, and only then commits: it splices the handle's copies,
 * uploads the changed descriptor words, the index block and the sub-root words, and derives the layout again.
 * Everything that can be refused is refused before the commit, the next frame being the unedited one:
 * PTX_E_INVALID -- a null handle, no scene, no frame set or no layout, a builder above 1, max_leaf above 64;
 * PTX_E_SCENE -- `mesh` is not a loaded mesh, roots whose leaf ranges do not ascend, overlap, reach past the
 * index block or do not tile their range, an index at or past the mesh's vertex count, a BLAS, index or
 * sub-root block shared with another descriptor, a built leaf of more than 127 triangles (PTX_BLAS_SAH makes
 * one where no split exists; the layout's packed reference holds 127), a depth whose traversal stack would
 * not fit LDS.  A HIP error after the commit began leaves the handle without a scene: ptx_upload_scene next.
 * Kept: the vertex records and every skin (ptx_skin_vertices works right after, with no ptx_set_skin), the
 * accumulation (not reset), the temporal denoiser's history (keyed by instance and sub-mesh; the instance
 * block is unchanged).  Dropped: the kept G-buffers, surface records, neighbour summaries and init state, so
 * ptx_denoise / ptx_upsample* are PTX_E_INVALID until a frame has run; the reuse / GI history outright, as for
 * a switched mesh under ptx_update_scene (its reservoirs name triangle numbers, and the index buffer was
 * reordered); ptx_upsample_temporal's history unless the handle follows (ptx_upsample_follow), then the edit
 * is pending.  A rebuild is a derivation of the layout: a mesh marked as deformed gets flag 2 for one call of
 * either follower ("layout derived again", ptx_denoise "Vertex motion"), because a snapshot in the old
 * triangle numbering must never be read with new numbers.  Band handles, ranks and paired hi / lo handles
 * each make the same call; the tree is a pure function of the input, so they agree.
 * Launches count in PTX_STAT_BUILD: the builder's, plus one (the positions).  The builder's arena lives for
 * the call only; the handle's tables change size with the node count (64 B + 4 B per pair). */
typedef struct ptx_rebuild_info {
    uint32_t n_accel;        /* the accel array's length now */
    uint32_t mesh_nodes;     /* nodes of the mesh's roots together */
    uint32_t max_depth;      /* of the mesh's new roots */
    uint32_t scene_words;    /* scene words that changed (descriptor word 4 of later meshes) */
    uint32_t reserved[4];
} ptx_rebuild_info;
int ptx_rebuild_mesh(ptx_handle *h, uint32_t mesh, uint32_t builder /* PTX_BLAS_LBVH | PTX_BLAS_SAH */,
                     uint32_t max_leaf /* 0 = 10, else 1..64 */, ptx_rebuild_info *info_out /* NULL ok */);
/* The lengths of the handle's three arrays now (a rebuild changes the accel array's); a NULL pointer is
 * skipped.  PTX_E_INVALID without a handle or a scene. */
int ptx_scene_sizes(ptx_handle *h, size_t *n_scene, size_t *n_geometry, size_t *n_accel);
/* The three arrays as the handle renders them now: scene -- the handle's copy (edits and shifted descriptors
 * included); geometry -- with every posed vertex block read from the device; accel -- as ptx_read_accel
 * returns it.  Blocking.  Each length must be ptx_scene_sizes' (PTX_E_INVALID otherwise, and without a scene,
 * a frame or a layout); a NULL array with length 0 is skipped. */
int ptx_read_scene(ptx_handle *h, uint32_t *scene_out, size_t n_scene, uint32_t *geometry_out, size_t n_geometry,
                   uint32_t *accel_out, size_t n_accel);   /* a NULL array with length 0 is skipped */
/* The surface-area cost of a mesh's trees as the device holds them now (after refits), summed over its roots
 * -- the number that tells a host when a rebuild pays (pathtracerdemo_amd/scene/lbvh.py sah_cost, traversal 1,
 * triangle 1.25).  Everything is f64 from the tables' f32 boxes, every operation rounded on its own, no
 * contraction: d = f64(hi) - f64(lo); area = 2.0 * ((d.x*d.y + d.y*d.z) + d.z*d.x); rel = area / area_root
 * where area_root > 0, else 0; a root or child that is interior adds rel, a leaf (rel * 1.25) * count.
 * Deterministic: a workgroup adds its terms in a fixed order (shuffles, then LDS) and writes one partial, the
 * host adds the partials in index order, nothing is atomic -- two calls on the same tables return the same
 * bits; against another summation order the result differs by rounding (at most nodes * 2^-52 relative).
 * Blocking; reads nothing a frame writes and changes nothing.  One launch, counted in PTX_STAT_BUILD; 8 bytes
 * per workgroup for the call, and 4 bytes per node pair (each pair's sub-mesh) uploaded with the layout and
 * counted in device_bytes.  Refusals are ptx_read_vertices', plus a null cost_out (PTX_E_INVALID). */
int ptx_blas_cost(ptx_handle *h, uint32_t mesh, double *cost_out);
int ptx_set_frame(ptx_handle *h, const uint32_t uniform[PTX_UNIFORM_WORDS]);
/* Run the configured pipeline for the current frame; if rgba_out != NULL copy the band's
 * accumulated RGBA f32 image (band_h * W * 4) into it (blocking). Otherwise asynchronous.
 * While camera (uniform words 0, 1, 4..22), layout key, band and scene are the ones a frame
 * context's G-buffer was traced for, a frame keeps that G-buffer instead of tracing the primary
 * rays again (same bits: PT_01 reads no frame word); ptx_run_pass / ptx_run_passes always run
 * the G-buffer pass they are given. */
int ptx_render(ptx_handle *h, float *rgba_out);
/* (reuse pipeline: whole-image handles only -- a band needs the halo exchange between its
 *  passes, see ptx_halo_*) */
int ptx_run_pass(ptx_handle *h, int pass);
/* Passes in order as one launch sequence per segment group (overlapped on two streams).
 * Every pass must read only its own pixel's results of the earlier passes, except that
 * PTX_PASS_SPATIAL may come first (it reads neighbours of the previous passes' output). */
int ptx_run_passes(ptx_handle *h, const int *passes, int n);
/* Spatial-reuse halo of a band handle.  Between TEMPORAL and SPATIAL a band needs the
 * G-buffer and reservoir rows of its neighbours: rows_top rows from the band above (its
 * last rows), rows_bottom from the band below.  A message is rows x W x bytes_per_row
 * (G-buffer rows, then reservoir rows).  pack copies THIS band's first rows_top / last
 * rows_bottom rows (what the neighbours need) into device buffers; unpack copies received
 * messages into the halo rows.  Both are async on the handle's stream; the buffers may be
 * device memory (RCCL) or host memory (then synchronize before reading a packed one). */
int ptx_halo_rows(ptx_handle *h, uint32_t *rows_top, uint32_t *rows_bottom, size_t *bytes_per_row);
int ptx_halo_pack(ptx_handle *h, void *dev_top, void *dev_bottom);
int ptx_halo_unpack(ptx_handle *h, const void *dev_top, const void *dev_bottom);
/* ---- multi-GPU: the frame split into row bands, one handle per band.
 * The one exchange is the spatial-reuse halo: between the temporal and spatial passes a band
 * receives the G-buffer + reservoir rows of its neighbours (rows_top from the band above,
 * rows_bottom from the band below; ptx_halo_rows).  The handle owns the RCCL communicator:
 *   ptx_comm_unique_id  <- ncclGetUniqueId on one rank; the caller ships the 128 bytes to the
 *                          others (e.g. a torch.distributed broadcast)
 *   ptx_comm_init       <- ncclCommInitRank for a band handle: rank r is the band above rank
 *                          r + 1; ptx_render then runs the whole frame, halo included
 *                          (grouped ncclSend / ncclRecv from the band's edge rows straight into
 *                          the neighbours' halo rows on the handle's streams, no host wait)
 *   ptx_comm_init_all   <- ncclCommInitAll: every band handle of ONE process (one per GPU)
 *   ptx_render_bands    <- one frame over n band handles of one process, in band order
 *                          (row_end of band i == row_begin of band i + 1): the halo moves over
 *                          their communicators, or by peer copies when they have none (several
 *                          bands may then share a GPU); rgba_out (optional) receives the bands'
 *                          accumulated rows in order (blocking)
 * Seeds and neighbour offsets use global pixel coordinates: any split renders the single
 * handle's frame bit for bit. */
#define PTX_COMM_ID_BYTES 128
int ptx_comm_unique_id(void *id_out, size_t bytes);
int ptx_comm_init(ptx_handle *h, const void *unique_id, size_t bytes, int rank, int world);
int ptx_comm_init_all(ptx_handle *const *handles, int n);
int ptx_render_bands(ptx_handle *const *handles, int n, float *rgba_out);
/* The communicator a band handle owns: its rank and world size (0 / 1 without one) and the
 * halo bytes it has sent so far -- what a benchmark reports to prove N ranks exchanged.
 * ptx_comm_init also swaps the band geometry with the neighbouring ranks once and fails on
 * rows that do not continue or halos that do not match; ptx_render checks the communicator's
 * asynchronous error state (ncclCommGetAsyncError) every frame. */
int ptx_comm_info(ptx_handle *h, int *rank, int *world, uint64_t *halo_bytes_sent);
/* Work census of a PTX_FLAG_ROW_CENSUS handle since the last ptx_reset_stats: per 8-row tile
 * row of the band, 5 u64 {rays, instance transforms, AABB tests, triangle tests, hits} of every
 * query traced for that row's pixels (the §8(d) algorithmic-bytes counters).  Cost-balanced
 * band boundaries come from it (pathtracerdemo_amd/bands.py). */
int ptx_row_census(ptx_handle *h, uint64_t *tile_row_counts, size_t n_tile_rows);
int ptx_reset_accumulation(ptx_handle *h);
int ptx_synchronize(ptx_handle *h);
int ptx_get_stats(ptx_handle *h, ptx_stats *out);
int ptx_reset_stats(ptx_handle *h);
int ptx_read_buffer(ptx_handle *h, int which, void *host_dst, size_t bytes);
/* A G-buffer written by the host is overwritten by the next frame on that frame context exactly
 * as before (the write drops the kept G-buffer); an unchanged camera alone no longer re-traces it. */
int ptx_write_buffer(ptx_handle *h, int which, const void *host_src, size_t bytes);
/* A buffer's device address.  On a handle whose frames are pipelined (whole-image reuse
 * pipeline on its own stream: two frames in flight) the G-buffer and
 * reservoir buffers alternate between two allocations frame by frame: the pointer returned
 * for PTX_BUF_GBUFFER / PTX_BUF_RESERVOIR is valid until the next ptx_render.  Accumulation,
 * history and counters never move.  After the G-buffer's pointer was handed out the handle
 * traces the G-buffer every frame again (the caller may write it at any time). */
int ptx_device_pointer(ptx_handle *h, int which, void **dev_ptr, size_t *bytes);
/* The reference's render pass (Renderer_TEST.Render, GC/Renderer_TEST.ts:233-255: a fullscreen
 * quad, SH/VertexShader.wgsl + SH/FragmentShader.wgsl:7-10) onto a canvas_w x canvas_h canvas:
 * canvas pixel (x, y), y = 0 the top row, shows texel (floor((2x+1)*600 / 2canvas_w),
 * floor((2canvas_h-2y-1)*450 / 2canvas_h)) of the accumulated image -- the shader's fixed
 * 600 x 450 window, flipped to screen order -- as unorm8 rgb (clamp, round to nearest even) with
 * alpha 255; a texel outside the image reads 0.  out: canvas_w * canvas_h * 4 bytes, RGBA
 * (bgra = 0, a 2D canvas's ImageData) or BGRA (bgra = 1, a bgra8unorm WebGPU canvas); blocking.
 * Whole-image handles (a split frame is presented from its gathered rows by the host). */
int ptx_present(ptx_handle *h, uint32_t canvas_w, uint32_t canvas_h, int bgra, uint8_t *out);
/* The same render pass without blocking the caller (the reference's Render() ends by drawing into
 * the canvas, GC/Renderer_TEST.ts:233-258, and WebGPUEngine's loop calls nothing else,
 * GC/service/WebGPUEngine.ts:199-200): ptx_present_async enqueues it for the frame last rendered,
 * with the copy into handle-owned pinned memory, on the handle's stream, and returns at once;
 * ptx_present_poll copies the bytes into `out` (canvas_w * canvas_h * 4) and returns PTX_OK once
 * that copy has landed, PTX_E_PENDING while it is in flight (hipEventQuery: never waits).  One
 * present may be in flight per handle (a second ptx_present_async before its poll returned
 * PTX_OK fails).  A later frame's accumulation waits for it on the GPU, so the bytes are exactly
 * the frame it was enqueued after. */
int ptx_present_async(ptx_handle *h, uint32_t canvas_w, uint32_t canvas_h, int bgra);
int ptx_present_poll(ptx_handle *h, uint8_t *out, size_t bytes);
/* The edge-avoiding a-trous wavelet filter of the accumulated image (Denoiser): guided
 * by the primary hit of the current frame context's G-buffer (same instance and sub-mesh, normal,
 * plane distance), luminance variance estimated from the image itself, so it fades as the image
 * converges.  Asynchronous: enqueued on the handle's stream behind the frame last rendered, exactly
 * where ptx_present_async enqueues (a pipelined handle's next frame accumulates after it).  Reads
 * the accumulation and the G-buffer; writes only its own buffers (allocated by the first call,
 * counted in device_bytes): PTX_BUF_DENOISED holds rgb after the last iteration, alpha 1; a pixel
 * without a primary hit keeps its colour.  The camera position is the one of the uniform set on
 * the handle: call it before the next frame's ptx_set_frame.  Whole-image handles of the pipelines with a G-buffer
 * after at least one frame (a frame split into bands: ptx_denoise_bands); anything else, or a parameter out of range, is PTX_E_INVALID.
 * Launches (PTX_STAT_DENOISE): 2 + iterations (guide records, variance, the iterations).
 *
 * Temporal mode (reserved[0] = 1; PTX_FLAG_FRAME_COLOR handles, PTX_E_INVALID otherwise, before the
 * GPU is touched): the filter's input is not the accumulation but the frame colours integrated over
 * the calls, carried across camera moves.  The handle keeps, from the previous temporal call, its
 * guide records, its uniform words 4..22 with their VP (the inverse of words 4..19), and per pixel
 * the integrated colour C, the luminance moments m1, m2 and the history length n (80 bytes per pixel
 * beside the spatial filter's 64, allocated by the first temporal call, counted in device_bytes).
 * A pixel with a primary hit looks its history up at itself when words 4..22 are that call's bit
 * for bit, else at the four pixels around its hit point's projection through that VP (bilinear
 * weights); a tap counts when it lies inside the image with the same instance and sub-mesh, n >= 1,
 * normals within dot >= 0.9 and within the plane distance r.  With history n = min(n_h + 1, 255),
 * alpha = max(1 / n, alpha_min) and C, m1, m2 move towards the frame's colour and luminance moments by
 * alpha; without, they start from them with n = 1.  The variance is max(0, m2 - m1^2) where n >= 4,
 * the spatial estimate on C elsewhere; the iterations then run unchanged on (C, variance) into
 * PTX_BUF_DENOISED, and (C, m1, m2, n) -- not the filtered image -- is the next call's history
 * (C and n: PTX_BUF_DENOISE_HISTORY).  A pixel without a primary hit keeps its accumulated colour,
 * n = 0.  ptx_upload_scene and ptx_reset_accumulation drop the history; ptx_set_frame and the frame
 * index never do (the engine's ResetFrameCount on a camera move keeps it); a call with reserved[0] = 0
 * is the spatial filter exactly and neither reads nor writes the state.
 *   Object motion: every temporal call also keeps the instance block of the scene array (33 words per
 * instance).  While no instance differs from the previous call's, bit for bit, the call is the one
 * above.  Otherwise (ptx_update_scene with PTX_EDIT_INSTANCES in between) every instance gets
 * D = M_prev * Minv_cur (words 0..15 of the kept block times words 16..31 of the current one, in
 * double, each element summed in k = 0..3 order and rounded once to f32) and a flag: 0 unchanged; 1
 * moved rigidly -- both matrices' bottom rows exactly (0, 0, 0, 1), every element finite, the same mesh
 * word, and max |L^T L - I| <= 1e-3 for D's upper 3x3 L; 2 anything else (a changed scale, another
 * mesh).  A pixel with a primary hit of instance i (its key >> 16): flag 0 as above; flag 2 no lookup,
 * it starts from the frame's colour with n = 1; flag 1 Q = D P and Nq = D N (the linear part, not
 * renormalised) are where its point and normal were, Q is reprojected through the previous call's VP
 * whether or not the camera words changed, taps and weights as above, and a tap is tested against
 * Nq (dot >= 0.9) and Q (|dot(Nq, P' - Q)| <= this pixel's r).
 *   Vertex motion (reserved[2] = 1, "follow vertices"; opt-in: with 0 every call is the one above, bit for
 * bit).  Tracking: a temporal call with reserved[2] = 1 that is enqueued completely leaves the handle
 * tracking, one with reserved[2] = 0 not tracking; reserved[2] > 1 is PTX_E_INVALID before the GPU is
 * touched; reserved[2] = 1 without the temporal mode is ignored, as reserved[1] is.  Snapshot: while a
 * handle is tracking and holds a temporal state, the first ptx_update_vertices / ptx_skin_vertices on a
 * mesh since that call saves the mesh's triangle records (the 80 bytes per triangle the refit rewrites:
 * three positions and normals) before the refit overwrites them -- a device-to-device copy on the call's
 * stream, no launch, PTX_STAT_REFIT counts what it counted -- and marks the mesh deformed; later updates
 * of the mesh before the next temporal call save nothing, so the snapshot is the shape the previous
 * temporal call saw.  The buffer (80 bytes per triangle of the scene) is allocated by the first call with
 * reserved[2] = 1 and counted in device_bytes.  At the next temporal call with reserved[2] = 1 every
 * instance whose mesh word equals the previous call's and whose mesh is marked gets flag 3, whatever
 * happened to its matrices (no rigidity is needed: a rescaled instance follows too); a switched mesh
 * stays flag 2; instances of meshes not marked keep flags 0 / 1 / 2 as above; then the marks are cleared
 * (a call with reserved[2] = 0 clears them unused and is the call above).  A pixel with a primary hit of
 * a flag-3 instance: Q and Nq are GetSurface's position and normalised normal of the pixel's current
 * G-buffer texel (instance, triangle, barycentrics) evaluated on the snapshot's triangle record under the
 * previous call's instance matrices (words 0..15 and 16..31 of the kept block) -- the surface point where
 * it was at that call; Q is always reprojected through that call's VP, as for flag 1, and taps, weights,
 * the n' >= 1, key, normal and plane tests (this pixel's r), the integration and a band's clip count are
 * unchanged.  With no mesh marked, a call with reserved[2] = 1 runs the kernels and gives the bits of the
 * same call with reserved[2] = 0.  ptx_upload_scene, ptx_reset_accumulation and everything else that drops
 * the temporal state drop the marks with it; a layout derived again by ptx_set_frame between two calls
 * moves the records, so the marked meshes' instances get flag 2 for that one call.  ptx_upsample_temporal
 * does not follow vertices and keeps dropping its history on a vertex update, unless the handle follows:
 * ptx_upsample_follow.
 * Launches: 3 + iterations (guide records, dn_temporal, variance, the iterations), following or not. */
typedef struct ptx_denoise_params {
    uint32_t iterations;      /* 1..6 (step 2^i in iteration i); 0 = default 5 */
    float sigma_lum;          /* luminance edge stop, in standard deviations; 0 = default 4 */
    float sigma_plane;        /* plane-distance edge stop, as a fraction of the distance to the camera; 0 = default 0.02 */
    uint32_t reserved[5];     /* [0] temporal: 0 = off, 1 = on; [1] alpha_min, the bit pattern of an f32: 0 = default
                                 0.05, else finite and in (0, 1] (read in temporal mode only); [2] follow vertices:
                                 0 = off, 1 = on (used in temporal mode only); [3..4] zero */
} ptx_denoise_params;
int ptx_denoise(ptx_handle *h, const ptx_denoise_params *p /* NULL = defaults */);
/* The same filter on a frame split into row bands.  handles: band handles in band order that cover
 * the image's rows (ptx_render_bands' continuity rules), each after at least one frame; or one
 * whole-image handle (n = 1: exactly ptx_denoise); or, n = 1 with a handle whose communicator has
 * world > 1, this rank's band of a frame every rank makes the call for (the neighbours' rows as
 * ptx_comm_init exchanged them).  Either every handle owns a communicator (the halo moves by one
 * group of sends / receives over them, counted in halo_bytes_sent) or none (peer copies; several
 * bands may share a GPU).  ptx_denoise itself keeps refusing band handles.
 *   A band filters the WINDOW of its rows [b0, b1) and min(R, rows available) rows above and below,
 * R = 2^(iterations + 1) (64 at the default 5, 128 at 6), as if the window were the whole image (rows
 * of the window outside the image: taps skipped, as ever).  With R halo rows the band's rows of the
 * result are the whole-image filter's bit for bit, with R - 1 they are not: the colour after k
 * iterations reaches r_k rows, the variance s_k, r_0 = 0, s_0 = 3, r_(k+1) = max(r_k + 2^(k+1),
 * s_k + 1), s_(k+1) = max(r_k, s_k) + 2^(k+1), so r_n = 2^(n+1).  One exchange per call brings, per
 * halo pixel, the neighbour's G-buffer texel (16 B) and accumulated colour (16 B), straight from its
 * buffers; with more than one band, a band of fewer than R rows is PTX_E_INVALID (the message names
 * the band and the rows needed), as are bands that differ in size or pipeline, a gap, TEST_MCPT, a
 * band that has not rendered, parameters out of ptx_denoise's ranges and temporal mode without
 * PTX_FLAG_FRAME_COLOR on every band -- all before any GPU work.
 *   Each band's PTX_BUF_DENOISED (temporal mode: and PTX_BUF_DENOISE_HISTORY) holds its own band_h
 * rows; the buffers (with room for 128 halo rows on either side) are allocated by the first call and
 * counted in device_bytes, launches count in PTX_STAT_DENOISE.  Asynchronous on each band's stream
 * behind the frame last rendered; a band's next frame waits on the GPU until its neighbours have
 * copied its rows.  Accumulation, reservoirs, history and G-buffer keep their bits.
 *   Temporal mode: each band runs the guide kernel and the history integration on its own rows; the
 * halo then carries the texel, {C, n} (16 B) and {m1, m2} (8 B); guides of the halo rows are
 * recomputed from the texels, the variance pass and the iterations run on the window, and what was
 * received becomes the state's halo rows: the band's state covers its window, for this call's filter
 * and the next call's history lookups.  In that next call a candidate tap inside the image but
 * outside the rows the state covers is not taken -- as if n' = 0 there -- and a pixel with at least
 * one such candidate adds 1 to PTX_COUNTER_DENOISE_CLIP on its band (the same-pixel rule never
 * clips).  So with the counter 0 on every band the split equals the whole-image handle bit for bit,
 * and in general a band's new {C, m1, m2, n} on its own rows is the whole-image definition with the
 * previous state's n' zeroed outside that band's window.  ptx_upload_scene and
 * ptx_reset_accumulation drop a band's state as ever; it then starts without history, and its
 * neighbours see n = 1 (n = 0 at misses) in the rows it sends.  reserved[2] (follow vertices) goes to every
 * band: each tracks, saves and marks for itself, since every band makes the same vertex calls. */
int ptx_denoise_bands(ptx_handle *const *handles, int n, const ptx_denoise_params *p /* NULL = defaults */);
/* Guided upsampling (Upsampling): the denoised image of `lo`, a whole-image handle of
 * w x h after at least one ptx_denoise (spatial or temporal), written at the size W x H = s*w x s*h
 * (one integer s in 2, 3, 4) of the whole-image handle `hi` into hi's PTX_BUF_DENOISED, alpha 1,
 * steered by hi's primary hits.  Primary rays are unjittered pixel centres, so lo's pixel (i, j)
 * looks through hi's image at (s*i + (s-1)/2, s*j + (s-1)/2).  The call traces nothing: it turns the
 * G-buffer of hi's current frame context, as it stands (a host-written one is honoured), into guide
 * records with sigma_plane and reads lo's output and the guide records of lo's last ptx_denoise.
 * hi pixel (x, y) sits at fx = (x + 0.5) / s - 0.5, x0 = floor(fx), ax = fx - x0 (y likewise) of lo:
 *   stage 1  the pixels (x0 + i, y0 + j), i, j in 0, 1 (j outer), inside lo's image with hi's key
 *            (instance and sub-mesh, or both without a primary hit), weighted by the bilinear weight
 *            times the denoiser's guide weight (1 at a pixel without a hit): sum(wt * c) / sum(wt)
 *            when sum(wt) > 0;
 *   stage 2  else the plain average of the pixels (x0 - 1 + i, y0 - 1 + j), i, j in 0..3, inside the
 *            image with that key, when there is one;
 *   stage 3  else lo's pixel (x / s, y / s).
 * Both handles: same device, pipelines with a G-buffer, uniform words 4..22 equal bit for bit, and
 * equal triangles, bvh_nodes and instances (ptx_stats) -- the cheap guard for "the same scene", the
 * rest of which is the caller's contract; hi has a scene and at least one G-buffer pass or frame
 * since its upload.  Anything else (a null handle, hi == lo, a band handle, TEST_MCPT, no denoised
 * image on lo, sizes that are no such multiple, a sigma_plane that is negative or not finite, a
 * non-zero reserved word) is PTX_E_INVALID with the reason in hi's ptx_last_error, before any GPU work.
 *   Asynchronous on hi's stream: it first waits for the tail of the stream lo's last denoise ran on,
 * and lo's next GPU work (a frame, denoise, reset, upload or destroy, on whichever of lo's streams
 * it runs) waits on the GPU until hi's kernels have read lo's buffers.  lo's accumulation, G-buffer, reservoirs, denoiser state and output
 * and hi's G-buffer keep their bits.  hi's buffers (32 B guide record + 16 B output per pixel) are
 * allocated by the first call and counted in device_bytes; PTX_BUF_DENOISED and
 * ptx_present_source(hi, PTX_BUF_DENOISED) then work on hi as after a first ptx_denoise.
 * Launches (hi's PTX_STAT_DENOISE): 2 (guide records, dn_upsample). */
typedef struct ptx_upsample_params {
    float sigma_plane;     /* plane-distance edge stop of the full-size guides; 0 = default 0.02 */
    uint32_t reserved[7];  /* zero */
} ptx_upsample_params;     /* 32 bytes */
int ptx_upsample(ptx_handle *hi, ptx_handle *lo, const ptx_upsample_params *p /* NULL = defaults */);
/* ptx_upsample for a frame split into row bands (Upsampling, Bands): n pairs in band
 * order, lo[i] a band [b0, b1) of the w x h frame after ptx_denoise_bands, hi[i] the band
 * [s*b0, s*b1) of the s*w x s*h frame on the same device (several pairs may share a GPU); every
 * hi[i]'s rows of the result equal the whole-image ptx_upsample's bit for bit.  The forms are
 * ptx_denoise_bands': n pairs of one process whose lo bands continue one another and cover the frame;
 * n = 1 with two whole-image handles (exactly ptx_upsample(hi[0], lo[0], p)); or, n = 1 with a lo[0]
 * whose communicator has world > 1, this rank's pair of a frame every rank makes the call for.
 *   Full-size row y reads small rows y0 - 1 .. y0 + 2, y0 = floor((y + 0.5) / s - 0.5): b0 - 2 for
 * y = s*b0, b1 + 1 for y = s*b1 - 1.  So one exchange per call brings each pair the last 2 own rows of
 * the lo band above and the first 2 of the lo band below: their PTX_BUF_DENOISED, 16 B per pixel, into
 * a buffer hi[i] owns (allocated by the first call, counted in device_bytes).  Either every lo owns a
 * communicator (one group of sends / receives over them, counted in lo's halo_bytes_sent) or none
 * (peer copies).  The guide records of those rows are not sent: they are the ones lo[i]'s last
 * ptx_denoise_bands left in its window (its halo is at least 4 rows).  All positions (x0, ax, y0, ay,
 * stage 3's y / s) are the frame's.
 *   Per pair ptx_upsample's preconditions hold (pipelines with a G-buffer, uniform words 4..22 and
 * triangles, bvh_nodes, instances equal, hi[i] with a scene and a G-buffer pass or frame since its
 * upload, lo[i] with a denoised image).  PTX_E_INVALID with the reason in hi[0]'s ptx_last_error,
 * before any GPU work: a null array or handle, n outside 1..64, a handle that appears twice, hi rows
 * that are not s times lo's, a pair on two devices, pairs that differ in size or pipeline, a gap
 * between bands or bands that do not cover the image (not in the rank form), a mix of bands with and
 * without communicators, with more than one band a lo band of fewer than 2 rows, TEST_MCPT, a lo band
 * without a denoised image (or whose last call was not ptx_denoise_bands), an hi band without a
 * G-buffer, cameras or scenes that differ, a sigma_plane that is negative or not finite, a non-zero
 * reserved word.  ptx_upsample itself keeps refusing band handles.
 *   hi[i]'s PTX_BUF_DENOISED holds its own band_h rows, alpha 1 (its buffers are laid out as a first
 * ptx_denoise_bands lays them out); launches (hi[i]'s PTX_STAT_DENOISE): 2 per band.  Asynchronous:
 * hi[i]'s stream waits for the tail of lo[i]'s last denoise and for its neighbours' rows; every
 * stream lo[i]'s next GPU work can run on waits until hi[i]'s kernels have read it and the
 * neighbouring pairs have copied its rows.  lo's accumulation, G-buffer, reservoirs, denoiser state
 * and output and hi's G-buffer keep their bits. */
int ptx_upsample_bands(ptx_handle *const *hi, ptx_handle *const *lo, int n,
                       const ptx_upsample_params *p /* NULL = defaults */);
/* Temporal upsampling (Temporal upsampling): super-resolution from small frames whose
 * sample positions cycle through the s x s full-size pixels of every block.
 *   ptx_phase_uniform (host arithmetic only: no handle, no GPU) makes the uniform of the W/s x H/s frame
 * whose pixel (i, j) looks through pixel (s*i + px, s*j + py) of hi_uniform's W x H frame: words 0, 1
 * become W/s, H/s, the translation column t of the inverse view-projection (words 16..19) becomes
 * (t + dx*c0) + dy*c1 per component, c0 and c1 its x and y columns (words 4..7, 8..11),
 * dx = float(2*px - (s-1)) / float(W), dy = float(2*py - (s-1)) / float(H), f32 without contraction;
 * every other word is copied, and so are words 16..19 when dx = dy = 0 (the centred phase of s = 3:
 * ptx_upsample's contract).  s in 2, 3, 4, px, py < s, W and H non-zero multiples of s, no null
 * pointer: PTX_E_INVALID otherwise.  The two arrays may be the same.
 *   ptx_upsample_temporal is ptx_upsample for a `lo` rendered and denoised through such a uniform, with a
 * history on `hi`.  ptx_upsample's preconditions hold with one change: lo's uniform words 4..22 equal,
 * bit for bit, those ptx_phase_uniform makes of hi's current uniform for (s, px, py).  hi pixel (x, y)
 * sits at fx = float(int(x) - int(px)) / float(s), x0 = floor(fx), ax = fx - x0 (y likewise) of lo:
 *   current estimate u   ptx_upsample's stages 1 and 2 at these positions; stage 3 is lo's pixel
 *                        (clamp(x0 + (ax >= 0.5), 0, w-1), clamp(y0 + (ay >= 0.5), 0, h-1));
 *   own sample d         where (x - px) and (y - py) are multiples of s and lo's pixel
 *                        ((x - px) / s, (y - py) / s) has hi's key (or neither has a primary hit): that
 *                        pixel's denoised rgb, and the pixel is "sampled";
 *   history H_h, n_h     only with the previous call's state on hi (its guide records, its {H, n} and its
 *                        uniform words 4..22 with their VP): ptx_denoise's temporal lookup -- the same
 *                        pixel when words 4..22 are that call's bit for bit, else the four pixels around
 *                        the hit point's projection with bilinear weights; a tap counts inside the image
 *                        with the same key, any n' >= 0, normals within dot >= 0.9 and within the plane
 *                        distance r -- H_h = sum(w * H') / sum(w) when a tap counted and sum(w) > 0,
 *                        n_h = min n'.  A pixel without a primary hit looks only at itself, only when
 *                        the words are equal, and only its key is compared;
 *   integration          sampled, history:  n = min(n_h + 1, 255), H = mix(H_h, d, max(1 / n, alpha_min))
 *                        sampled, none:     H = d, n = 1
 *                        not sampled, history with n_h >= 1:  H = mix(H_h, u, alpha_fill), n = n_h
 *                        otherwise:         H = u, n = 0
 *                        (mix(a, b, t) = a * (1 - t) + b * t).
 * hi's PTX_BUF_DENOISED is {H.rgb, 1}, PTX_BUF_UPSAMPLE_HISTORY {H.rgb, n}; with this call's guide
 * records and words 4..22 it is the next call's history (two sets, one read, one written: 96 bytes per
 * pixel beside the 16 of the output, allocated by the first call, counted in device_bytes).
 * ptx_upload_scene, ptx_reset_accumulation, ptx_upsample, ptx_upsample_bands, ptx_denoise and
 * ptx_denoise_bands on hi drop the history (the next call is a first call); ptx_set_frame never does.
 * ptx_update_scene with PTX_EDIT_INSTANCES on hi drops it too: the temporal upsampler does not follow
 * moved objects unless the handle follows: ptx_upsample_follow (the temporal mode of ptx_denoise always
 * does); a material or light edit keeps it.
 * After the call hi is no source of a ptx_upsample until it has been denoised or upsampled itself.
 *   PTX_E_INVALID with the reason in hi's ptx_last_error, before any GPU work: everything ptx_upsample
 * refuses (band handles: ptx_upsample_temporal_bands), a phase not below s, a lo whose camera is not that
 * phase's (the unshifted camera at s = 2 and s = 4 included), an alpha_min that is not 0 or finite and
 * in (0, 1], an alpha_fill that is not negative-and-finite (the default) or in [0, 1], a non-zero
 * reserved word.
 *   Ordering is ptx_upsample's: hi's stream waits for the tail of lo's last denoise, every stream lo can
 * next run on waits for hi's kernels.  Nothing of lo changes its bits; of hi only these buffers do.
 * Launches (hi's PTX_STAT_DENOISE): 2 (guide records, dn_upsample_temporal). */
int ptx_phase_uniform(const uint32_t hi_uniform[PTX_UNIFORM_WORDS], uint32_t s, uint32_t px, uint32_t py,
                      uint32_t lo_uniform_out[PTX_UNIFORM_WORDS]);
typedef struct ptx_upsample_temporal_params {
    float sigma_plane;    /* as ptx_upsample; 0 = default 0.02 */
    uint32_t px, py;      /* phase of lo's frame, < s */
    float alpha_min;      /* least weight of a new own sample; 0 = default 0.02 */
    float alpha_fill;     /* weight of the interpolated estimate on a pixel not sampled this call that has
                             sampled history; negative = default 0.05, 0 keeps the history as it is */
    uint32_t reserved[3]; /* zero */
} ptx_upsample_temporal_params; /* 32 bytes */
int ptx_upsample_temporal(ptx_handle *hi, ptx_handle *lo, const ptx_upsample_temporal_params *p /* NULL = defaults, phase (0, 0) */);
/* Following (opt-in: a switch on the full-size handle, whole image or band; 0 = off, the default, 1 = on.
 * With the switch never set every call and every drop is the one above, launch for launch and bit for bit).
 * The call itself launches nothing and touches no GPU memory; PTX_E_INVALID for a null handle or follow > 1.
 *   A handle is tracking when its last completely enqueued ptx_upsample_temporal / _bands call was made
 * with the switch on; switching off ends the tracking, and if an edit is pending (below) drops the state, so
 * that the next call is the first call it would have been.  Every call made with the switch on keeps the
 * instance block of the scene array (33 words per instance) and the layout it ran under; the first one
 * allocates a snapshot buffer of the upsampler's own, 80 bytes per triangle of the scene (counted in
 * device_bytes; the denoiser's snapshot is the shape *its* previous temporal call saw, another moment).
 *   While tracking with a state, ptx_update_scene with PTX_EDIT_INSTANCES, ptx_update_vertices and
 * ptx_skin_vertices on hi keep the state and mark an edit pending.  The first vertex call on a mesh since the
 * last upsample call first saves the mesh's triangle records -- a device-to-device copy on the call's stream
 * ahead of the refit, no launch -- and marks the mesh; later updates before the next call save nothing.  The
 * G-buffer rule is unchanged: the next call is refused until hi has run a G-buffer pass or a frame.
 *   The next call with the switch on, a state and a pending edit gives every instance a flag from the kept
 * block and the current one, by ptx_denoise's rule ("Object motion"): 0 unchanged, 1 moved rigidly
 * (D = M_prev * Minv_cur), 2 anything else, a switched mesh included; and 3 for an instance with the same mesh
 * word whose mesh is marked, whatever became of its matrices ("Vertex motion") -- 2 instead where the records
 * were not saved, the layout was derived again since, or the buffer sizes differ.  The table (and, with a
 * flag 3, the kept instances) is uploaded with a synchronous copy on hi's stream: this one call waits for
 * the frame it follows, as the denoiser's does.  A hit pixel's history lookup then goes by the flag of its
 * instance (key >> 16; past the table: 0); the estimate u, the own sample d and the integration are unchanged:
 *   flag 0   as above;
 *   flag 2   no lookup (sampled: H = d, n = 1; otherwise H = u, n = 0);
 *   flag 1   Q = D P, Nq = D N (linear part, not renormalised) are where the point and its normal were at the
 *            previous call; Q is always projected through that call's VP, under the same camera words too;
 *            the four taps and bilinear weights are the reprojection's, and a tap counts inside the image with
 *            the same key, n' >= 0, dot(Nq, N') >= 0.9 and |dot(Nq, P' - Q)| <= this pixel's r;
 *   flag 3   Q and Nq are the position and normalised normal of this pixel's G-buffer texel (triangle,
 *            barycentrics) on the snapshot's triangle record under the previous call's instance matrices;
 *            then as flag 1.
 * A pixel without a primary hit is unchanged.  A call with the switch off on a handle with a pending edit is
 * a first call.  The marks and the pending edit are cleared by the next upsample call, used or not, and by
 * everything that drops the state (ptx_upload_scene, ptx_reset_accumulation, ptx_upsample*, ptx_denoise* on hi).
 *   Bands: every band makes the same edits and builds its table from its own kept block; nothing new is
 * exchanged, and a band that keeps its state across an edit sends its state rows as ever.  A flag-1 or flag-3
 * pixel has taps off itself under the same camera too: such a tap inside the image but outside the covered
 * history rows is not taken and counts in PTX_COUNTER_UPSAMPLE_CLIP, as a reprojected one.
 * Launches: 2, following or not (guide records; dn_upsample_temporal, with a table its FOLLOW instance). */
int ptx_upsample_follow(ptx_handle *hi, uint32_t follow);
/* ptx_upsample_temporal for a frame split into row bands (Temporal upsampling, bands):
 * n pairs in band order, lo[i] a band of the small frame after ptx_denoise_bands, hi[i] the band of
 * the full-size frame with s times its rows.  The forms are ptx_upsample_bands': n pairs of one
 * process whose lo bands continue one another and cover the frame; n = 1 with two whole-image handles
 * (exactly ptx_upsample_temporal(hi[0], lo[0], p) with reserved[0] zeroed); or n = 1 with a lo[0] whose
 * communicator has world > 1: the rank's pair of a frame every rank makes the call for.  Either every
 * lo owns a communicator or none does (peer copies; several pairs may share a GPU).
 *   In this call reserved[0] of the parameters is history_rows T: 0 = 32, else 1..128; reserved[1..2]
 * are zero.  Per pair ptx_upsample_bands' preconditions hold and ptx_upsample_temporal's camera rule:
 * lo[i]'s words 4..22 are ptx_phase_uniform's of hi[i]'s uniform for (s, px, py), bit for bit.
 *   The definition is the whole-image call's with every position the frame's; band offsets enter
 * addresses only.  The small side: full-size row y reads small rows floor((y - py) / s) - 1 .. + 2, so 2
 * rows of each neighbouring lo band suffice for every phase (their guide records are the ones lo[i]'s
 * last ptx_denoise_bands left in its window); a pixel's own sample is a row of lo[i] itself.
 *   The history: a band's state covers rows [Y0 - min(T, Y0), Y1 + min(T, H - Y1)) of the frame: its
 * own rows as its previous call wrote them, the others its neighbours' own edge rows of their
 * previous call, brought by this call's exchange.  A candidate tap inside the image but outside the
 * covered rows is not taken, exactly as if it failed the n' >= 0 test, and a pixel with such a
 * candidate adds 1 to PTX_COUNTER_UPSAMPLE_CLIP on its band (the same-pixel rule, a pixel without
 * a primary hit and cw <= 0 never clip).  With the counter 0 on every band the split equals the
 * whole-image pair bit for bit, in PTX_BUF_DENOISED and PTX_BUF_UPSAMPLE_HISTORY; in general a band's
 * result is the whole-image definition with the previous state's taps outside its covered rows removed.
 *   One exchange per call, before the kernels, three messages per side: lo[i]'s first / last 2 rows of
 * PTX_BUF_DENOISED (16 B per pixel) and, where the frame has a neighbour, the first / last T rows of
 * the set hi[i] reads, guide records (32 B) and {H, n} (16 B), over lo's communicators (counted in
 * lo's halo_bytes_sent) or by peer copies.  They are posted in every call; a band without a state (a
 * first call, or after a drop) sends rows with n below 0, where every tap fails.  Each band takes its
 * mode (no history / same camera / reproject) from its own state: a band whose state was dropped
 * alone starts without history and its neighbours find no taps in its rows.
 *   Everything that drops the whole-image state drops a band's (ptx_upload_scene,
 * ptx_reset_accumulation, ptx_upsample, ptx_upsample_bands, ptx_denoise, ptx_denoise_bands on hi[i]);
 * ptx_set_frame never does.  After the call hi[i] is no source of a ptx_upsample.  Buffers of hi[i]:
 * PTX_BUF_DENOISED and PTX_BUF_UPSAMPLE_HISTORY hold its band_h rows; the two sets carry up to 128
 * rows above and below the band's (or what the frame has), and with the 2 x 2 small halo rows they
 * are allocated by the first call and counted in device_bytes.  Nothing of lo changes its bits; of hi
 * only these buffers do.
 *   PTX_E_INVALID with the reason in hi[0]'s ptx_last_error, before any GPU work and before anything
 * is posted: everything ptx_upsample_bands refuses, everything ptx_upsample_temporal refuses about its
 * parameters, phase and camera, history_rows above 128, with more than one band a full-size band of
 * fewer than T rows, a mix of lo bands with and without communicators.  ptx_upsample_temporal itself
 * keeps refusing band handles and non-zero reserved words.
 *   Ordering: hi[i]'s stream waits for the tail of lo[i]'s last denoise and for its neighbours' rows;
 * every stream lo[i] can next run on waits until hi[i]'s kernels have read it and, with peer copies,
 * until the neighbouring pairs have copied its rows; with peer copies hi[i]'s kernels, which write
 * the set its neighbours copied from in the previous call, wait for their copies.
 * Launches per band (hi[i]'s PTX_STAT_DENOISE): 2 (guide records, dn_upsample_temporal_win). */
int ptx_upsample_temporal_bands(ptx_handle *const *hi, ptx_handle *const *lo, int n,
                                const ptx_upsample_temporal_params *p /* NULL = defaults, phase (0, 0) */);
/* What ptx_present and ptx_present_async read: PTX_BUF_ACCUM (the default) or PTX_BUF_DENOISED
 * (fails before the first ptx_denoise, ptx_upsample or ptx_upsample_temporal). */
int ptx_present_source(ptx_handle *h, int which);
/* What this libptx.so is, as one JSON object in `out` (NUL-terminated, truncated to `bytes`):
 * {"abi": 5, "build": "product" | "ab" (every PTX_AB switch live: the measurement build) | "wgt"
 *  (per-wave timing), "arch": "gfx950", "ptx_ab": <PTX_AB as read>, "ptx_ab_ignored": [keys this
 *  build does not honour], "rccl": <the communicator library loaded, "" before ptx_comm_*>}.
 * Returns the full length (like snprintf).  A benchmark line carries it, so a run made on the wrong
 * library, or with switches the shipped library ignores, is labelled as such. */
int ptx_build_info(char *out, size_t bytes);
/* Closest-hit queries (TraceRay, SH/PT_1_InitPass.wgsl:605-715) for arbitrary rays.
 * rays: n x {o.x,o.y,o.z,d.x, d.y,d.z,-,-} f32 (32 B); hits: n x {t, flags|inst|mat (u32 bits),
 * prim (u32 bits), bary.x, bary.y, pos.x, pos.y, pos.z} (32 B; flags bit31 = valid).
 * eps_mode 0 = G-buffer epsilons (PT_01), 1 = secondary-pass epsilons (PT_1/PT_4/MCPT).
 * ptx_trace takes host arrays (blocking); ptx_trace_device takes device pointers (async).
 * Both run a kernel of their own (the lane-refill walk trace_queue_sm, or one thread per ray on a
 * PTX_FLAG_SIMPLE_KERNELS handle): no frame traces through it. */
int ptx_trace(ptx_handle *h, const float *rays, float *hits, size_t n, int eps_mode);
int ptx_trace_device(ptx_handle *h, const void *rays_dev, void *hits_dev, size_t n, int eps_mode);
/* Arbitrary queries through the kernel the handle's frames trace with (wave_trace: the streamed walk
 * with the instance cull when the root / instance tables fit LDS, the global-table fallback when they
 * do not, the counting instance on a PTX_FLAG_COUNT_WORK handle; occ_only != 0: the any-hit instance
 * of the GI spatial rounds).  Host arrays, blocking.
 * queries: n x {o.x,o.y,o.z,remain, d.x,d.y,d.z,kind} (32 B, the trace queue's layout); kind is a u32
 * bit pattern: 0 closest hit (remain unused), 1 Visibility (SH/PT_1_InitPass.wgsl:774-802: the
 * transmittance over `remain` along d, through at most 5 transmissive hits), 2 occlusion (0 when a hit
 * has t <= remain, else 1).
 * results: n x 8 f32 -- a closest query's is ptx_trace's hit record; a Visibility or occlusion query's
 * word 0 is the transmittance and words 1..7 are 0.
 * PTX_E_INVALID, before any GPU work: null arrays with n > 0, eps_mode outside 0 / 1, a kind outside
 * 0..2, occ_only with a query that is not an occlusion query, a PTX_FLAG_SIMPLE_KERNELS or
 * PTX_FLAG_ROW_CENSUS handle, no scene or no frame.  n = 0 is PTX_OK.  Stats slot PTX_PASS_TRACE. */
int ptx_trace_queries(ptx_handle *h, const float *queries, float *results, size_t n, int eps_mode, int occ_only);
/* Use an external hipStream_t (e.g. torch's current stream); NULL restores the own stream. */
int ptx_set_stream(ptx_handle *h, void *hip_stream);
int ptx_destroy(ptx_handle *h);
const char *ptx_last_error(const ptx_handle *h);

#ifdef __cplusplus
}
#endif
#endif
