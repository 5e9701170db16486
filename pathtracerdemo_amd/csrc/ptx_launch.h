// ptx_launch.h -- host-side launch wrappers exported by ptx_kernels.hip to ptx_api.cpp and ptx_scene.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "ptx_device.h"

namespace ptx {

constexpr int kTile = 16;
constexpr int kBlock = 256;

// Runtime switches are read from ONE environment variable, PTX_AB, a comma-separated list of
// KEY or KEY=int; a key that is absent gives `dflt`.  env_knob (ptx_api.cpp): the few the
// shipped library honours, each covered by a test -- COMM_TIMEOUT_S (test_gpu_loopback.py),
// DEBUG_FILL (test_gpu_debug_fill.py), HALO_PROXY_US (a band timed alone with PTX_FLAG_HALO_SKIP:
// the exchange's one-GPU stand-in, test_gpu_bands.py).  Any other key in PTX_AB is named on stderr
// and in ptx_build_info.  ab_knob: the A/B and diagnostic switches of the measurement builds
// (make variant NAME=x ALT_DEFS=-DPTX_AB_BUILD, make wgt; selected with PTX_LIB_PATH) -- in the
// shipped library every one is its default, a compile-time constant, and the losing branches
// fold away.  bench.py echoes PTX_AB (and any other PTX_* variable) in its line.
int env_knob(const char *key, int dflt);
#ifdef PTX_AB_BUILD
inline int ab_knob(const char *key, int dflt) { return env_knob(key, dflt); }
#else
constexpr int ab_knob(const char *, int dflt) { return dflt; }
#endif

// Whether a logic kernel's launch takes the LDS_SHADE instantiation (stage_shading): the scene's
// shading tables fit, and -- measurement builds only -- the kernel's bit of PTX_AB=SHADE_LDS=mask
// is set (a kernel alone on the LDS or the global tables; the shipped library stages in all).
// (bit 8 was wspatial_start: staged it was no faster, profiles/logic_tables/, so it reads the global tables)
enum : int { SL_INIT_START = 1, SL_INIT_STEP = 2, SL_TEMPORAL_START = 4, SL_JOB_STEP = 16 };
inline bool shade_from_lds(const Scene &sc, int kernel_bit) {
    static const int mask = ab_knob("SHADE_LDS", SL_INIT_START | SL_INIT_STEP | SL_TEMPORAL_START | SL_JOB_STEP);
    return shading_fits_lds(sc) && (mask & kernel_bit) != 0;
}
inline size_t shade_lds_bytes(bool staged, const Scene &sc) { return staged ? shading_lds_bytes(sc) : 0u; }

// dynamic LDS bytes for a traversal stack of `depth` entries per thread
inline size_t stack_lds_bytes(uint32_t depth) { return (size_t)depth * kBlock * sizeof(uint32_t); }

hipError_t launch_gbuffer(const Scene &sc, uint4 *gbuf, uint32_t stack_depth, hipStream_t s);
hipError_t launch_init(const Scene &sc, const uint4 *gbuf, uint4 *reservoir, uint32_t stack_depth, hipStream_t s);
hipError_t launch_final(const Scene &sc, const uint4 *gbuf, const uint4 *reservoir, float4 *accum,
                        uint32_t stack_depth, hipStream_t s);
hipError_t launch_mcpt(const Scene &sc, float4 *accum, uint32_t stack_depth, hipStream_t s);
// the reference's render pass: the Scene texture's fixed 600 x 450 window onto a cw x ch unorm8 canvas
hipError_t launch_present(const float4 *tex, uint32_t W, uint32_t H, uint32_t cw, uint32_t ch, bool bgra,
                          uint32_t *out, hipStream_t s);

// the denoiser (ptx_denoise.hip).  Its kernels address a row window: a W x rows image -- the whole
// frame, or a band with the halo rows its neighbours sent (ptx_denoise_bands) -- filtered as if it
// were the whole image; every buffer a launch is given starts at the window's row 0.
struct DnWin {
    uint32_t y0;      // the row of the frame that is row 0 of the window (of the buffers)
    uint32_t rows;    // the rows the window (the buffers) holds: a tap outside [0, rows) is outside the image
    uint32_t c0, c1;  // the rows this launch computes, [c0, c1)
};
// A filter input whose rows lie in two buffers: window rows [o0, o1) in `own` (its row 0 = window
// row o0: a band's accumulation), the rows above and then the rows below them in `halo`.
struct DnImage {
    const float4 *own, *halo;
    uint32_t o0, o1;
};
// guide records (2 float4 per pixel) of the band's own rows from its G-buffer (gbuf and guide start
// at the band's first row), and of a window's halo rows from received texels (`top` rows above the
// band, then `bottom` below; guide starts at the window's row 0); the variance pass
// image -> {r, g, b, v}; one a-trous iteration at `step` (a power of two; `last`: the output's alpha is 1)
hipError_t launch_denoise_guide(const Scene &sc, const uint4 *gbuf, float4 *guide, float sigma_plane, hipStream_t s);
hipError_t launch_denoise_guide_halo(const Scene &sc, const uint4 *texels, uint32_t top, uint32_t bottom, float4 *guide,
                                     float sigma_plane, hipStream_t s);
hipError_t launch_denoise_variance(uint32_t W, const DnWin &win, const DnImage &img, const float4 *guide, float4 *out,
                                   hipStream_t s);
hipError_t launch_denoise_atrous(uint32_t W, const DnWin &win, uint32_t step, const float4 *in, const float4 *guide,
                                 float4 *out, float sigma_lum, bool last, hipStream_t s);
// temporal mode: the history lookup and integration over rows [c0, c1) of the window, the band's own
// rows, where frame and accum start (mode 0 no history, 1 same pixel, 2 through vp_prev; p*: the
// previous call's guide, history and moment records, which start at row prev_y0 of the W x H frame
// and hold prev_rows rows; *clip counts the pixels with a candidate past them) -> history {C.rgb, n},
// moments {m1, m2}; the variance pass on that history, the moments' variance where n >= 4
// obj (nullptr: no instance changed since the previous call, dn_temporal<false>): n_obj entries, one per
// instance -- how its pixels find their history (dn_temporal<true>, ptx_denoise.hip)
struct DnObj {
    float d[16];    // column-major D = M_prev * Minv_cur: a point of the instance now -> at the previous call
    uint32_t flag;  // 0 unchanged, 1 moved rigidly (follow D), 2 anything else (no history); 3 its mesh was deformed
                    // (dn_temporal_verts alone: follow the vertices)
    uint32_t pad[3];
};
// Following vertices (a call that finds a mesh deformed since the previous one, dn_temporal_verts): a second
// table beside obj, an instance as the previous call saw it, in the device Inst's form; the band's G-buffer
// texels (from its first row, like frame); and the triangle records saved before the refits, Scene::tverts'
// layout.  snap == nullptr: the two kernels above.
struct DnPrev {
    float m[16], minv[16];    // words 0..15 and 16..31 of the kept instance block
    uint32_t mesh, tri_base;  // mesh | kInstIdentity as in Inst (inst_point's shortcut); the mesh's first triangle record
    uint32_t pad[2];
};
struct DnVerts {
    const uint4 *gbuf = nullptr;
    const DnPrev *prev = nullptr;
    const float4 *snap = nullptr;
};
hipError_t launch_denoise_temporal(uint32_t W, uint32_t H, const DnWin &win, const float *vp_prev, float alpha_min,
                                   uint32_t mode, uint32_t prev_y0, uint32_t prev_rows, const float4 *guide,
                                   const float4 *frame, const float4 *accum, const float4 *pguide, const float4 *phist,
                                   const float2 *pmom, float4 *hist, float2 *mom, unsigned long long *clip,
                                   const DnObj *obj, uint32_t n_obj, const DnVerts &verts, hipStream_t s);
hipError_t launch_denoise_variance_moments(uint32_t W, const DnWin &win, const float4 *hist, const float2 *mom,
                                           const float4 *guide, float4 *out, hipStream_t s);
// ptx_upsample: the (W / s) x (H / s) image `color_lo` with its guide records, written at W x H under
// `guide_hi` (s: 2, 3 or 4)
hipError_t launch_denoise_upsample(uint32_t s, uint32_t W, uint32_t H, const float4 *guide_hi, const float4 *guide_lo,
                                   const float4 *color_lo, float4 *out, hipStream_t st);
// ptx_upsample_temporal: the same inputs, `color_lo` rendered through phase (px, py) of the s x s block,
// integrated with the previous call's guide records and history {H.rgb, n} (mode: 0 none, 1 the same
// camera words, 2 reprojected through vp_prev) into `hist` and, with alpha 1, `out`
// fo (ptx_upsample_follow): the table of a following call that finds an instance changed or a mesh deformed
// since the previous one -- DnObj per instance and, with a flag 3 among them, DnVerts, both as
// launch_denoise_temporal takes them (gbuf: the full-size band's texels from its first row).  obj == nullptr:
// the kernel without the table (FOLLOW = 0).
struct UtFollow {
    const DnObj *obj = nullptr;
    uint32_t n_obj = 0;
    uint32_t n_snap = 0;  // triangle records verts.snap holds (a texel's triangle is clamped to them)
    DnVerts verts;
};
hipError_t launch_denoise_upsample_temporal(uint32_t s, uint32_t W, uint32_t H, uint32_t px, uint32_t py, float alpha_min,
                                            float alpha_fill, uint32_t mode, const float *vp_prev, const UtFollow &fo,
                                            const float4 *guide_hi, const float4 *guide_lo, const float4 *color_lo,
                                            const float4 *guide_prev, const float4 *hist_prev, float4 *hist, float4 *out,
                                            hipStream_t st);
// ptx_upsample_bands: rows [Y0, Y1) of the W x H frame (guide_hi and out start at row Y0) from a row
// window of the small frame: `rows` rows from its row y0 on, where guide_lo starts; the window's rows
// [o0, o1) are color_lo's (a band's own rows), the rows above and then the rows below them halo_lo's.
struct UpWin {
    uint32_t y0, rows, o0, o1;
    uint32_t Y0, Y1;
};
hipError_t launch_denoise_upsample_win(uint32_t s, uint32_t W, uint32_t H, const UpWin &win, const float4 *guide_hi,
                                       const float4 *guide_lo, const float4 *color_lo, const float4 *halo_lo, float4 *out,
                                       hipStream_t st);
// ptx_upsample_temporal_bands: the same rows and window (`up`), integrated with the rows
// [hy0, hy0 + hrows) of the frame the previous state covers, where guide_prev and hist_prev start;
// hist and out start at row Y0.  *clip counts the pixels with a history tap inside the frame but
// outside those rows (the tap is not taken): under a moved camera, and with a table (fo) under any.
struct UtWin {
    UpWin up;
    uint32_t hy0, hrows;
    unsigned long long *clip;
};
hipError_t launch_denoise_upsample_temporal_win(uint32_t s, uint32_t W, uint32_t H, uint32_t px, uint32_t py, float alpha_min,
                                                float alpha_fill, uint32_t mode, const float *vp_prev, const UtWin &win,
                                                const UtFollow &fo, const float4 *guide_hi, const float4 *guide_lo,
                                                const float4 *color_lo, const float4 *halo_lo, const float4 *guide_prev,
                                                const float4 *hist_prev, float4 *hist, float4 *out, hipStream_t st);

// ptx_update_vertices (ptx_refit.hip): one mesh's derived tables from its new vertices.  The ranges of
// the mesh in the tables, from build_layout (ptx_handle::lay_mesh_*); G, tris, tverts, nodes and subs
// are the whole tables, `box` the scratch {lo.xyz, hi.xyz} per triangle of the mesh, `order` the
// mesh's pairs by height (global pair indices).
struct RefitMesh {
    const uint32_t *G;
    float4 *tris, *tverts;
    NodePair *nodes;
    SubRoot *subs;
    float2 *box;            // 3 float2 per triangle: {lo.x, lo.y}, {lo.z, hi.x}, {hi.y, hi.z}
    const uint32_t *order;
    uint32_t vertex, index;  // first word in G of the mesh's vertex records / of its index buffer
    uint32_t tri_base, n_tris, sub_base, n_subs;
};
// the triangle records (edge form, vertex / normal) and boxes of the mesh's n_tris triangles
hipError_t launch_refit_tris(const RefitMesh &m, hipStream_t s);
// one height of the tree: the pairs order[first, first + n), whose interior children are lower
hipError_t launch_refit_level(const RefitMesh &m, uint32_t first, uint32_t n, hipStream_t s);
// the root records' boxes, after the last height
hipError_t launch_refit_roots(const RefitMesh &m, hipStream_t s);

// ptx_skin_vertices (ptx_skin.hip): the bound vertices [0, n) of one skin written over words 0..5 of
// their records, which begin at word `word0` of G (16-byte aligned).  `bind` holds three float4 per
// vertex -- {p.xyz, n.x}, {n.y, n.z, w0, w1}, {w2, w3, j0 | j1 << 16, j2 | j3 << 16} --, the delta tables
// are target-major (3 floats per target and vertex; target_nrm may be null), `palette` three float4
// per joint, all on the device.  The refit chain of ptx_update_vertices follows it on the stream.
constexpr uint32_t kSkinMaxJoints = 256u, kSkinMaxTargets = 8u;
struct SkinArgs {
    uint32_t *G;
    const float4 *bind;
    const float *target_pos, *target_nrm;
    const float4 *palette;
    const float *target_weights;
    uint32_t word0, n, n_joints, n_targets;
};
hipError_t launch_skin_vertices(const SkinArgs &a, hipStream_t s);

// ptx_build_blas (ptx_build.hip): one mesh's BLAS as an LBVH.  Every pointer is device memory of the call.
// Radix nodes are numbered by sorted position: the internal node i of a group at first_tri + i (ids [0, T)),
// the leaf of sorted position p at T + p (ids [T, 2T)).
struct BuildArgs {
    const float *pos;            // V x 3
    const uint32_t *idx;         // 3T, the input index buffer
    const uint2 *groups;         // n_groups x {first_tri, tri_count}
    uint32_t n_tris, n_groups, max_leaf;
    uint32_t n_nodes;            // nodes nodes_out holds (build_emit)
    float2 *tbox;                // 3 float2 per triangle, input order: {lo.x, lo.y}, {lo.z, hi.x}, {hi.y, hi.z}
    float *centre;               // 3 per triangle, input order
    uint32_t *seg;               // per position: 2g + 1 inside group g, 2g in the gap ahead of it
    uint32_t *cbound;            // 6 per group, zeroed: ~ordered(min) xyz, ordered(max) xyz of the centres
    unsigned long long *key_in, *key_out;  // segment << 30 | code, before and after the sort
    uint32_t *val_in, *val_out;  // the triangle's input position
    void *sort_temp;
    size_t sort_bytes;
    uint2 *rng, *child;          // per internal node: its sorted positions [a, b]; its children's ids
    uint32_t *parent;            // per id, 0xFF-filled: the parent's id (a root keeps 0xFFFFFFFF)
    float2 *nbox;                // per id: the box of an emitted node, tbox's layout
    uint32_t *esize;             // per id: emitted nodes of its subtree
    uint32_t *done;              // per id, zeroed: the stamp of the launch that finished it (build_level)
    uint32_t *gsize;             // per group: its root's esize, 0 while unfinished
    const uint32_t *goff;        // per group: its root's node in nodes_out
    uint32_t *nodes_out;         // 8 words per node
    uint32_t *idx_out;           // 3T
    uint32_t *max_depth;         // zeroed
};
enum class BuildStep { Tris, Keys, Sort, Tree, Leaves, Level, Roots, Emit, Gather };
// the sort's temporary storage for A.n_tris keys of A.n_groups groups
hipError_t build_sort_bytes(const BuildArgs &A, size_t *bytes);
// one step of the chain; `stamp` is build_level's (2, 3, ...: one launch per height of the emitted tree)
hipError_t launch_build(const BuildArgs &A, BuildStep step, uint32_t stamp, hipStream_t s);

// ptx_build_blas, PTX_BLAS_SAH (ptx_build_sah.hip): the host builder's binned-SAH tree, top-down, a launch per
// level.  Every pointer is device memory of the call.  Nodes are numbered as they are made: the roots 0 ..
// n_groups - 1, a node's two children consecutively from counters[0]; a level's nodes are a contiguous range.
struct SahArgs {
    const float *pos;            // V x 3
    const uint32_t *idx;         // 3T, the input index buffer
    const uint2 *groups;         // n_groups x {first_tri, tri_count}
    uint32_t n_tris, n_groups, max_leaf;
    uint32_t node_cap;           // nodes the tables hold: sum(2 * tri_count - 1)
    uint32_t n_nodes;            // nodes made (sah_emit)
    float *rec;                  // 6 per triangle, input order: the centre xyz, the half-extent xyz
    uint32_t *order[2];          // per position: the triangle there, at even and at odd levels
    uint32_t *final_order;       // per position: the triangle there once its leaf is made (gaps: itself)
    uint2 *n_range;              // per node: {first position, count}
    float *n_box;                // 6 per node
    uint4 *n_link;               // per node: {parent (a root: 0xFFFFFFFF), left child (right: + 1), the split
                                 // axis or 3 for a leaf, group}
    uint32_t *n_size;            // per node: nodes of its subtree
    uint32_t *counters;          // [0] nodes made, [1] the largest leaf
    const uint32_t *goff;        // per group: its root's node in nodes_out
    uint32_t *nodes_out;         // 8 words per node
    uint32_t *idx_out;           // 3T
};
enum class SahStep { Init, Level, Size, Emit, Gather };
// one step: Init and Gather over n = n_tris, Level over the n nodes from first_node at depth `level` (one
// workgroup each), Size over the same range, Emit over n = n_nodes
hipError_t launch_sah(const SahArgs &A, SahStep step, uint32_t first_node, uint32_t n, uint32_t level, hipStream_t s);

// ptx_rebuild_mesh (ptx_build.hip): the packed positions (n_vertices x 3, device) of the vertex records that
// begin at word `vertex_word` of the device's geometry array G
hipError_t launch_build_positions(const uint32_t *G, uint32_t vertex_word, uint32_t n_vertices, float *pos, hipStream_t s);

// ptx_blas_cost (ptx_cost.hip): the surface-area cost of one mesh's trees from the device's tables.  One thread
// per child of the mesh's n_pairs pairs (from pair `pair_base`) and one per root record (n_subs from `sub_base`);
// pair_sub[p] is pair p's sub-mesh (a global SubRoot index).  `partial` takes one f64 per workgroup
// (cost_blocks(n_pairs, n_subs) of them), reduced in a fixed order; the host adds them in index order.
struct CostArgs {
    const NodePair *nodes;
    const SubRoot *subs;
    const uint32_t *pair_sub;
    uint32_t pair_base, n_pairs, sub_base, n_subs;
    double *partial;
};
uint32_t cost_blocks(uint32_t n_pairs, uint32_t n_subs);
hipError_t launch_blas_cost(const CostArgs &a, hipStream_t s);

// closest-hit queries for a ray array (ptx_kernels.hip)
hipError_t launch_trace_rays(const Scene &sc, const float4 *rays, float4 *hits, uint32_t n, int eps_mode,
                             uint32_t stack_depth, hipStream_t s);

// wavefront variant (ptx_wave.hip): the default.  A pass is a fixed sequence of rounds:
// logic round 0 (start), then {trace r, logic r+1} for r < kWaveRounds[pass].  Every
// launch has one workgroup per segment; queue lengths live on the device
// (cnt[(2r) * nseg + j] pixels of segment j active after logic round r, cnt[(2r+1) *
// nseg + j] rays it emitted), so the host never synchronises inside a pass.
constexpr uint32_t kWaveStateSlots = 10u;  // float4 per pixel (PT_1 needs the most)
// PT_1 state slots the reuse pipeline's temporal pass reads (vertex 2 / 3 hit compacts, the
// selected NEE candidate's Visibility or -1 for an env candidate): ptx_wave.hip IS_*
constexpr uint32_t kStateCs2 = 7u, kStateCs3 = 8u, kStateTsel = 9u;
constexpr uint32_t kWaveSegPixels = 768u;  // padded pixels per segment (12 8x8 tiles); 768 > 512 > 1024 > 256
constexpr int kWaveRoundsInit = 3, kWaveRoundsFinal = 3, kWaveRoundsMcpt = 4;
constexpr int kWaveMaxRounds = 5;
struct WaveBufs {
    float4 *state;       // kWaveStateSlots * npix, SoA
    uint32_t npix;       // pixels of the band
    uint32_t seg_px;     // padded pixels per segment
    uint32_t nseg;       // segments of the band
    uint32_t seg_base;   // first segment of this launch sequence (workgroup j -> segment
    uint32_t seg_count;  //   seg_base + j), and how many it covers
    uint32_t cluster;    // segment layout: 16/cluster runs of `cluster` adjacent 8x8 tiles
    uint32_t ray_stride; // ray slots per segment (seg_px * max rays per pixel per round)
    float4 *rays;        // 2 float4 per ray: {o, remain}, {d, kind}
    float4 *res[3];      // 2 float4 per ray, ping-pong by round parity (nres = 2) or one per
    uint32_t nres;       // round (nres = 3: the spatial reuse pass, whose combine reads every
                         // round's light-ray results; res_buf)
    uint32_t *act[2];    // active pixel / job lists (nseg * act_stride), ping-pong
    uint32_t act_stride; // list entries per segment (seg_px; seg_px * jobs per pixel for reuse)
    uint32_t *cnt;       // 2 * kWaveMaxRounds * nseg counts
    // Tile set of the launch: virtual tile v (what the segments spread over) is band tile
    // v < ntile0 ? tile0 + v : tile1 + (v - ntile0), for v < ntile0 + ntile1 (8x8 tiles in
    // raster order).  Default: the whole band.  A band's spatial pass runs its interior rows
    // and its halo-dependent edge rows as two tile sets (the exchange overlaps the first).
    uint32_t tile0, ntile0, tile1, ntile1;
    // Queue memory: virtual segment j lives in physical slot seg_phys + j (ray / result / list
    // storage, count words at cnt[(2r or 2r+1) * cnt_stride + slot]).  Two tile sets in flight
    // at once use disjoint physical slots.
    uint32_t seg_phys, cnt_stride;
    // DI reuse pipeline: primary-hit surface records (2 uint4 per pixel, first band row; halo
    // rows at negative / >= npix indices), written by winit_start; nullptr otherwise
    uint4 *surf;
};
// occ_only: every query of the round is Q_OCC (any-hit kernel instance)
hipError_t wave_trace(const Scene &sc, const WaveBufs &w, int round, int eps_mode, uint32_t stack_depth,
                      hipStream_t s, bool occ_only = false);
hipError_t wave_init_round(const Scene &sc, const WaveBufs &w, int round, const uint4 *gbuf, uint4 *reservoir,
                           hipStream_t s);
// PT_4 of the reuse pipeline in one launch, replays walked inline (scene tables in LDS)
hipError_t wave_final_one(const Scene &sc, const WaveBufs &w, const uint4 *gbuf, const uint4 *reservoir, float4 *accum,
                          uint32_t depth, hipStream_t s);
// PT_4 behind a spatial combine that shaded (ReuseArgs::fuse_final): wfinal_one over each
// segment's replay list only; a workgroup whose list is empty leaves before staging the tables
hipError_t wave_final_replay(const Scene &sc, const WaveBufs &w, const uint4 *gbuf, const uint4 *reservoir, float4 *accum,
                             const uint32_t *replay, uint32_t *replay_cnt, uint32_t depth, hipStream_t s);
hipError_t wave_final_round(const Scene &sc, const WaveBufs &w, int round, const uint4 *gbuf, const uint4 *reservoir,
                            float4 *accum, hipStream_t s);
hipError_t wave_gbuffer(const Scene &sc, const WaveBufs &w, uint4 *gbuf, uint32_t stack_depth, hipStream_t s);
hipError_t launch_trace_rays_sm(const Scene &sc, const float4 *rays, float4 *hits, uint32_t n, int eps_mode,
                                uint32_t stack_depth, hipStream_t s);
// color: nullptr mixes every finished path into accum (WriteColor); else the path colours go to
// color (a pipelined frame) and wave_mix_frame mixes them in after the previous frame's
hipError_t wave_mcpt_round(const Scene &sc, const WaveBufs &w, int round, float4 *accum, float4 *color,
                           hipStream_t s);
hipError_t wave_mix_frame(const Scene &sc, const float4 *color, float4 *accum, hipStream_t s);

// reuse passes (ptx_reuse.hip): round 0 start, 1..kWaveRoundsReuse step, then combine
constexpr int kWaveRoundsReuse = 3;
struct ReuseArgs {
    const uint4 *gbuf;  // G-buffer of the band's first row; halo rows at negative / >= npix indices
    uint4 *cur;         // PT_1 reservoirs (temporal output in place), same addressing
    uint4 *hist;        // spatial output = PT_4 input = next frame's history, cur's addressing
                        // (a band's halo rows: the neighbours' previous spatial output, motion pass)
    float4 *jstate;     // shift-job state, 6 float4 slots x njobs (SoA)
    float4 *jres;       // per job: {f (PathContribution, rgb), q} (q = 0: invalid); p_hat = Luminance(f)
    uint32_t njobs, jpp;  // jobs of the pass (npix * jpp), jobs per pixel
    // job id of (pixel, slot) = pix * jpx + slot * jslot: slot planes (jpx 1, jslot npix), so a
    // wave's jobs -- one 8x8 tile, one slot -- read and write whole 128-byte lines of the SoA
    // state (pixel-major, jpx = jpp: 16-byte pieces 16 * jpp bytes apart)
    uint32_t jpx, jslot;
    uint32_t radius, neighbors, cap, hist_valid;
    uint32_t use_init;  // temporal: this frame's PT_1 wave state (path hits, NEE Visibility) is in w.state
    const uint4 *nbr;   // spatial: per-pixel neighbour summary (wave_reuse_summary), cur's addressing
    uint4 *nbr_out;     // the same buffer: the temporal pass writes its output's summaries
    const uint4 *surf;  // primary-hit surface records (WaveBufs::surf), cur's addressing
    // spatial: a job's light segment is finished by the combine -- every light ray a job emits
    // leaves {ray index, result buffer, -, kJobPending} in jres (the pass keeps one result
    // buffer per trace round, WaveBufs::nres = 3), and the combine reads its Visibility result
    // and the job's F slot itself (wjob_step's phase-1 arithmetic); no step launch after the
    // last trace round, and the steps see heavy jobs only
    uint32_t fold_last;
    uint32_t ray_cap;   // ray slots of the wave buffers: a stale jres word (a slot the combine
                        // loads but does not use) never sends the fold's gather out of bounds
    // temporal reuse under camera motion (wtmotion_*, ptx_reuse.hip): the previous frame's
    // VP^-1 (its camera points) and VP (the reprojection), its primary-hit surface records
    // (cur's addressing); motion = 1 selects the pass.  hist / psurf hold the previous frame's
    // band rows [prev_row_lo, prev_row_hi) (band-relative: a band's motion halo, the whole image
    // [0, H)); a pixel reprojected outside them has no history (and counts in *clip)
    uint32_t motion;
    float vpinv_prev[16], vp_prev[16];
    const uint4 *psurf;
    int32_t prev_row_lo, prev_row_hi;
    unsigned long long *clip;  // nullptr: not counted
    // spatial combine followed by PT_4 in one launch sequence: the combine does PT_4's per-pixel
    // cases itself (wfinal_one's, with the values it holds: the same mix_color into accum and
    // Scene::frame_color), and a pixel whose contribution is unknown -- the only kind PT_4 has to
    // replay -- goes to its segment's replay list: replay[slot * seg_px ..] with its length in
    // replay_cnt[slot] (slot = the segment's physical queue slot; wave_final_replay consumes the
    // list and zeroes the length), the listed pixels counted in *replay_total
    uint32_t fuse_final;
    float4 *accum;
    uint32_t *replay, *replay_cnt;
    unsigned long long *replay_total;
};
// the motion temporal pass's jobs per pixel: the canonical sample at home, the reprojected
// history sample here, the canonical sample in the previous frame's domain
constexpr uint32_t kMotionJobs = 3u;
constexpr uint32_t kJobPending = 0xFFFFFFFFu;  // jres.w of such a job (a NaN: never a stored q)
// The fold keeps ONE result buffer per trace round (WaveBufs::res[0..2], res_sel = round % 3):
// a fourth round would overwrite the round-0 light results the combine still reads.
static_assert(kWaveRoundsReuse <= 3, "fold_last: one result buffer per reuse trace round");
// rounds of {trace, step} between a reuse pass's start and combine launches
int reuse_rounds(int pass_temporal, const ReuseArgs &A);
hipError_t wave_reuse_round(const Scene &sc, const WaveBufs &w, int pass_temporal, int round, const ReuseArgs &A,
                            hipStream_t s);
// Spatial pass prologue over every band + halo pixel (npx of them, from the first halo row):
// the 16-byte neighbour summary {p_hat, q, W, valid | length | C} the spatial kernels gather
// instead of a G-buffer line and a reservoir line per neighbour.
// With `surf`, the same pixels' primary-hit surface records too (halo rows just received).
hipError_t wave_reuse_summary(const Scene &sc, const uint4 *gbuf, const uint4 *res, uint4 *nbr, uint4 *surf,
                              size_t npx, hipStream_t s);
// The surface records of the launch's segments from the G-buffer (a reuse pass whose band
// records are stale: no PT_1 since the G-buffer or the scene changed)
hipError_t wave_surface(const Scene &sc, const WaveBufs &w, const uint4 *gbuf, hipStream_t s);

// ReSTIR GI (ptx_gi.hip; pipeline PTX_PIPELINE_RESTIR_GI): pass 0 init (logic rounds 0..2,
// traces between), 1 temporal (one launch), 2 spatial (start, trace, combine), 3 final,
// 4 temporal under camera motion (start, trace, combine).
constexpr int kWaveRoundsGiInit = 2, kWaveRoundsGiSpatial = 1;
constexpr uint32_t kGiResU4 = 4u;  // 64-byte GI reservoir (oracle/pt_oracle_gi.c)
struct GiArgs {
    const uint4 *gbuf;  // G-buffer of the band's first row; halo rows at negative / >= npix indices
    uint4 *cur;         // GI reservoirs (init output, temporal output in place), same addressing
    uint4 *hist;        // spatial output = final input = next frame's history (band only)
    float4 *direct;     // per-pixel direct light (band)
    float4 *accum;      // accumulated radiance (band)
    uint32_t *jray;     // spatial: per job its occlusion ray's index, or 0xffffffff (no path)
    uint32_t jpp;       // spatial jobs per pixel (2 * neighbors)
    uint32_t jpx, jslot;  // job (pixel, slot) at jray[pix * jpx + slot * jslot]: slot planes
                          // (jpx 1, jslot = band pixels) or pixel-major (jpx = jpp, jslot 1)
    uint32_t radius, neighbors, cap, hist_valid;
    // temporal reuse under camera motion (pass 4; ReuseArgs' motion fields): the previous frame's
    // VP^-1 and VP, its G-buffer (gbuf's addressing, rows [prev_row_lo, prev_row_hi) held:
    // the band and its halo rows), history rows the same; a reprojection outside them counts in *clip.
    // Jobs: slot 0 the history here, slot 1 this sample at p', slots 2 / 3 p' and its confidence.
    float vpinv_prev[16], vp_prev[16];
    const uint4 *pgbuf;
    int32_t prev_row_lo, prev_row_hi;
    unsigned long long *clip;
};
constexpr uint32_t kGiMotionSlots = 4u;
hipError_t wave_gi_round(const Scene &sc, const WaveBufs &w, int pass, int round, const GiArgs &A, hipStream_t s);

}  // namespace ptx
