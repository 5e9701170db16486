"""Host-side mirror of the reference renderer class over the HIP C ABI.

Same surface and semantics as ``Renderer`` of apps/frontend/src/graphics-core/
Renderer_TEST.ts (constructor :83-126, GetCamera :129-132, ResetFrameCount :134-137,
Initialize :141-163, Update :165-206, Render :208-261), with the WebGPU device replaced
by libptx.so on one MI355X.  ``pipeline="mcpt"`` mirrors the legacy Renderer.ts
(TEST_MCPT.wgsl brute force, GC/Renderer.ts:536-647); ``pipeline="reuse"`` adds the
build-defined temporal + spatial reuse passes between PT_1 and PT_4;
``pipeline="gi"`` is BASELINE configs[4], ReSTIR GI.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from . import _native as N
from .scene.camera import Camera
from .scene.world import CompiledScene, World, serialize_world


def phase_uniform(hi_uniform: np.ndarray, s: int, px: int, py: int) -> np.ndarray:
    """The uniform of the frame of 1/s the size whose pixel (i, j) looks through pixel (s*i + px, s*j + py) of
    `hi_uniform`'s frame (ptx_phase_uniform: host arithmetic, no renderer and no GPU needed)."""
    return N.phase_uniform(hi_uniform, s, px, py)


class Renderer:
    def __init__(self, width: int, height: int, device: int = -1, pipeline: str = "restir",
                 row_begin: int = 0, row_end: int = 0, count_work: bool = False, variant: str = "wave",
                 time_launches: bool = False, single_stream: bool = False, reuse_radius: int = 0,
                 reuse_neighbors: int = 0, temporal_cap: int = 0, row_census: bool = False,
                 halo_overlap: bool = False, halo_skip: bool = False, frame_color: bool = False):
        self._lib = N.load()
        self.width, self.height = int(width), int(height)
        self.pipeline = pipeline
        # the temporal Denoise / denoise_bands follow deformed and skinned meshes (ptx_denoise_params.reserved[2]);
        # 0 / 1 (a larger value is the library's to refuse)
        self.follow_vertices: bool | int = False
        self._upsample_follow = False  # set_upsample_follow: the handle's ptx_upsample_follow switch
        cfg = N.PtxConfig(width=self.width, height=self.height, row_begin=row_begin, row_end=row_end,
                          device=device,
                          pipeline=N.PIPELINES[pipeline], reuse_radius=reuse_radius,
                          reuse_neighbors=reuse_neighbors, temporal_cap=temporal_cap,
                          flags=(N.PTX_FLAG_COUNT_WORK if count_work else 0) | N.VARIANT_FLAGS[variant]
                          | (N.PTX_FLAG_TIME_LAUNCHES if time_launches else 0)
                          | (N.PTX_FLAG_SINGLE_STREAM if single_stream else 0)
                          | (N.PTX_FLAG_ROW_CENSUS if row_census else 0)
                          | (N.PTX_FLAG_HALO_OVERLAP if halo_overlap else 0)
                          | (N.PTX_FLAG_HALO_SKIP if halo_skip else 0)
                          | (N.PTX_FLAG_FRAME_COLOR if frame_color else 0))
        self._h = ctypes.c_void_p()
        rc = self._lib.ptx_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != N.PTX_OK:
            raise N.PtxError(f"ptx_create failed ({rc})")
        self.row_begin = row_begin
        self.row_end = row_end or self.height
        self.compiled: CompiledScene | None = None
        self.camera: Camera | None = None
        self.frame_count = 0
        self.uniform = None
        self._skins: dict = {}  # mesh -> (first, n, joints, targets) of SetSkin

    # ------------------------------------------------------------------ reference surface
    def GetCamera(self) -> Camera:
        return self.camera

    def ResetFrameCount(self) -> None:
        self.frame_count = 0

    def Initialize(self, world: World | CompiledScene) -> None:
        """Renderer_TEST.Initialize: camera at (0,0,6), yaw/pitch 0, FrameCount 0, upload."""
        self.camera = Camera(self.width, self.height)
        self.camera.set_location(0, 0, 6)
        self.camera.set_yaw(0)
        self.camera.set_pitch(0)
        self.ResetFrameCount()
        self.compiled = world if isinstance(world, CompiledScene) else serialize_world(world)
        cs = self.compiled
        self._call("ptx_upload_scene", self._h, cs.scene.ctypes.data, len(cs.scene), cs.geometry.ctypes.data,
                   len(cs.geometry), cs.accel.ctypes.data if len(cs.accel) else None, len(cs.accel))
        self._skins = {}  # (the upload drops every skin)
        self._call("ptx_reset_accumulation", self._h)

    def UpdateScene(self, world: World | CompiledScene) -> int:
        """Edit instances, materials and lights in place (ptx_update_scene): `world` is the scene of
        Initialize with instances moved, turned, scaled or switched to another loaded mesh, materials
        or lights changed -- the same meshes, counts and offsets, else ValueError.  Returns the mask of
        the blocks that changed (PTX_EDIT_INSTANCES | PTX_EDIT_MATERIALS | PTX_EDIT_LIGHTS; 0: nothing
        to do).  Kept G-buffers and histories are dropped only as far as the edit needs; the frame
        count is the caller's (ResetFrameCount, as on a camera move)."""
        cs = world if isinstance(world, CompiledScene) else serialize_world(world)
        old = self.compiled
        if old is None:
            raise ValueError("UpdateScene: Initialize first")
        if (cs.offsets != old.offsets or cs.instance_count != old.instance_count or cs.light_count != old.light_count
                or len(cs.scene) != len(old.scene) or len(cs.geometry) != len(old.geometry)
                or len(cs.accel) != len(old.accel)):
            raise ValueError("UpdateScene: the edited scene has another layout (offsets, counts, geometry or accel "
                             "length): Initialize uploads it")
        scene = np.ascontiguousarray(cs.scene, dtype=np.uint32)
        mask = ctypes.c_uint32(0)
        self._call("ptx_update_scene", self._h, scene.ctypes.data, len(scene), ctypes.byref(mask))
        self.compiled = cs
        return int(mask.value)

    def UpdateVertices(self, mesh: int, positions, normals=None, first: int = 0) -> None:
        """Deform mesh `mesh` in place (ptx_update_vertices): `positions` (n, 3) f32 replace the positions
        of its vertices [first, first + n), `normals` (optional, (n, 3)) their normals; the uv words stay.
        The library derives the mesh's triangles again and refits its BLAS on the GPU, the topology
        kept; histories are kept and dropped as by an instance edit (include/ptx.h).  `compiled` is
        afterwards what the handle renders: the geometry array rewritten, the accel array read_accel()'s.
        A refused call (a range past the mesh, a position that is not finite: PtxError) changes nothing."""
        from .scene.world import STRIDE_VERTEX, mesh_blocks
        cs = self.compiled
        if cs is None or self.uniform is None:
            raise ValueError("UpdateVertices: Initialize and Update first")
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        b = mesh_blocks(cs, int(mesh))
        n_vert = (b["vertex_end"] - b["vertex"]) // STRIDE_VERTEX
        if first < 0 or first + len(pos) > n_vert:
            raise ValueError(f"UpdateVertices: vertices [{first}, {first + len(pos)}) of mesh {mesh}, which has {n_vert}")
        w0 = b["vertex"] + STRIDE_VERTEX * first
        rec = np.array(cs.geometry[w0:w0 + STRIDE_VERTEX * len(pos)], dtype=np.uint32).reshape(len(pos), STRIDE_VERTEX)
        rec[:, 0:3] = pos.view(np.uint32)
        if normals is not None:
            nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
            if len(nrm) != len(pos):
                raise ValueError("UpdateVertices: one normal per position")
            rec[:, 3:6] = nrm.view(np.uint32)
        self._call("ptx_update_vertices", self._h, int(mesh), int(first), len(rec), rec.ctypes.data if len(rec) else None)
        if not len(rec):
            return
        geometry = np.array(cs.geometry, dtype=np.uint32)
        geometry[w0:w0 + rec.size] = rec.reshape(-1)
        self.compiled = dataclasses.replace(cs, geometry=geometry, accel=self.read_accel())

    def read_accel(self) -> np.ndarray:
        """The accel array as the handle traces it now (ptx_read_accel): the uploaded one, the boxes of
        every reachable node from the device's tables -- after UpdateVertices, the refit."""
        out = np.zeros(len(self.compiled.accel), dtype=np.uint32)
        self._call("ptx_read_accel", self._h, out.ctypes.data if len(out) else None, len(out))
        return out

    def build_blas(self, positions, indices, groups, max_leaf_tris: int = 10, builder: str = "lbvh"):
        """A mesh's BLAS built on the GPU (ptx_build_blas), with scene.bvh.build_blas' signature and results --
        (roots: one u32 node array per group, the reordered indices, the largest depth).  `builder`: "lbvh"
        (bit for bit scene.lbvh.build_blas_lbvh's tree) or "sah" (bit for bit scene.sah.build_blas_sah's: the
        host SAH builder's nodes, a leaf's triangles in input order).  Needs no scene; changes nothing a frame
        reads.  compile_scene(name, builder=renderer.build_blas) compiles a scene with these trees."""
        if builder not in self._BLAS_BUILDERS:
            raise ValueError(f"build_blas: builder {builder!r} (one of {sorted(self._BLAS_BUILDERS)})")
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        grp = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1, 2)
        if len(idx) % 3:
            raise ValueError("build_blas: three indices per triangle")
        n_words = 8 * int((2 * grp[:, 1].astype(np.int64) - 1).clip(min=0).sum())
        nodes = np.zeros(n_words, np.uint32)
        out_idx = np.zeros(len(idx), np.uint32)
        counts = np.zeros(len(grp), np.uint32)
        depth = ctypes.c_uint32(0)
        d = N.PtxBlasDesc(positions=pos.ctypes.data, n_vertices=len(pos), indices=idx.ctypes.data, n_tris=len(idx) // 3,
                          groups=grp.ctypes.data if len(grp) else None, n_groups=len(grp), max_leaf=int(max_leaf_tris))
        d.reserved[0] = self._BLAS_BUILDERS[builder]
        self._call("ptx_build_blas", self._h, ctypes.byref(d), nodes.ctypes.data if n_words else None, n_words,
                   out_idx.ctypes.data, counts.ctypes.data if len(grp) else None, ctypes.addressof(depth))
        ends = 8 * np.cumsum(counts.astype(np.int64))
        roots = [nodes[e - 8 * int(c):e].copy() for e, c in zip(ends, counts)]
        return roots, out_idx, int(depth.value)

    _BLAS_BUILDERS = {"lbvh": N.PTX_BLAS_LBVH, "sah": N.PTX_BLAS_SAH}

    def build_blas_sah(self, positions, indices, groups, max_leaf_tris: int = 10):
        """build_blas with the SAH builder, in build_blas' own signature:
        compile_scene(name, builder=renderer.build_blas_sah)."""
        return self.build_blas(positions, indices, groups, max_leaf_tris, builder="sah")

    def RebuildMesh(self, mesh: int, builder: str = "sah", max_leaf_tris: int = 10) -> dict:
        """Build mesh `mesh`'s BLAS again from the vertex records the device holds now and splice it into the
        handle (ptx_rebuild_mesh; scene.world.rebuild_mesh is the rule): after a pose far from the one the tree
        was built for, where a refit leaves inflated boxes.  Skins, the accumulation and the denoiser's history
        stay, the reuse history is dropped (include/ptx.h).  Returns the call's info (n_accel, mesh_nodes,
        max_depth, scene_words); `compiled` is afterwards read_scene()'s arrays with max_bvh_depth updated.
        A refused call (PtxError) changes nothing."""
        if builder not in self._BLAS_BUILDERS:
            raise ValueError(f"RebuildMesh: builder {builder!r} (one of {sorted(self._BLAS_BUILDERS)})")
        if self.compiled is None or self.uniform is None:
            raise ValueError("RebuildMesh: Initialize and Update first")
        info = N.PtxRebuildInfo()
        self._call("ptx_rebuild_mesh", self._h, int(mesh), self._BLAS_BUILDERS[builder], int(max_leaf_tris), ctypes.byref(info))
        scene, geometry, accel = self.read_scene()
        self.compiled = dataclasses.replace(self.compiled, scene=scene, geometry=geometry, accel=accel,
                                            max_bvh_depth=self.stats()["max_bvh_depth"])
        return {k: int(getattr(info, k)) for k in ("n_accel", "mesh_nodes", "max_depth", "scene_words")}

    def read_scene(self):
        """(scene, geometry, accel) u32 arrays as the handle renders them now (ptx_read_scene): the scene array
        with edits and shifted descriptors, the geometry with every posed vertex block read from the device,
        the accel array as read_accel() returns it."""
        n = [ctypes.c_size_t(0) for _ in range(3)]
        self._call("ptx_scene_sizes", self._h, *[ctypes.byref(k) for k in n])
        out = [np.zeros(int(k.value), dtype=np.uint32) for k in n]
        args = []
        for a in out:
            args += [a.ctypes.data if len(a) else None, len(a)]
        self._call("ptx_read_scene", self._h, *args)
        return tuple(out)

    def blas_cost(self, mesh: int) -> float:
        """The surface-area cost of mesh `mesh`'s trees as the device holds them now (ptx_blas_cost;
        scene.world.mesh_cost is the rule): it grows as refits inflate the boxes, and tells when RebuildMesh pays."""
        cost = ctypes.c_double(0.0)
        self._call("ptx_blas_cost", self._h, int(mesh), ctypes.byref(cost))
        return float(cost.value)

    def SetSkin(self, mesh: int, joints, weights, bind=None, targets=None, target_normals=None, first: int = 0) -> None:
        """Bind a skin to vertices [first, first + n) of mesh `mesh` (ptx_set_skin): `joints` (n, 4) integers,
        `weights` (n, 4) f32, `bind` (n, 6) f32 {p, n} (None: the records as the handle holds them now),
        `targets` (T, n, 3) f32 morph position deltas, `target_normals` the same shape.  n == 0 removes the
        mesh's skin.  Nothing a frame reads changes; a refused call (PtxError) binds nothing."""
        if self.compiled is None or self.uniform is None:
            raise ValueError("SetSkin: Initialize and Update first")
        j = np.ascontiguousarray(joints, dtype=np.uint32).reshape(-1, 4)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 4)
        if len(j) != len(w):
            raise ValueError("SetSkin: four joints and four weights per vertex")
        n = len(j)
        keep = [j, w]

        def table(a, shape, what):
            if a is None:
                return None, 0
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != len(shape) or a.shape[1:] != shape[1:]:
                raise ValueError(f"SetSkin: {what} must have the shape {shape}")
            keep.append(a)
            return a.ctypes.data if a.size else None, len(a)
        b, nb = table(bind, (n, 6), "bind")
        if bind is not None and nb != n:
            raise ValueError("SetSkin: one bind record per vertex")
        tp, nt = table(targets, (0, n, 3), "targets")
        tn, ntn = table(target_normals, (0, n, 3), "target_normals")
        if target_normals is not None and ntn != nt:
            raise ValueError("SetSkin: one table of normal deltas per target")
        n_joints = int(j.max()) + 1 if n else 1
        d = N.PtxSkinDesc(mesh=int(mesh), first_vertex=int(first), n_vertices=n, n_joints=n_joints, n_targets=nt,
                          joints=j.ctypes.data if n else None, weights=w.ctypes.data if n else None, bind=b,
                          target_pos=tp, target_nrm=tn)
        self._call("ptx_set_skin", self._h, ctypes.byref(d))
        if n:
            self._skins[int(mesh)] = (int(first), n, n_joints, nt)
        else:
            self._skins.pop(int(mesh), None)

    def SkinVertices(self, mesh: int, palette, target_weights=None) -> None:
        """Pose the skinned range of mesh `mesh` and refit its BLAS on the GPU (ptx_skin_vertices): `palette`
        (J, 12) f32 with J at least the skin's joint count (1 + the largest bound index), `target_weights`
        one f32 per bound morph target.  `compiled` is afterwards what the handle renders: the range's
        records read_vertices()'s, the accel array read_accel()'s.  A refused call changes nothing."""
        if int(mesh) not in self._skins:
            raise ValueError(f"SkinVertices: mesh {mesh} has no skin")
        first, n, n_joints, nt = self._skins[int(mesh)]
        pal = np.ascontiguousarray(palette, dtype=np.float32).reshape(-1, 12)
        if len(pal) < n_joints:
            raise ValueError(f"SkinVertices: {len(pal)} matrices for {n_joints} joints")
        tw = None if target_weights is None else np.ascontiguousarray(target_weights, dtype=np.float32).reshape(-1)
        if (tw is None) != (nt == 0) or (tw is not None and len(tw) != nt):
            raise ValueError(f"SkinVertices: the skin has {nt} morph targets")
        self._call("ptx_skin_vertices", self._h, int(mesh), pal.ctypes.data, None if tw is None else tw.ctypes.data)
        from .scene.world import STRIDE_VERTEX, mesh_blocks
        cs = self.compiled
        w0 = mesh_blocks(cs, int(mesh))["vertex"] + STRIDE_VERTEX * first
        geometry = np.array(cs.geometry, dtype=np.uint32)
        geometry[w0:w0 + STRIDE_VERTEX * n] = self.read_vertices(mesh, first, n).reshape(-1)
        self.compiled = dataclasses.replace(cs, geometry=geometry, accel=self.read_accel())

    def read_vertices(self, mesh: int, first: int = 0, n: int | None = None) -> np.ndarray:
        """(n, 8) u32: the device's current records of vertices [first, first + n) of mesh `mesh`
        (ptx_read_vertices; n None: to the end of the mesh's vertex block)."""
        from .scene.world import STRIDE_VERTEX, mesh_blocks
        if n is None:
            b = mesh_blocks(self.compiled, int(mesh))
            n = (b["vertex_end"] - b["vertex"]) // STRIDE_VERTEX - first
        out = np.zeros((max(int(n), 0), STRIDE_VERTEX), dtype=np.uint32)
        self._call("ptx_read_vertices", self._h, int(mesh), int(first), len(out), out.ctypes.data if len(out) else None)
        return out

    def Update(self) -> None:
        """Renderer_TEST.Update: FrameCount++ and the 33-word uniform block."""
        self.frame_count += 1
        u = self.compiled.uniform(self.width, self.height, self.camera.view_projection_inverse(),
                                  self.camera.location, self.frame_count)
        self.set_uniform(u)

    def Render(self) -> None:
        """Renderer_TEST.Render: the configured passes, accumulated into the Scene texture."""
        self._call("ptx_render", self._h, None)

    # ------------------------------------------------------------------ extras
    def set_uniform(self, u: np.ndarray) -> None:
        self.uniform = np.ascontiguousarray(u, dtype=np.uint32)
        self._call("ptx_set_frame", self._h, self.uniform.ctypes.data)

    def run_pass(self, pass_id: int) -> None:
        self._call("ptx_run_pass", self._h, pass_id)

    def run_passes(self, passes) -> None:
        """Several passes as one overlapped launch sequence (include/ptx.h ptx_run_passes)."""
        arr = (ctypes.c_int * len(passes))(*passes)
        self._call("ptx_run_passes", self._h, arr, len(passes))

    def halo_rows(self):
        """(rows above, rows below, bytes per halo row) of a reuse band (ptx_halo_rows)."""
        t, b, n = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_size_t()
        self._call("ptx_halo_rows", self._h, ctypes.byref(t), ctypes.byref(b), ctypes.byref(n))
        return int(t.value), int(b.value), int(n.value)

    def halo_pack(self, dev_top: int | None, dev_bottom: int | None) -> None:
        self._call("ptx_halo_pack", self._h, dev_top, dev_bottom)

    def halo_unpack(self, dev_top: int | None, dev_bottom: int | None) -> None:
        self._call("ptx_halo_unpack", self._h, dev_top, dev_bottom)

    # ------------------------------------------------------------------ multi-GPU (include/ptx.h)
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId: made on one rank, shipped to the others by the caller."""
        lib = N.load()
        buf = ctypes.create_string_buffer(N.PTX_COMM_ID_BYTES)
        rc = lib.ptx_comm_unique_id(buf, N.PTX_COMM_ID_BYTES)
        if rc != N.PTX_OK:
            raise N.PtxError(f"ptx_comm_unique_id failed ({rc}): is RCCL installed?")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """The handle's own RCCL communicator: Render() then exchanges the halo itself."""
        buf = ctypes.create_string_buffer(bytes(unique_id), N.PTX_COMM_ID_BYTES)
        self._call("ptx_comm_init", self._h, buf, N.PTX_COMM_ID_BYTES, rank, world)

    def comm_info(self) -> dict:
        """The handle's communicator: rank, world size (1 without one), halo bytes sent so far."""
        rank, world, sent = ctypes.c_int(0), ctypes.c_int(1), ctypes.c_uint64(0)
        self._call("ptx_comm_info", self._h, ctypes.byref(rank), ctypes.byref(world), ctypes.byref(sent))
        return {"rank": rank.value, "world": world.value, "halo_bytes_sent": sent.value}

    @staticmethod
    def comm_init_all(renderers) -> None:
        """ncclCommInitAll over the band renderers of this process (one per GPU)."""
        arr = (ctypes.c_void_p * len(renderers))(*[r._h.value for r in renderers])
        lib = N.load()
        N.check(lib, renderers[0]._h, lib.ptx_comm_init_all(arr, len(renderers)), "ptx_comm_init_all")

    @staticmethod
    def render_bands(renderers, out: np.ndarray | None = None) -> None:
        """One frame over the band renderers of this process, halo exchanged on the device
        (their communicators, or peer copies); `out` (rows of all bands, W, 4) f32 optional."""
        arr = (ctypes.c_void_p * len(renderers))(*[r._h.value for r in renderers])
        lib = N.load()
        ptr = None
        if out is not None:
            rows = sum(r.band_rows for r in renderers)
            assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == rows * renderers[0].width * 4
            ptr = out.ctypes.data
        rc = lib.ptx_render_bands(arr, len(renderers), ptr)
        if rc != N.PTX_OK:
            msgs = [lib.ptx_last_error(r._h) for r in renderers]
            raise N.PtxError(f"ptx_render_bands failed ({rc}): "
                             + "; ".join(m.decode(errors="replace") for m in msgs if m))

    def row_census(self) -> np.ndarray:
        """(tile rows, 5) u64 {rays, instance transforms, AABB tests, triangle tests, hits}
        per 8-row tile row of the band (handle made with row_census=True)."""
        out = np.zeros(((self.band_rows + 7) // 8, 5), dtype=np.uint64)
        self._call("ptx_row_census", self._h, out.ctypes.data, out.shape[0])
        return out

    @property
    def reservoir_words(self) -> int:
        """32 (the reference's 128-byte Reservoir) or 16 (the GI reservoir)."""
        return 16 if self.pipeline == "gi" else 32

    def read_history(self) -> np.ndarray:
        """The reuse / GI pipeline's spatial output (final pass input, next frame's history)."""
        return self._read(N.PTX_BUF_RESERVOIR_HIST, np.uint32, self.reservoir_words)

    def read_direct(self) -> np.ndarray:
        """The GI init pass's direct light (band_h, W, 4) f32."""
        return self._read(N.PTX_BUF_DIRECT, np.float32, 4)

    def synchronize(self) -> None:
        self._call("ptx_synchronize", self._h)

    def reset_accumulation(self) -> None:
        self._call("ptx_reset_accumulation", self._h)

    @property
    def band_rows(self) -> int:
        return self.row_end - self.row_begin

    def _read(self, which: int, dtype, comps: int) -> np.ndarray:
        out = np.zeros((self.band_rows, self.width, comps), dtype=dtype)
        self._call("ptx_read_buffer", self._h, which, out.ctypes.data, out.nbytes)
        return out

    def read_image(self) -> np.ndarray:
        return self._read(N.PTX_BUF_ACCUM, np.float32, 4)

    def read_gbuffer(self) -> np.ndarray:
        return self._read(N.PTX_BUF_GBUFFER, np.uint32, 4)

    def read_reservoir(self) -> np.ndarray:
        return self._read(N.PTX_BUF_RESERVOIR, np.uint32, self.reservoir_words)

    def write_buffer(self, which: int, arr: np.ndarray) -> None:
        arr = np.ascontiguousarray(arr)
        self._call("ptx_write_buffer", self._h, which, arr.ctypes.data, arr.nbytes)

    def read_counters(self) -> dict:
        c = np.zeros(32, dtype=np.uint64)
        self._call("ptx_read_buffer", self._h, N.PTX_BUF_COUNTERS, c.ctypes.data, c.nbytes)
        # cull_misses: queries of the counting build whose instance cull would have skipped an
        # instance with a root its pre-filter passes (the cull's conservativeness check: always 0)
        return {"rays": int(c[0]), "instance_xforms": int(c[1]), "aabb_tests": int(c[2]), "tri_tests": int(c[3]),
                "hits": int(c[4]), "cull_misses": int(c[5]),
                # motion_clips (every build): pixels of a moved camera's frames whose reprojection
                # fell past a band's motion halo (no history there; 0 keeps bands bit-identical)
                "motion_clips": int(c[N.PTX_COUNTER_MOTION_CLIP]),
                # replays (every build): pixels whose spatial output carried no contribution when
                # the spatial pass shaded them itself, so PT_4 replayed their paths
                "replays": int(c[N.PTX_COUNTER_REPLAY])}

    def stats(self) -> dict:
        s = N.PtxStats()
        self._call("ptx_get_stats", self._h, ctypes.byref(s))
        return {"frames": s.frames, "kernel_ms_total": list(s.kernel_ms_total),
                "kernel_launches": list(s.kernel_launches), "triangles": s.triangles, "bvh_nodes": s.bvh_nodes,
                "instances": s.instances, "max_bvh_depth": s.max_bvh_depth, "device_bytes": s.device_bytes}

    def Present(self, canvas_w: int | None = None, canvas_h: int | None = None, bgra: bool = False) -> np.ndarray:
        """The reference's render pass (Renderer_TEST.Render's fullscreen quad + FragmentShader.wgsl)
        onto a canvas_w x canvas_h canvas (default: the image size): (canvas_h, canvas_w, 4) uint8,
        RGBA (a 2D canvas's ImageData) or BGRA (a bgra8unorm WebGPU canvas); include/ptx.h ptx_present."""
        cw, ch = int(canvas_w or self.width), int(canvas_h or self.height)
        out = np.zeros((ch, cw, 4), np.uint8)
        self._call("ptx_present", self._h, cw, ch, 1 if bgra else 0, out.ctypes.data)
        return out

    def present_async(self, canvas_w: int | None = None, canvas_h: int | None = None, bgra: bool = False) -> None:
        """Enqueue Present for the frame last rendered without waiting (ptx_present_async);
        present_poll() returns the bytes once they have landed."""
        cw, ch = int(canvas_w or self.width), int(canvas_h or self.height)
        self._call("ptx_present_async", self._h, cw, ch, 1 if bgra else 0)
        self._present_shape = (ch, cw, 4)

    def present_poll(self) -> np.ndarray | None:
        """The bytes of the present in flight, or None while it is still running (never waits)."""
        out = np.zeros(self._present_shape, np.uint8)
        rc = self._lib.ptx_present_poll(self._h, out.ctypes.data, out.nbytes)
        if rc == N.PTX_E_PENDING:
            return None
        N.check(self._lib, self._h, rc, "ptx_present_poll")
        return out

    def Denoise(self, iterations: int = 0, sigma_lum: float = 0.0, sigma_plane: float = 0.0,
                temporal: bool | int = False, alpha_min: float = 0.0) -> None:
        """Enqueue the edge-avoiding a-trous filter of the accumulated image behind the frame last
        rendered (ptx_denoise; 0 = the defaults: 5 iterations, sigma_lum 4, sigma_plane 0.02);
        read_denoised() or Present with source "denoised" show the result.  temporal (a renderer
        made with frame_color=True): filter the frame colours integrated over the calls instead,
        their history reprojected across camera moves; alpha_min (0 = 0.05) is the least weight of
        the new frame.  With the renderer's `follow_vertices` set (an attribute, False by default; read by
        every temporal call), a pixel on a mesh that UpdateVertices / SkinVertices deformed since the previous
        temporal call looks its history up where that surface point was then (ptx_denoise_params.reserved[2])."""
        p = N.PtxDenoiseParams(iterations=int(iterations), sigma_lum=float(sigma_lum), sigma_plane=float(sigma_plane))
        p.reserved[0] = int(temporal)
        p.reserved[1] = int(np.float32(alpha_min).view(np.uint32))
        p.reserved[2] = int(self.follow_vertices)
        self._call("ptx_denoise", self._h, ctypes.byref(p))

    def Upsample(self, lo: "Renderer", sigma_plane: float = 0.0) -> None:
        """Write the denoised image of `lo` -- a renderer of 1/2, 1/3 or 1/4 this one's size with the same
        scene and camera, after its Denoise() -- at this renderer's size, steered by this renderer's
        G-buffer as it stands (ptx_upsample; run_pass(PTX_PASS_GBUFFER) or a frame first; sigma_plane
        0 = 0.02).  read_denoised() or Present with source "denoised" show the result."""
        p = N.PtxUpsampleParams(sigma_plane=float(sigma_plane))
        self._call("ptx_upsample", self._h, lo._h, ctypes.byref(p))

    def UpsampleTemporal(self, lo: "Renderer", px: int, py: int, sigma_plane: float = 0.0, alpha_min: float = 0.0,
                         alpha_fill: float = -1.0) -> None:
        """Upsample for a `lo` whose frame was rendered through phase (px, py) of every s x s block of this
        renderer's pixels (lo.set_phase_of(self, s, px, py) before its frame), integrated over the calls:
        each small pixel's value goes where it was sampled, the rest is interpolated, and the history
        follows camera moves (ptx_upsample_temporal).  alpha_min (0 = 0.02): the least weight of a new own
        sample; alpha_fill (negative = 0.05, 0 = none): the weight of the interpolated estimate on a pixel
        not sampled this call.  read_denoised() / read_upsample_history() show the result."""
        p = N.PtxUpsampleTemporalParams(sigma_plane=float(sigma_plane), px=int(px), py=int(py), alpha_min=float(alpha_min),
                                        alpha_fill=float(alpha_fill))
        self._call("ptx_upsample_temporal", self._h, lo._h, ctypes.byref(p))

    def set_upsample_follow(self, on: bool | int) -> None:
        """Switch this full-size renderer's UpsampleTemporal / upsample_temporal_bands to follow moved instances
        and deformed or skinned meshes (ptx_upsample_follow): from the first call made with it on, UpdateScene,
        UpdateVertices and SkinVertices keep the history, and the next call looks a moved surface's history up
        where it was.  Off (the default): an instance edit and a vertex update drop the history.  No GPU work."""
        self._call("ptx_upsample_follow", self._h, int(on))
        self._upsample_follow = bool(on)

    @property
    def upsample_follow(self) -> bool:
        """The switch set_upsample_follow last set."""
        return self._upsample_follow

    def set_phase_of(self, hi: "Renderer", s: int, px: int, py: int) -> None:
        """Set this (small) renderer's uniform to the one that looks through pixel (px, py) of every s x s
        block of `hi`'s current frame (ptx_phase_uniform); the frame index is hi's."""
        self.set_uniform(N.phase_uniform(hi.uniform, s, px, py, self._lib))

    def read_upsample_history(self) -> np.ndarray:
        """The last UpsampleTemporal's integrated colour and own-sample count (H, W, 4) f32 {H.rgb, n}."""
        return self._read(N.PTX_BUF_UPSAMPLE_HISTORY, np.float32, 4)

    @staticmethod
    def denoise_bands(renderers, out: np.ndarray | None = None, iterations: int = 0, sigma_lum: float = 0.0,
                      sigma_plane: float = 0.0, temporal: bool | int = False, alpha_min: float = 0.0) -> None:
        """Denoise over the band renderers of this process (ptx_denoise_bands): every band filters its
        rows and 2^(iterations + 1) halo rows brought from its neighbours on the device (their
        communicators, or peer copies), which gives the whole image's result on its rows.  Parameters as
        Denoise; `out` (rows of all bands, W, 4) f32 optional: the bands' denoised rows in order
        (blocking).  read_denoised / read_denoise_history / denoise_clips work per band."""
        lib = N.load()
        arr = (ctypes.c_void_p * len(renderers))(*[r._h.value for r in renderers])
        p = N.PtxDenoiseParams(iterations=int(iterations), sigma_lum=float(sigma_lum), sigma_plane=float(sigma_plane))
        p.reserved[0] = int(temporal)
        p.reserved[1] = int(np.float32(alpha_min).view(np.uint32))
        follow = {int(r.follow_vertices) for r in renderers}  # (every band tracks for itself: each makes the same vertex calls)
        if len(follow) > 1:
            raise ValueError("denoise_bands: follow_vertices differs between the bands")
        p.reserved[2] = follow.pop() if follow else 0
        if out is not None:
            rows = sum(r.band_rows for r in renderers)
            assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == rows * renderers[0].width * 4
        rc = lib.ptx_denoise_bands(arr, len(renderers), ctypes.byref(p))
        if rc != N.PTX_OK:
            msgs = [lib.ptx_last_error(r._h) for r in renderers]
            raise N.PtxError(f"ptx_denoise_bands failed ({rc}): "
                             + "; ".join(m.decode(errors="replace") for m in msgs if m))
        if out is not None:
            flat, row = out.reshape(rows, renderers[0].width, 4), 0
            for r in renderers:
                flat[row:row + r.band_rows] = r.read_denoised()
                row += r.band_rows

    @staticmethod
    def upsample_bands(his, los, sigma_plane: float = 0.0) -> None:
        """Upsample over band pairs of this process (ptx_upsample_bands): los[i] is a band of the small
        frame after denoise_bands, his[i] the band of s times its rows of the full-size frame on the same
        device, with a G-buffer; each pair reads 2 rows of its neighbours' denoised images, brought on the
        device (the small bands' communicators, or peer copies), which gives the whole-image Upsample's
        result on its rows.  read_denoised works per full-size band."""
        assert len(his) == len(los)
        lib = N.load()
        a = (ctypes.c_void_p * len(his))(*[r._h.value for r in his])
        b = (ctypes.c_void_p * len(los))(*[r._h.value for r in los])
        p = N.PtxUpsampleParams(sigma_plane=float(sigma_plane))
        rc = lib.ptx_upsample_bands(a, b, len(his), ctypes.byref(p))
        if rc != N.PTX_OK:
            msgs = [lib.ptx_last_error(r._h) for r in list(his) + list(los)]
            raise N.PtxError(f"ptx_upsample_bands failed ({rc}): "
                             + "; ".join(m.decode(errors="replace") for m in msgs if m))

    @staticmethod
    def upsample_temporal_bands(his, los, px: int, py: int, sigma_plane: float = 0.0, alpha_min: float = 0.0,
                                alpha_fill: float = -1.0, history_rows: int = 0) -> None:
        """UpsampleTemporal over band pairs of this process (ptx_upsample_temporal_bands): los[i] is a band of
        the small frame after denoise_bands, rendered through phase (px, py) (los[i].set_phase_of(his[i], s,
        px, py) before its frame), his[i] the band of s times its rows of the full-size frame.  Each pair
        reads 2 rows of its neighbours' denoised images and history_rows (0 = 32, at most 128) rows of
        their previous state, brought on the device; a history tap past those rows is not taken and counts
        in upsample_clips().  With no clips the bands' rows are the whole-image UpsampleTemporal's.
        read_denoised / read_upsample_history work per full-size band."""
        assert len(his) == len(los)
        if len({r.upsample_follow for r in his}) > 1:  # (every band tracks for itself: each makes the same edits)
            raise ValueError("upsample_temporal_bands: upsample_follow differs between the bands")
        lib = N.load()
        a = (ctypes.c_void_p * len(his))(*[r._h.value for r in his])
        b = (ctypes.c_void_p * len(los))(*[r._h.value for r in los])
        p = N.PtxUpsampleTemporalParams(sigma_plane=float(sigma_plane), px=int(px), py=int(py), alpha_min=float(alpha_min),
                                        alpha_fill=float(alpha_fill))
        p.reserved[0] = int(history_rows)
        rc = lib.ptx_upsample_temporal_bands(a, b, len(his), ctypes.byref(p))
        if rc != N.PTX_OK:
            msgs = [lib.ptx_last_error(r._h) for r in list(his) + list(los)]
            raise N.PtxError(f"ptx_upsample_temporal_bands failed ({rc}): "
                             + "; ".join(m.decode(errors="replace") for m in msgs if m))

    def upsample_clips(self) -> int:
        """Pixels of this full-size band's upsample_temporal_bands calls (since the last reset_stats) with a
        history candidate inside the image but outside the rows the band's state covered: not taken.  0 on
        every band: the split is the whole image's bit for bit (PTX_COUNTER_UPSAMPLE_CLIP)."""
        c = np.zeros(N.PTX_COUNTER_UPSAMPLE_CLIP + 1, dtype=np.uint64)
        self._call("ptx_read_buffer", self._h, N.PTX_BUF_COUNTERS, c.ctypes.data, c.nbytes)
        return int(c[N.PTX_COUNTER_UPSAMPLE_CLIP])

    def denoise_clips(self) -> int:
        """Pixels of this band's temporal denoise_bands calls (since the last reset_stats) with a history
        candidate inside the image but outside the rows the band's state covered: not taken.  0 on every
        band: the split is the whole image's bit for bit (PTX_COUNTER_DENOISE_CLIP)."""
        c = np.zeros(8, dtype=np.uint64)
        self._call("ptx_read_buffer", self._h, N.PTX_BUF_COUNTERS, c.ctypes.data, c.nbytes)
        return int(c[N.PTX_COUNTER_DENOISE_CLIP])

    def read_frame_color(self) -> np.ndarray:
        """The radiance of the frame last rendered alone (band_h, W, 4) f32 {r, g, b, 1}
        (frame_color=True; unspecified at pixels without a primary hit)."""
        return self._read(N.PTX_BUF_FRAME_COLOR, np.float32, 4)

    def read_denoise_history(self) -> np.ndarray:
        """The last temporal Denoise's integrated colour and history length (band_h, W, 4) f32 {C.rgb, n}."""
        return self._read(N.PTX_BUF_DENOISE_HISTORY, np.float32, 4)

    def read_denoised(self) -> np.ndarray:
        """The denoised image (band_h, W, 4) f32: rgb after the last iteration, alpha 1."""
        return self._read(N.PTX_BUF_DENOISED, np.float32, 4)

    def set_present_source(self, source: str) -> None:
        """What Present / present_async show: "accum" (the default) or "denoised"."""
        which = {"accum": N.PTX_BUF_ACCUM, "denoised": N.PTX_BUF_DENOISED}[source]
        self._call("ptx_present_source", self._h, which)

    def trace(self, rays: np.ndarray, eps_mode: int = 1) -> np.ndarray:
        """Closest hits for an (n, 8) f32 ray array {o.xyz, d.xyz, -, -}; returns (n, 8) f32
        {t, flags|inst|mat bits, prim bits, bary.x, bary.y, pos.xyz} (include/ptx.h)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        hits = np.zeros_like(rays)
        self._call("ptx_trace", self._h, rays.ctypes.data, hits.ctypes.data, len(rays), eps_mode)
        return hits

    def trace_queries(self, queries: np.ndarray, eps_mode: int = 1, occ_only: bool = False) -> np.ndarray:
        """Queries through the kernel this renderer's frames trace with (ptx_trace_queries; trace() runs
        a kernel of its own): (n, 8) f32 {o.xyz, remain, d.xyz, kind}, kind the u32 bit pattern 0 closest
        hit, 1 Visibility, 2 occlusion; returns (n, 8) f32 -- trace()'s hit record for a closest query,
        {transmittance, 0 x 7} for the others.  occ_only: the any-hit kernel (every query of kind 2)."""
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 8)
        out = np.zeros_like(queries)
        self._call("ptx_trace_queries", self._h, queries.ctypes.data, out.ctypes.data, len(queries), int(eps_mode),
                   1 if occ_only else 0)
        return out

    def reset_stats(self) -> None:
        self._call("ptx_reset_stats", self._h)

    def set_stream(self, stream_ptr: int | None) -> None:
        self._call("ptx_set_stream", self._h, stream_ptr)

    def close(self) -> None:
        if self._h:
            self._lib.ptx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name: str, *args):
        N.check(self._lib, self._h, getattr(self._lib, name)(*args), name)
