"""numpy restatement of vertex motion in the denoiser's temporal lookup (include/ptx.h ptx_denoise,
"Vertex motion"; DESIGN.md §4.6 "Following vertices"), built on tests/denoise_motion_ref.py.

Test infrastructure only: the checker of dn_temporal_verts in pathtracerdemo_amd/csrc/ptx_denoise.hip.
A call takes, beside MotionDenoiser's inputs, the scene, geometry and accel arrays the frame was rendered
from, the frame's G-buffer, and the meshes that ptx_update_vertices / ptx_skin_vertices were called on since
the previous temporal call (`deformed`).  The class keeps the previous call's arrays: its geometry is what
the library's snapshot holds, the shape that call saw, however many updates followed.

While the previous temporal call followed too (the handle is tracking) an instance whose mesh word is that
call's and whose mesh is in `deformed` gets flag 3, whatever became of its matrices; every other instance
keeps MotionDenoiser's flag.  A hit pixel of a flag-3 instance takes Q and Nq from GetSurface
(tests/wgsl_ref.py through denoise_ref.guides_from_gbuffer) of this frame's texel on the previous call's
scene and geometry arrays, and then runs flag 1's lookup: Q always reprojected, the taps tested against Q
and Nq with this pixel's r.  With no flag 3 the call is MotionDenoiser's, by the same code.
"""
from __future__ import annotations

import numpy as np

import denoise_motion_ref as M
import denoise_ref as D

f32 = np.float32
STRIDE = M.STRIDE


class FollowDenoiser(M.MotionDenoiser):
    def __init__(self):
        super().__init__()
        self.tracking = False  # the last temporal call had follow=True
        self.prev = None       # (scene, geometry, accel) of the previous temporal call
        self._follow = None    # of a call with a flag 3: (Q, Nq) per pixel

    def reset(self):
        super().reset()
        self.prev = None

    def denoise(self, frame_color, accum, G, uniform, insts=None, temporal=True, follow=True, scene=None,
                geometry=None, accel=None, gbuffer=None, deformed=(), **kw):
        if not temporal:
            return super().denoise(frame_color, accum, G, uniform, temporal=False, **kw)
        insts = np.ascontiguousarray(insts, np.uint32).copy()
        flags3 = None
        if follow and self.tracking and self.state is not None and self.insts is not None \
                and len(self.insts) == len(insts) and self.prev is not None:
            p, c = self.insts.reshape(-1, STRIDE), insts.reshape(-1, STRIDE)
            marked = np.array([p[i, 32] == c[i, 32] and int(c[i, 32]) in set(deformed) for i in range(len(c))], bool)
            if marked.any():
                flags3 = marked
        self._follow = None
        if flags3 is None:
            out = super().denoise(frame_color, accum, G, uniform, insts=insts, **kw)
        else:
            # MotionDenoiser.denoise with the table made here: its flags where an instance is not marked
            if not np.array_equal(self.insts, insts):
                flags, Ds = M.object_table(self.insts, insts)
            else:
                flags, Ds = np.zeros(len(flags3), np.int64), np.zeros((len(flags3), 16), np.float32)
            flags = np.where(flags3, 3, flags)
            self._obj, self.flags = (flags, Ds), flags
            # Q, Nq of the flag-3 pixels: GetSurface of this frame's texel in the previous call's arrays
            g = np.array(gbuffer, np.uint32)
            pf, _ = self.pixel_flags(G)
            g[..., 0] = np.where(pf == 3, g[..., 0], g[..., 0] & np.uint32(0x7FFFFFFF))  # (the others: no hit, skipped)
            Gp = D.guides_from_gbuffer(uniform, self.prev[0], self.prev[1], self.prev[2], g)
            self._follow = (Gp.P, Gp.N)
            out = M.T.TemporalDenoiser.denoise(self, frame_color, accum, G, uniform, **kw)
            self.insts = insts
        self.tracking = bool(follow)
        self.prev = tuple(np.array(a, np.uint32) for a in (scene, geometry, accel)) if scene is not None else None
        return out

    def _lookup(self, G, camera):
        if self._follow is None:
            return super()._lookup(G, camera)
        # MotionDenoiser._lookup with flag 3 beside flag 1: the same reprojection of another Q, Nq
        H, W = G.key.shape
        s = self.state
        pf, inst = self.pixel_flags(G)
        Dm = self._obj[1][inst]
        P, N = G.P, G.N
        rigid, verts = pf == 1, pf == 3
        follow = rigid | verts
        Q = np.stack([((Dm[..., 0 + r] * P[..., 0] + Dm[..., 4 + r] * P[..., 1]) + Dm[..., 8 + r] * P[..., 2])
                      + Dm[..., 12 + r] for r in range(3)], -1).astype(np.float32)
        Nq = np.stack([(Dm[..., 0 + r] * N[..., 0] + Dm[..., 4 + r] * N[..., 1]) + Dm[..., 8 + r] * N[..., 2]
                       for r in range(3)], -1).astype(np.float32)
        Q = np.where(rigid[..., None], Q, np.where(verts[..., None], self._follow[0], P))
        Nq = np.where(rigid[..., None], Nq, np.where(verts[..., None], self._follow[1], N))
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        same_cam = np.array_equal(camera, s.camera)
        self.same_pixel = same_cam
        same = np.full((H, W), same_cam) & ~follow
        vp = s.vp
        cx = ((vp[0] * Q[..., 0] + vp[4] * Q[..., 1]) + vp[8] * Q[..., 2]) + vp[12]
        cy = ((vp[1] * Q[..., 0] + vp[5] * Q[..., 1]) + vp[9] * Q[..., 2]) + vp[13]
        cw = ((vp[3] * Q[..., 0] + vp[7] * Q[..., 1]) + vp[11] * Q[..., 2]) + vp[15]
        fx = ((cx / cw + f32(1)) * f32(0.5)) * f32(W) - f32(0.5)
        fy = ((cy / cw + f32(1)) * f32(0.5)) * f32(H) - f32(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        runs = G.hit & (pf != 2) & (same | (cw > 0))
        sw = np.zeros((H, W), np.float32)
        sC = np.zeros((H, W, 3), np.float32)
        s1 = np.zeros((H, W), np.float32)
        s2 = np.zeros((H, W), np.float32)
        nh = np.full((H, W), np.inf, np.float32)
        taken_any = np.zeros((H, W), bool)
        self.taps = np.where(runs, 0, -1)
        k = 0
        for j in (0, 1):
            for i in (0, 1):
                qxf, qyf = x0 + f32(i), y0 + f32(j)
                inside = (qxf >= 0) & (qxf < f32(W)) & (qyf >= 0) & (qyf < f32(H))
                w = ((ax if i else f32(1) - ax) * (ay if j else f32(1) - ay)).astype(np.float32)
                inside = np.where(same, k == 0, inside)
                w = np.where(same, f32(1), w).astype(np.float32)
                qx = np.where(same, xs, np.where(inside, qxf, 0).astype(np.int64))
                qy = np.where(same, ys, np.where(inside, qyf, 0).astype(np.int64))
                kq, nq = s.G.key[qy, qx], s.n[qy, qx]
                ok = runs & inside & (kq == G.key) & (nq >= 1)
                ok &= D.dot3(Nq, s.G.N[qy, qx]) >= f32(0.9)
                ok &= np.abs(D.dot3(Nq, s.G.P[qy, qx] - Q)) <= G.r
                sw = np.where(ok, sw + w, sw)
                sC = np.where(ok[..., None], sC + w[..., None] * s.C[qy, qx], sC)
                s1 = np.where(ok, s1 + w * s.m1[qy, qx], s1)
                s2 = np.where(ok, s2 + w * s.m2[qy, qx], s2)
                nh = np.where(ok, np.minimum(nh, nq), nh)
                taken_any |= ok
                self.taps = self.taps + ok
                k += 1
        have = taken_any & (sw > 0)
        return have, sC / sw[..., None], s1 / sw, s2 / sw, nh
