"""numpy restatement of following in the temporal upsampler (include/ptx.h ptx_upsample_follow; DESIGN.md §4.6
"Following in the temporal upsampler"), built on tests/upsample_temporal_ref.py's TemporalUpsampler,
tests/denoise_motion_ref.py's object_table and the snapshot evaluation of tests/denoise_follow_ref.py.

Test infrastructure only: the checker of dn_upsample_temporal<S, FOLLOW> (pathtracerdemo_amd/csrc/ptx_denoise.hip)
and of the handle's bookkeeping (ptx_api.cpp upsample_follow_table), whose outputs must equal these bit for bit.

A call takes, beside TemporalUpsampler's inputs, the switch (`follow`), the scene, geometry and accel arrays
hi's G-buffer was traced in, that G-buffer, and the meshes ptx_update_vertices / ptx_skin_vertices were called
on since the previous call (`deformed`; `unsaved`: those of them whose records the library could not save, and
`relayout`: the layout was derived again since the previous call -- both give flag 2 where flag 3 would stand).
The class keeps the previous call's arrays: its geometry is what the library's snapshot holds.

The handle is tracking when the previous call was made with follow=True (set_follow(False) ends it, as
switching off does).  An edit -- the instance block differs from the kept one, or a mesh was deformed --
  * on a handle that is not tracking drops the state: the call is a first call (today's behaviour);
  * on a tracking handle called with follow=True gives every instance a flag: denoise_motion_ref.object_table's
    0 / 1 / 2, and 3 for an instance with the same mesh word whose mesh is in `deformed`.
The estimate u, the own sample d and the integration are TemporalUpsampler's.  Only the lookup of a hit pixel
changes, by the flag of its instance (key >> 16; past the table: 0):
  0  as TemporalUpsampler: the same pixel under the same camera words, else P through the previous VP;
  2  no lookup;
  1  Q = D P, Nq = D N (dn_temporal_px's element order, not renormalised); Q always through the previous VP,
     the four taps and bilinear weights of the reprojection; a tap counts inside the image with the same key,
     n' >= 0, dot(Nq, N') >= 0.9 and |dot(Nq, P' - Q)| <= this pixel's r;
  3  Q, Nq = GetSurface of this frame's texel on the previous call's scene and geometry arrays; then as 1.
With no flag set the call is TemporalUpsampler's, by the same code.

Exposed after a call: `flags` (per instance, None without a table), `taps` (per pixel, the taps that counted;
-1: no lookup ran), `pixel_flags`, and `cands`: per candidate k = 2 j + i, (a tap off the pixel itself inside
the image (H, W) bool, its row) -- what a band clips against its covered rows.
"""
from __future__ import annotations

import numpy as np

import denoise_motion_ref as M
import denoise_ref as D
import upsample_temporal_ref as UT

f32 = np.float32
STRIDE = M.STRIDE


class FollowUpsampler(UT.TemporalUpsampler):
    def __init__(self):
        super().__init__()
        self.tracking = False  # the previous call was made with follow=True
        self.insts = None      # the instance block that call kept
        self.prev = None       # (scene, geometry, accel) of that call
        self.flags = None
        self.taps = None
        self.pixel_flags = None
        self.cands = None
        self._obj = None
        self._verts = None     # of a call with a flag 3: (Q, Nq) per pixel

    def reset(self):
        """Everything that drops the state drops the marks with it; the switch and the tracking stay."""
        super().reset()

    def set_follow(self, on):
        """ptx_upsample_follow between two calls: switching off ends the tracking."""
        if not on:
            self.tracking = False

    def upsample(self, lo_rgb, G_lo, G_hi, hi_uniform, s, px, py, alpha_min=0.0, alpha_fill=-1.0, follow=True,
                 insts=None, scene=None, geometry=None, accel=None, gbuffer=None, deformed=(), unsaved=(),
                 relayout=False):
        insts = np.ascontiguousarray(insts, np.uint32).copy()
        self._obj, self._verts, self.flags = None, None, None
        changed = self.insts is not None and (len(self.insts) != len(insts) or not np.array_equal(self.insts, insts))
        changed = changed or len(tuple(deformed)) > 0
        if self.state is not None and changed:
            if not (self.tracking and follow) or self.insts is None or len(self.insts) != len(insts):
                self.reset()
            else:
                self._table(insts, G_hi, hi_uniform, gbuffer, set(deformed), set(unsaved), relayout)
        out = super().upsample(lo_rgb, G_lo, G_hi, hi_uniform, s, px, py, alpha_min, alpha_fill)
        self.taps = self.info["taps"]
        self.tracking = bool(follow)
        # (kept whatever the switch: what the scene was at this call is how the next one knows of an edit)
        self.insts = insts
        self.prev = tuple(np.array(a, np.uint32) for a in (scene, geometry, accel)) if scene is not None else None
        return out

    def _table(self, insts, G, uniform, gbuffer, deformed, unsaved, relayout):
        p, c = self.insts.reshape(-1, STRIDE), insts.reshape(-1, STRIDE)
        if not np.array_equal(self.insts, insts):
            flags, Ds = M.object_table(self.insts, insts)
        else:
            flags, Ds = np.zeros(len(c), np.int64), np.zeros((len(c), 16), np.float32)
        for i in range(len(c)):
            mesh = int(c[i, 32])
            if p[i, 32] == c[i, 32] and mesh in deformed:
                flags[i] = 3 if (self.prev is not None and mesh not in unsaved and not relayout) else 2
        if not flags.any():
            return  # (a table without a flag is no table)
        self._obj, self.flags = (flags, Ds), flags
        if (flags == 3).any():
            g = np.array(gbuffer, np.uint32)
            pf, _ = self._pixel_flags(G)
            g[..., 0] = np.where(pf == 3, g[..., 0], g[..., 0] & np.uint32(0x7FFFFFFF))  # (the others: no hit, skipped)
            Gp = D.guides_from_gbuffer(uniform, self.prev[0], self.prev[1], self.prev[2], g)
            self._verts = (Gp.P, Gp.N)

    def _pixel_flags(self, G):
        flags = self._obj[0]
        inst = np.where(G.hit, G.key >> np.uint32(16), 0).astype(np.int64)
        known = G.hit & (inst < len(flags))
        inst = np.minimum(inst, len(flags) - 1)
        return np.where(known, flags[inst], 0), inst

    def _lookup(self, G, camera):
        H, W = G.key.shape
        st = self.state
        if self._obj is None:
            self.pixel_flags = np.zeros((H, W), np.int64)
            pf, rigid, verts = self.pixel_flags, np.zeros((H, W), bool), np.zeros((H, W), bool)
            Q, Nq = G.P, G.N
        else:
            pf, inst = self._pixel_flags(G)
            self.pixel_flags = pf
            Dm = self._obj[1][inst]
            P, N = G.P, G.N
            rigid, verts = pf == 1, pf == 3
            Q = np.stack([((Dm[..., 0 + r] * P[..., 0] + Dm[..., 4 + r] * P[..., 1]) + Dm[..., 8 + r] * P[..., 2])
                          + Dm[..., 12 + r] for r in range(3)], -1).astype(np.float32)
            Nq = np.stack([(Dm[..., 0 + r] * N[..., 0] + Dm[..., 4 + r] * N[..., 1]) + Dm[..., 8 + r] * N[..., 2]
                           for r in range(3)], -1).astype(np.float32)
            Q = np.where(rigid[..., None], Q, P)
            Nq = np.where(rigid[..., None], Nq, N)
            if self._verts is not None:
                Q = np.where(verts[..., None], self._verts[0], Q)
                Nq = np.where(verts[..., None], self._verts[1], Nq)
        moved = rigid | verts
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        same_cam = np.array_equal(camera, st.camera)
        same = np.full((H, W), same_cam) & ~moved
        vp = st.vp
        cx = ((vp[0] * Q[..., 0] + vp[4] * Q[..., 1]) + vp[8] * Q[..., 2]) + vp[12]
        cy = ((vp[1] * Q[..., 0] + vp[5] * Q[..., 1]) + vp[9] * Q[..., 2]) + vp[13]
        cw = ((vp[3] * Q[..., 0] + vp[7] * Q[..., 1]) + vp[11] * Q[..., 2]) + vp[15]
        fx = ((cx / cw + f32(1)) * f32(0.5)) * f32(W) - f32(0.5)
        fy = ((cy / cw + f32(1)) * f32(0.5)) * f32(H) - f32(0.5)
        x0, y0 = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0, fy - y0
        # the same-pixel rule runs on every pixel, the projection on a hit pixel in front of the previous camera
        runs = (pf != 2) & (same | (G.hit & (cw > 0)))
        sw = np.zeros((H, W), np.float32)
        sC = np.zeros((H, W, 3), np.float32)
        nh = np.full((H, W), np.inf, np.float32)
        taps = np.where(runs, 0, -1)
        any_ = np.zeros((H, W), bool)
        self.cands = []
        k = 0
        for j in (0, 1):
            for i in (0, 1):
                qxf, qyf = x0 + f32(i), y0 + f32(j)
                inside = (qxf >= 0) & (qxf < f32(W)) & (qyf >= 0) & (qyf < f32(H))  # (NaN: outside)
                w = ((ax if i else f32(1) - ax) * (ay if j else f32(1) - ay)).astype(np.float32)
                self.cands.append((runs & ~same & inside, np.where(inside, qyf, 0).astype(np.int64)))
                inside = np.where(same, k == 0, inside)
                w = np.where(same, f32(1), w).astype(np.float32)
                qx = np.where(same, xs, np.where(inside, qxf, 0).astype(np.int64))
                qy = np.where(same, ys, np.where(inside, qyf, 0).astype(np.int64))
                nq = st.n[qy, qx]
                ok = runs & inside & (st.G.key[qy, qx] == G.key) & (nq >= 0)
                geo = (D.dot3(Nq, st.G.N[qy, qx]) >= f32(0.9)) & (np.abs(D.dot3(Nq, st.G.P[qy, qx] - Q)) <= G.r)
                ok &= ~G.hit | geo
                sw = np.where(ok, sw + w, sw)
                sC = np.where(ok[..., None], sC + st.H[qy, qx] * w[..., None], sC)
                nh = np.where(ok, np.minimum(nh, nq), nh)
                any_ |= ok
                taps = taps + ok
                k += 1
        return any_ & (sw > 0), sC / sw[..., None], nh, taps, same_cam
