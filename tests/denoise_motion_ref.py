"""numpy restatement of object motion in the denoiser's temporal lookup (include/ptx.h ptx_denoise,
"Object motion"; DESIGN.md §Scene edits), built on tests/denoise_temporal_ref.py.

Test infrastructure only: the checker of dn_temporal<true> in pathtracerdemo_amd/csrc/ptx_denoise.hip.
Every temporal call keeps the instance block of the scene array (33 words per instance: M, M^-1, mesh)
beside its camera.  The next call compares block and snapshot per instance: with none different it is
TemporalDenoiser's call bit for bit; otherwise every instance gets a flag and D = M_prev * Minv_cur, and
a hit pixel of instance i = key >> 16 looks its history up by flag:
  0  unchanged: the same pixel when the camera words are the previous call's, else P reprojected;
  2  no lookup: the pixel starts from the frame's colour with n = 1;
  1  moved rigidly: Q = D P and Nq = D N (linear part, not renormalised) are where the point and its
     normal were; Q is always reprojected through the previous call's VP, the taps and weights are the
     reprojection's, and a tap is tested against Q and Nq with this pixel's r.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import denoise_temporal_ref as T

f32 = np.float32
STRIDE = 33
RIGID_TOL = 1e-3


def object_table(prev, cur):
    """(flags (n,) int, D (n, 16) f32 column-major) from two instance blocks."""
    prev = np.ascontiguousarray(prev, np.uint32).reshape(-1, STRIDE)
    cur = np.ascontiguousarray(cur, np.uint32).reshape(-1, STRIDE)
    assert prev.shape == cur.shape
    n = len(cur)
    flags, Ds = np.zeros(n, np.int64), np.zeros((n, 16), np.float32)
    for i in range(n):
        if np.array_equal(prev[i], cur[i]):
            continue
        m = prev[i, :16].view(np.float32)
        v = cur[i, 16:32].view(np.float32)
        d = np.zeros(16, np.float32)
        with np.errstate(all="ignore"):
            for col in range(4):
                for row in range(4):
                    s = 0.0
                    for k in range(4):
                        s += float(m[row + 4 * k]) * float(v[k + 4 * col])
                    d[row + 4 * col] = np.float32(s)
            rigid = bool(prev[i, 32] == cur[i, 32])
            for a in (m, v):
                rigid &= bool(a[3] == 0 and a[7] == 0 and a[11] == 0 and a[15] == 1)
            rigid &= bool(np.isfinite(m).all() and np.isfinite(v).all() and np.isfinite(d).all())
            worst = 0.0
            if rigid:
                for a in range(3):
                    for b in range(3):
                        s = 0.0
                        for k in range(3):
                            s += float(d[k + 4 * a]) * float(d[k + 4 * b])
                        worst = max(worst, abs(s - (1.0 if a == b else 0.0)))
        flags[i] = 1 if rigid and worst <= RIGID_TOL else 2
        Ds[i] = d
    return flags, Ds


class MotionDenoiser(T.TemporalDenoiser):
    """TemporalDenoiser whose calls also take the scene's instance block (`insts`)."""

    def __init__(self):
        super().__init__()
        self.insts = None  # the previous temporal call's instance block
        self.flags = None  # of the last call, if it found an instance changed: the per-instance flags
        self._obj = None

    def reset(self):
        super().reset()
        self.insts = None

    def denoise(self, frame_color, accum, G, uniform, insts=None, temporal=True, **kw):
        if not temporal:
            return super().denoise(frame_color, accum, G, uniform, temporal=False, **kw)
        insts = np.ascontiguousarray(insts, np.uint32).copy()
        self._obj, self.flags = None, None
        if self.state is not None and self.insts is not None and len(self.insts) == len(insts) \
                and not np.array_equal(self.insts, insts):
            self._obj = object_table(self.insts, insts)
            self.flags = self._obj[0]
        out = super().denoise(frame_color, accum, G, uniform, **kw)
        self.insts = insts
        return out

    def pixel_flags(self, G):
        """(H, W) flag of every pixel's instance (0 without a hit)."""
        flags = self._obj[0]
        inst = np.where(G.hit, G.key >> np.uint32(16), 0).astype(np.int64)
        known = G.hit & (inst < len(flags))
        return np.where(known, flags[np.minimum(inst, len(flags) - 1)], 0), np.minimum(inst, len(flags) - 1)

    def _lookup(self, G, camera):
        if self._obj is None:
            return super()._lookup(G, camera)
        H, W = G.key.shape
        s = self.state
        pf, inst = self.pixel_flags(G)
        Dm = self._obj[1][inst]  # (H, W, 16)
        P, N = G.P, G.N
        follow = pf == 1
        Q = np.stack([((Dm[..., 0 + r] * P[..., 0] + Dm[..., 4 + r] * P[..., 1]) + Dm[..., 8 + r] * P[..., 2])
                      + Dm[..., 12 + r] for r in range(3)], -1).astype(np.float32)
        Nq = np.stack([(Dm[..., 0 + r] * N[..., 0] + Dm[..., 4 + r] * N[..., 1]) + Dm[..., 8 + r] * N[..., 2]
                       for r in range(3)], -1).astype(np.float32)
        Q = np.where(follow[..., None], Q, P)
        Nq = np.where(follow[..., None], Nq, N)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        same_cam = np.array_equal(camera, s.camera)
        self.same_pixel = same_cam
        same = np.full((H, W), same_cam) & ~follow
        # the reprojection of Q (flag 0: Q = P)
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
                # the same-pixel rule: one tap, the pixel itself with weight 1
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
