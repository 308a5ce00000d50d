"""NumPy FP64 restatement of the motion build of temporal accumulation (temporal_reproject<true> of raytracer_project_amd/csrc/zr_temporal.hip),
operation for operation, on top of tests/temporal_model.py: a frame one refit after the history's.  Per hit pixel the world-list entry under it (the entry plane,
Scene.render_gbuffer_entries) names a word of the refit's motion table (Scene.motion()): STATIC -> the static steps exactly; CUT -> no history; a slot ->
Xr = A X_p and nr = Nm n_p / |Nm n_p| take X_p's and n_p's places in the projection into the previous view and in the plane and normal tests, while depth_p
stays that of X_p in the current view.  Also the host's record arithmetic (zr_motion.h) for hand-made placements, for the tests that build tables by hand."""
import numpy as np

import temporal_model as tm
from temporal_model import MISS, SNAP, clean, clean_variance, dot3

STATIC, CUT = 0xFFFFFFFF, 0xFFFFFFFE     # ZR_MOTION_STATIC, ZR_MOTION_CUT
RECORD = 21


def record(A_lin, A_t, Nm=None):
    """a record from a 3x3 linear part, a translation and (default: the inverse transpose, by NumPy — hand-made tables use exact matrices) the normal map"""
    A_lin = np.asarray(A_lin, dtype=np.float64); A_t = np.asarray(A_t, dtype=np.float64)
    Nm = np.linalg.inv(A_lin).T if Nm is None else np.asarray(Nm, dtype=np.float64)
    r = np.zeros(RECORD)
    for k in range(3):
        r[4 * k:4 * k + 3] = A_lin[k]; r[4 * k + 3] = A_t[k]
    r[12:] = Nm.reshape(9)
    return r + 0.0


def moved_points(records, word, X, n):
    """the motion build's Xr, nr and `followed` for pixels with table words `word` (H, W): a slot applies its record, STATIC keeps X and n, CUT is not followed"""
    X = np.asarray(X, dtype=np.float64); n = np.asarray(n, dtype=np.float64)
    word = np.asarray(word, dtype=np.int64)
    records = np.asarray(records, dtype=np.float64).reshape(-1, RECORD)
    has = word < len(records)                       # (STATIC and CUT are above every slot)
    a = records[np.where(has, word, 0)] if len(records) else np.zeros(word.shape + (RECORD,))
    Xr, g = np.empty_like(X), np.empty_like(n)
    with np.errstate(all="ignore"):
        for k in range(3):
            Xr[..., k] = ((a[..., 4 * k] * X[..., 0] + a[..., 4 * k + 1] * X[..., 1]) + a[..., 4 * k + 2] * X[..., 2]) + a[..., 4 * k + 3]
            g[..., k] = (a[..., 12 + 3 * k] * n[..., 0] + a[..., 13 + 3 * k] * n[..., 1]) + a[..., 14 + 3 * k] * n[..., 2]
        l = np.sqrt(dot3(g, g))
        nr = g / l[..., None]
    followed = np.where(has, l > 0, word != CUT)
    keep = ~has | ~(l > 0)
    return np.where(keep[..., None], X, Xr), np.where(keep[..., None], n, nr), followed


class History(tm.History):
    """tm.History with the motion build: accumulate_moved() for a frame one refit after the one held; accumulate() is the static build, unchanged"""

    def accumulate_moved(self, cur_view, g, entry, slot, records, color, variance, alpha=0.4, max_history=32, plane_tolerance=0.03, normal_cos=0.9):
        """entry: (H, W) world-list entry under each pixel (MISS on a miss); slot, records: Scene.motion() of the refit between the held frame and this one"""
        H, W = self.H, self.W
        c, V = clean(color).reshape(H, W, 3), clean_variance(variance).reshape(H, W, 3)
        X, n, m = g["position"], g["normal"], g["mat"]
        hit = m != MISS
        slot = np.asarray(slot, dtype=np.int64)
        entry = np.asarray(entry, dtype=np.int64)
        named = hit & (entry != MISS) & (entry < len(slot))
        word = np.where(named, slot[np.where(named, entry, 0)] if len(slot) else STATIC, STATIC)
        sw = np.zeros((H, W)); sh = np.zeros((H, W, 3)); sv = np.zeros((H, W, 3))
        min_n = np.full((H, W), 0x7FFFFFFF, dtype=np.int64)
        if self.frames > 0:
            pv = self.view
            Xr, nr, followed = moved_points(records, word, X, n)
            with np.errstate(all="ignore"):
                d = np.where(hit[..., None], Xr - pv["center"], Xr)
                zc = -dot3(d, pv["w"])
                s = pv["f"] / zc
                q = (pv["center"] + d * s[..., None]) - pv["pixel00"]
                fx = dot3(q, pv["a"]); fy = dot3(q, pv["b"])
                depth = -dot3(X - cur_view["center"], cur_view["w"])
                rx, ry = np.rint(fx), np.rint(fy)
                fx = np.where(np.abs(fx - rx) <= SNAP, rx, fx)
                fy = np.where(np.abs(fy - ry) <= SNAP, ry, fy)
                ok = followed & (zc > 0) & (fx >= -1.0) & (fx <= float(W)) & (fy >= -1.0) & (fy <= float(H))
                fx = np.where(ok, fx, 0.0); fy = np.where(ok, fy, 0.0)
                flx, fly = np.floor(fx), np.floor(fy)
                wx, wy = fx - flx, fy - fly
                x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
                bound = plane_tolerance * depth
                for dy in (0, 1):
                    for dx in (0, 1):
                        w = (wx if dx else 1.0 - wx) * (wy if dy else 1.0 - wy)
                        qx, qy = x0 + dx, y0 + dy
                        inside = ok & (w > 0) & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                        cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                        nq = self.len[cy, cx]
                        counts = inside & (nq > 0) & (self.g["mat"][cy, cx] == m)
                        e = self.g["position"][cy, cx] - Xr
                        plane = np.abs(dot3(e, nr)) <= bound
                        facing = dot3(nr, self.g["normal"][cy, cx]) >= normal_cos
                        counts &= ~hit | (plane & facing)
                        sw = np.where(counts, sw + w, sw)
                        sh = np.where(counts[..., None], sh + w[..., None] * self.col[cy, cx], sh)
                        sv = np.where(counts[..., None], sv + w[..., None] * self.var[cy, cx], sv)
                        min_n = np.where(counts, np.minimum(min_n, nq), min_n)
        have = sw > 0
        N = np.where(have, np.minimum(min_n + 1, max_history), 1).astype(np.int32)
        with np.errstate(all="ignore"):
            beta = np.maximum(1.0 / N.astype(np.float64), alpha)
            om = 1.0 - beta
            h = sh / sw[..., None]; vh = sv / sw[..., None]
            out = np.where(have[..., None], h + beta[..., None] * (c - h), c)
            vout = np.where(have[..., None], (om * om)[..., None] * vh + (beta * beta)[..., None] * V, V)
        self.view, self.g = cur_view, {k: np.array(a) for k, a in g.items()}
        self.col, self.var, self.len = out, vout, N
        self.frames += 1
        return out, vout, N
