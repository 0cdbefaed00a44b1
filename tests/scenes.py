"""Test scenes whose content crosses the kernels' decomposition, and a float64 classifier of their constraints.

datagen.synth_pair renders one smooth surface at 1.0-2.3 m with 8 x 8 holes on an 8-aligned grid: no lane pair (2l, 2l + 1) is ever
half valid, no validity change falls inside an 8-row strip, nothing is occluded at the true pose.  edge_scene() renders a slanted
background plane (3 m to beyond the 12 m sensor range) with foreground boxes at 0.3-0.8 m, from two poses, by analytic ray casting
(nearest hit wins), and punches holes placed on purpose: single pixels of every parity, bands with every other column invalid,
rectangles of size 1-13 at random offsets, rows 8k + 7 / 8k + 8, columns 127 / 128 and the image border.  It returns the dict of
datagen.synth_pair, so the oracle's pyramids, the GPU ingest and the reference's match() take it unchanged.

classify() restates the projection, bounds (Q4), NaN-tap (Q9) and occlusion (Q5) tests of one linearisation in float64 from the
oracle's float32 planes, with each pixel's margin to the decision it depends on.  Plain numpy, deterministic from the seed.
"""
import numpy as np

FR1_K = np.array([517.3, 516.5, 318.6, 255.3], dtype=np.float32)
SENSOR_RANGE_RAW = 60000          # 12 m at 5000 counts per metre: farther returns are raw 0, as a sensor drops them

# decision classes of a selected reference pixel (classify)
VALID, NO_DEPTH, OUT_OF_BOUNDS, NAN_TAP, OCCLUDED = 0, 1, 2, 3, 4


def se3_exp(xi):
    """exp of the twist (v, omega) as a 4 x 4 (Rodrigues, the formula of datagen/synth.cpp)"""
    u, w = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < 1e-6:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    O = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + a * O + b * (O @ O)
    M[:3, 3] = (np.eye(3) + b * O + c * (O @ O)) @ u
    return M


class _Scene:
    """The analytic scene in the reference camera's frame: the plane a x + b y + c z = 1 (1/z = c + a x/z + b y/z) and axis-aligned boxes."""

    def __init__(self, rng):
        self.plane = np.array([rng.uniform(-0.03, 0.03), rng.uniform(0.26, 0.28), rng.uniform(0.205, 0.215)])   # (a, b, c)
        self.boxes = []
        for k in range(3):
            z0 = (0.3, 0.5, 0.7)[k] + rng.uniform(0.0, 0.1)                  # front face at 0.3-0.8 m
            ang = rng.uniform(0.06, 0.13)                                      # half size, as an angle seen from the camera
            cx, cy = rng.uniform(-0.45, 0.45), rng.uniform(-0.3, 0.3)
            half = np.array([ang * z0 * rng.uniform(0.8, 1.4), ang * z0 * rng.uniform(0.8, 1.4), rng.uniform(0.03, 0.15)])
            centre = np.array([cx * z0, cy * z0, z0 + half[2]])
            self.boxes.append((centre - half, centre + half))
        # texture: per surface, sinusoids of the 3-D point; wavelengths in proportion to the surface's distance (no aliasing)
        self.tex = []
        for scale in (0.4, 0.06, 0.06, 0.06):
            dirs = rng.uniform(-1, 1, (6, 3))
            dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
            k = 2 * np.pi / (scale * np.array([0.4, 0.6, 0.9, 1.4, 2.2, 3.5]))
            self.tex.append((dirs, k, rng.uniform(0, 2 * np.pi, 6), 0.5 + 0.1 * np.arange(6)))
        self.base = [0.0] + list(rng.uniform(-0.4, 0.4, 3))                     # per-surface brightness: intensity edges at depth edges

    def cast(self, o, d):
        """nearest hit of rays o + s d, d = R (x, y, 1) of the ray's own camera (s: the depth in that camera): (s, surface id, point)"""
        n = self.plane
        den = d @ n
        s = (1.0 - o @ n) / den                                                 # n . p = 1
        s = np.where((den > 0) & (s > 0), s, np.inf)
        sid = np.zeros(s.shape, np.int32)
        with np.errstate(divide="ignore", invalid="ignore"):
            for i, (lo, hi) in enumerate(self.boxes):
                t0 = (lo - o) / d
                t1 = (hi - o) / d
                tn = np.minimum(t0, t1).max(-1)
                tf = np.maximum(t0, t1).min(-1)
                hit = (tn <= tf) & (tn > 0) & (tn < s)
                s = np.where(hit, tn, s)
                sid = np.where(hit, i + 1, sid)
        return s, sid, o + s[..., None] * d

    def grey(self, p, sid, noise):
        t = np.zeros(sid.shape)
        for i, (dirs, k, ph, amp) in enumerate(self.tex):
            on = sid == i
            v = (amp * np.sin(k * (p[on] @ dirs.T) + ph)).sum(-1) / (0.75 * amp.sum()) + self.base[i]
            t[on] = v
        g = 127.5 + 80.0 * np.clip(t, -1.5, 1.5) + noise
        return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def _quantise_depth(z):
    q = np.rint(np.where(np.isfinite(z), z, 0.0) * 5000.0)
    return np.where((q >= 1) & (q <= SENSOR_RANGE_RAW), q, 0).astype(np.uint16)


def punch_holes(depth, rng):
    """Holes that cross the kernels' decomposition (in place): see the module docstring."""
    h, w = depth.shape
    # single invalid pixels, every parity of x and y
    for px in range(2):
        for py in range(2):
            n = max(8, w * h // 2000)
            xs = 2 * rng.integers(0, w // 2, n) + px
            ys = 2 * rng.integers(0, h // 2, n) + py
            depth[np.minimum(ys, h - 1), np.minimum(xs, w - 1)] = 0
    # bands where every other column is invalid: every lane pair of the band is half valid (odd columns in one, even in the other)
    for parity in range(2):
        bw, bh = max(8, w // 6), max(4, h // 12)
        x0, y0 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        depth[y0:y0 + bh, x0 + parity:x0 + bw:2] = 0
    # rectangles of size 1-13 at random offsets
    for _ in range(max(4, w * h // 1500)):
        rw, rh = rng.integers(1, 14, 2)
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        depth[y0:y0 + rh, x0:x0 + rw] = 0
    # the strip rows y = 8k + 7 and 8k + 8, the strip columns 128k - 1 and 128k, the border rows and columns: short segments
    for _ in range(max(4, w // 16)):
        y = 8 * int(rng.integers(0, max(1, (h - 9) // 8))) + 7 + int(rng.integers(0, 2))
        x0, n = int(rng.integers(0, w)), int(rng.integers(1, 24))
        depth[min(y, h - 1), x0:x0 + n] = 0
    for x in range(127, w, 128):
        for xx in (x, x + 1):
            if xx < w:
                for _ in range(max(1, h // 40)):
                    y0, n = int(rng.integers(0, h)), int(rng.integers(1, 12))
                    depth[y0:y0 + n, xx] = 0
    for _ in range(max(2, w // 64)):
        for edge in ("top", "bottom", "left", "right"):
            if edge in ("top", "bottom"):
                x0, n = int(rng.integers(0, w)), int(rng.integers(1, 12))
                depth[0 if edge == "top" else h - 1, x0:x0 + n] = 0
            else:
                y0, n = int(rng.integers(0, h)), int(rng.integers(1, 12))
                depth[y0:y0 + n, 0 if edge == "left" else w - 1] = 0


def edge_scene(seed, w=640, h=480, K=None):
    """-> dict(grey_ref u8, depth_ref u16, grey_cur u8, depth_cur u16, K, xi_true) like datagen.synth_pair: xi_true is the twist of
    the transform match() should return (current -> reference)."""
    rng = np.random.default_rng([seed, w, h])
    K = np.ascontiguousarray(FR1_K * (w / 640.0) if K is None else K, dtype=np.float32)
    fx, fy, ox, oy = (float(k) for k in K)
    scene = _Scene(rng)
    # motion like synth's (|v| <= 3 cm, |omega| <= 0.03 rad), with a translation of at least 1.5 cm across the line of sight: the
    # foreground boxes then occlude and disocclude several pixels of background along their edges at the true pose
    xi = np.zeros(6)
    for part, lo in ((0, 0.5), (1, 0.3)):
        dvec = rng.uniform(-1, 1, 3)
        if part == 0:
            dvec[2] *= 0.5
        xi[3 * part:3 * part + 3] = dvec / np.linalg.norm(dvec) * 0.03 * rng.uniform(lo, 1.0)
    M = se3_exp(xi)                                         # current -> reference
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rays = np.stack([(xx - ox) / fx, (yy - oy) / fy, np.ones_like(xx)], -1)
    out = dict(K=K, xi_true=xi)
    for view, (o, d) in (("ref", (np.zeros(3), rays)), ("cur", (M[:3, 3], rays @ M[:3, :3].T))):
        s, sid, p = scene.cast(o, d)
        depth = _quantise_depth(s)
        out["grey_" + view] = scene.grey(p, sid, rng.uniform(-1.5, 1.5, (h, w)))
        punch_holes(depth, rng)
        out["depth_" + view] = depth
    return out


def classify(Zr, selected, cur, K, T, eps_uv=None, slopes=False):
    """The fate of every reference pixel of one linearisation, in float64.
    Zr: the reference level's depth plane (float32, NaN = no depth); selected: its selection mask; cur: the current level's six planes
    (intensity, depth, intensity_dx, intensity_dy, depth_dx, depth_dy; float32); K = (fx, fy, ox, oy); T: the 4 x 4 (or 3 x 4) warp
    reference -> current that the linearisation takes (in float64: pass the float32 matrix the kernels see).
    Returns (cls [h, w] of VALID / NO_DEPTH / OUT_OF_BOUNDS / NAN_TAP / OCCLUDED, -1 where not selected; ambiguous [h, w]: the
    float32 arithmetic of a kernel may decide otherwise -- the tap coordinate lies within eps_uv of a bound or of an integer where
    the taps' NaN pattern changes, or the depth residual lies within its rounding of the occlusion threshold).  eps_uv defaults to
    2.5e-7 (w + h), about four float32 ulp of the largest tap coordinate (the contracted schedule's coordinates are within three).
    slopes: also return |d/du| + |d/dv| of the bilinear blend of intensity and of depth at each pixel's tap coordinate (how far a
    residual moves per pixel of coordinate error: large across a depth edge)."""
    h, w = Zr.shape
    if eps_uv is None:
        eps_uv = 2.5e-7 * (w + h)
    fx, fy, ox, oy = (float(k) for k in K)
    T = np.asarray(T, np.float64)
    I, Zc = (np.asarray(a, np.float64) for a in cur[:2])
    Z = np.asarray(Zr, np.float64)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    X, Y = (xx - ox) / fx * Z, (yy - oy) / fy * Z
    qx = T[0, 0] * X + T[0, 1] * Y + T[0, 2] * Z + T[0, 3]
    qy = T[1, 0] * X + T[1, 1] * Y + T[1, 2] * Z + T[1, 3]
    qz = T[2, 0] * X + T[2, 1] * Y + T[2, 2] * Z + T[2, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        u, v = fx * qx / qz + ox, fy * qy / qz + oy
    cls = np.full((h, w), -1, np.int8)
    amb = np.zeros((h, w), bool)
    sel = selected.astype(bool)
    has_z = sel & ~np.isnan(Z)
    cls[sel & ~has_z] = NO_DEPTH
    margin = np.minimum(np.minimum(u, w - 2 - u), np.minimum(v, h - 2 - v))
    inb = has_z & (margin >= 0)
    cls[has_z & ~inb] = OUT_OF_BOUNDS
    amb |= has_z & (np.abs(np.nan_to_num(margin, nan=1e9)) < eps_uv)
    bad = np.zeros((h, w), bool)
    for p in cur:
        bad |= np.isnan(p)

    def nan_taps(uu, vv):
        u0 = np.clip(np.floor(uu), 0, w - 2).astype(np.int64)
        v0 = np.clip(np.floor(vv), 0, h - 2).astype(np.int64)
        return bad[v0, u0] | bad[v0, u0 + 1] | bad[v0 + 1, u0] | bad[v0 + 1, u0 + 1]
    ui, vi = np.where(inb, u, 0.0), np.where(inb, v, 0.0)
    nt = nan_taps(ui, vi)
    for du, dv in ((-eps_uv, -eps_uv), (-eps_uv, eps_uv), (eps_uv, -eps_uv), (eps_uv, eps_uv)):
        amb |= inb & (nan_taps(ui + du, vi + dv) != nt)
    cls[inb & nt] = NAN_TAP
    ok = inb & ~nt
    u0 = np.clip(np.floor(ui), 0, w - 2).astype(np.int64)
    v0 = np.clip(np.floor(vi), 0, h - 2).astype(np.int64)
    a1, b1 = ui - u0, vi - v0
    a0, b0 = 1 - a1, 1 - b1
    z00, z10, z01, z11 = (np.nan_to_num(Zc[v0 + j, u0 + i]) for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)))
    cZ = b0 * (a0 * z00 + a1 * z10) + b1 * (a0 * z01 + a1 * z11)
    r1 = cZ - qz
    sigma = 0.0012 + 0.0019 * (Z - 0.4) ** 2
    occ = ok & ~(r1 > -20.0 * sigma)
    cls[occ] = OCCLUDED
    cls[ok & ~occ] = VALID
    # how far the float32 residual can stray: a few ulp of the depths involved, plus the blend's slope times the coordinate's error
    slope = np.abs(b0 * (z10 - z00) + b1 * (z11 - z01)) + np.abs(a0 * (z01 - z00) + a1 * (z11 - z10))
    err = 1e-6 * (np.abs(qz) + np.abs(cZ) + 1.0) + eps_uv * slope
    amb |= ok & (np.abs(np.nan_to_num(r1 + 20.0 * sigma)) < err)
    if slopes:
        i00, i10, i01, i11 = (np.nan_to_num(I[v0 + j, u0 + i]) for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)))
        slope_I = np.abs(b0 * (i10 - i00) + b1 * (i11 - i01)) + np.abs(a0 * (i01 - i00) + a1 * (i11 - i10))
        return cls, amb, slope_I, slope
    return cls, amb
