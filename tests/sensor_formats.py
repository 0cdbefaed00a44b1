"""The raw sensor formats of the ingest (DVO_HIP_PIXEL_BAYER_*, DVO_HIP_PIXEL_YUYV8 / _UYVY8), stated a second time in numpy and
independently of dvo_slam_amd/csrc/sensor_formats.h: whole-image array arithmetic over letter masks and floor divisions where the header
works per pixel with phase bits and shifts.  demosaic / yuv422_to_bgr give the BGR8 image that DEFINES a sensor plane; mosaic / to_yuv422
make sensor planes from BGR images (inputs only: nothing is asserted about them)."""
import numpy as np

BAYER = ("bayer_rggb8", "bayer_bggr8", "bayer_gbrg8", "bayer_grbg8")
YUV = ("yuyv8", "uyvy8")
FORMATS = BAYER + YUV


def channels(fmt):
    return 1 if fmt in BAYER else 2


def _letters(pattern, h, w):
    """[h, w] array of 'r' / 'g' / 'b': the colour each site of the mosaic samples.  pattern: "rggb" or "bayer_rggb8", the 2 x 2 block at
    the image's top-left corner, row-major"""
    p = pattern.replace("bayer_", "").replace("8", "")
    assert sorted(p) == ["b", "g", "g", "r"], pattern
    block = np.array([[p[0], p[1]], [p[2], p[3]]])
    return np.tile(block, ((h + 1) // 2, (w + 1) // 2))[:h, :w]


def demosaic(raw, pattern):
    """bilinear demosaic of the [h, w] uint8 mosaic -> [h, w, 3] uint8 BGR, neighbours outside the image by reflection about the edge pixel"""
    raw = np.asarray(raw)
    if raw.ndim == 3:
        raw = raw[:, :, 0]
    h, w = raw.shape
    assert h >= 2 and w >= 2 and raw.dtype == np.uint8
    p = np.pad(raw.astype(np.int64), 1, mode="reflect")          # (index -1 -> 1, w -> w - 2)
    centre = p[1:-1, 1:-1]
    north, south, west, east = p[:-2, 1:-1], p[2:, 1:-1], p[1:-1, :-2], p[1:-1, 2:]
    cross = (north + south + west + east + 2) // 4
    diag = (p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:] + 2) // 4
    hor, ver = (west + east + 1) // 2, (north + south + 1) // 2
    site = _letters(pattern, h, w)
    # the colour the non-green sites of each row sample
    row_colour = np.where((site == "r").any(axis=1), "r", "b")[:, None].repeat(w, axis=1)
    out = {}
    out["g"] = np.where(site == "g", centre, cross)
    for c, other in (("r", "b"), ("b", "r")):
        out[c] = np.select([site == c, site == other, row_colour == c], [centre, diag, hor], ver)
    return np.stack([out["b"], out["g"], out["r"]], axis=-1).astype(np.uint8)


def yuv422_to_bgr(raw, order):
    """[h, w, 2] uint8 YUV 4:2:2 (order "yuyv8": Y0 U Y1 V; "uyvy8": U Y0 V Y1) -> [h, w, 3] uint8 BGR: BT.601 limited range in 20-bit
    fixed point, both pixels of a pair with the pair's chroma"""
    raw = np.asarray(raw)
    h, w, two = raw.shape
    assert two == 2 and w % 2 == 0 and raw.dtype == np.uint8
    quad = raw.reshape(h, w // 2, 4).astype(np.int64)
    iy, iu, iv = ((0, 2), 1, 3) if order.startswith("yuyv") else ((1, 3), 0, 2)
    assert order.startswith("yuyv") or order.startswith("uyvy"), order
    luma = np.stack([quad[:, :, iy[0]], quad[:, :, iy[1]]], axis=-1).reshape(h, w)
    u = np.repeat(quad[:, :, iu], 2, axis=1) - 128
    v = np.repeat(quad[:, :, iv], 2, axis=1) - 128
    y = np.maximum(luma - 16, 0) * 1220542 + 2 ** 19
    one = 2 ** 20
    r = np.floor_divide(y + 1673527 * v, one)
    g = np.floor_divide(y - 409993 * u - 852492 * v, one)
    b = np.floor_divide(y + 2116026 * u, one)
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def to_bgr(raw, fmt):
    return demosaic(raw, fmt) if fmt in BAYER else yuv422_to_bgr(raw, fmt)


def packed(bgr):
    """0x00RRGGBB per pixel (cloud_colour.h)"""
    c = bgr.astype(np.uint32)
    return c[..., 2] << 16 | c[..., 1] << 8 | c[..., 0]


def mosaic(bgr, pattern):
    """the [h, w] uint8 mosaic that samples the BGR image at each site's colour"""
    h, w, _ = bgr.shape
    site = _letters(pattern, h, w)
    return np.select([site == "b", site == "g"], [bgr[:, :, 0], bgr[:, :, 1]], bgr[:, :, 2]).astype(np.uint8)


def to_yuv422(bgr, order):
    """a [h, w, 2] uint8 YUV 4:2:2 plane of the BGR image (w even): BT.601 limited range, a pair's chroma the mean of its two pixels'"""
    h, w, _ = bgr.shape
    assert w % 2 == 0
    b, g, r = (bgr[:, :, k].astype(np.float64) for k in range(3))
    y = 16.0 + 0.257 * r + 0.504 * g + 0.098 * b
    u = 128.0 - 0.148 * r - 0.291 * g + 0.439 * b
    v = 128.0 + 0.439 * r - 0.368 * g - 0.071 * b
    u2 = 0.5 * (u[:, 0::2] + u[:, 1::2])
    v2 = 0.5 * (v[:, 0::2] + v[:, 1::2])
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    out = np.empty((h, w // 2, 4), np.uint8)
    if order.startswith("yuyv"):
        out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3] = q(y[:, 0::2]), q(u2), q(y[:, 1::2]), q(v2)
    else:
        assert order.startswith("uyvy"), order
        out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3] = q(u2), q(y[:, 0::2]), q(v2), q(y[:, 1::2])
    return out.reshape(h, w, 2)


def to_sensor(bgr, fmt):
    return mosaic(bgr, fmt) if fmt in BAYER else to_yuv422(bgr, fmt)


EVERY_YUV_SHAPE = (4096, 8192)     # h, w: 2^24 pixel pairs


def every_yuv(order):
    """the [4096, 8192, 2] plane whose pixel pair i (raster order) holds Y0 = i & 255, U = i >> 8 & 255, V = i >> 16 and Y1 = 255 - Y0:
    every (Y, U, V) at both positions of a pair"""
    h, w = EVERY_YUV_SHAPE
    i = np.arange(h * (w // 2), dtype=np.uint32)
    y0, u, v = (i & 255).astype(np.uint8), (i >> 8 & 255).astype(np.uint8), (i >> 16).astype(np.uint8)
    y1 = (255 - y0).astype(np.uint8)
    quad = np.stack([y0, u, y1, v] if order.startswith("yuyv") else [u, y0, v, y1], axis=-1)
    return quad.reshape(h, w, 2)


def every_yuv_bgr():
    """the BGR image of every_yuv(order), the same for both orders, computed in slabs of rows"""
    h, w = EVERY_YUV_SHAPE
    plane = every_yuv("yuyv8")
    return np.concatenate([yuv422_to_bgr(plane[y:y + 256], "yuyv8") for y in range(0, h, 256)], axis=0)


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def one_hots(h, w):
    """[h, w] images with a single 255: at each of the four mosaic phases (near the centre) and at each corner"""
    cy, cx = (h // 2) & ~1, (w // 2) & ~1
    spots = {(cy + dy, cx + dx) for dy in (0, 1) for dx in (0, 1) if cy + dy < h and cx + dx < w}
    spots |= {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}
    out = []
    for y, x in sorted(spots):
        a = np.zeros((h, w), np.uint8)
        a[y, x] = 255
        out.append(a)
    return out
