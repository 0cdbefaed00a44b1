"""The camera models of the suite, in one place: CAMERAS(w, h) -> {name: float32 K = [fx, fy, ox, oy]} of a w x h image.

Every generator of the suite defaults to the fr1 intrinsics scaled by the image width -- a forgiving camera: fx = fy to 0.15 %, the
principal point within a pixel of the image centre in x, a mid-range field of view.  The others each take one of those comforts away:
  fr1      FR1_K w / 640                             the control
  aniso    0.6 w, 1.3 w, 0.37 w, 0.61 h              fx from fy, ox from oy, both far from the centre
  wide     0.35 w, 0.35 w, w/2 - 0.5, h/2 - 0.5      110 degrees across: large tx / ty table entries, strong parallax spread per tile
  tele     2.5 w, 2.5 w, 0.45 w + 0.25, 0.55 h - 0.25  pixel motion per radian x 3; a principal point whose halvings are no exact quarter pixels
  outside  0.9 w, 0.8 w, -0.1 w, 1.05 h              the principal point outside the image (a cropped sensor): ox < 0, oy > h
datagen.synth_pair renders a metric scene (depth 1.0-2.3 m whatever the camera), so each of them keeps about three quarters of the
selected pixels as constraints.  tests/test_camera_models.py (CPU) and tests/test_gpu_camera_models.py (GPU) run them."""
import numpy as np

FR1_K = np.array([517.3, 516.5, 318.6, 255.3], dtype=np.float32)
NAMES = ("fr1", "aniso", "wide", "tele", "outside")


def CAMERAS(w, h):
    k = lambda *v: np.array(v, dtype=np.float32)   # noqa: E731
    return {
        "fr1": np.ascontiguousarray(FR1_K * (w / 640.0), dtype=np.float32),      # (the generators' default, the same bits)
        "aniso": k(0.6 * w, 1.3 * w, 0.37 * w, 0.61 * h),
        "wide": k(0.35 * w, 0.35 * w, w / 2.0 - 0.5, h / 2.0 - 0.5),
        "tele": k(2.5 * w, 2.5 * w, 0.45 * w + 0.25, 0.55 * h - 0.25),
        "outside": k(0.9 * w, 0.8 * w, -0.1 * w, 1.05 * h),
    }


def level_K(K, level):
    """K of a pyramid level: halved `level` times in float32 (IntrinsicMatrix::scale(0.5f), Q17)"""
    K = np.asarray(K, np.float32).copy()
    for _ in range(level):
        K = K * np.float32(0.5)
    return K
