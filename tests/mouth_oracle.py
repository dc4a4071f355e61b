"""Mouth ROIs from whole camera frames in float64 numpy (rtfs-net_amd/datas.py mouth_affine / mouth_rois, csrc/k_mouth.hip; DESIGN.md
"Mouth ROIs from camera frames").  ``affine`` and ``rois`` hold the arithmetic once, in the order the C planner and the kernel use, and
are compared with them bit for bit; every numpy operation here is one correctly rounded IEEE operation (+ - * / sqrt floor rint), none
fused.  ``reference_matrix`` restates the reference's own alignment matrix (RTFSNet_file.py:32-56) for comparison only."""
import numpy as np

FACE = 256.0            # the reference's aligned face (desiredFaceWidth / Height)
EYE = (0.35, 0.35)      # ... and desiredLeftEye
TX, TY = 0.5 * FACE, EYE[1] * FACE
SPAN = 0.3 * FACE       # (1 - 2 * 0.35) * 256 up to rounding: the issue's constant is 0.3 * 256


def _check(eyes, lips, out_hw, crop_hw):
    eyes, lips = np.asarray(eyes, dtype=np.float64), np.asarray(lips, dtype=np.float64)
    if eyes.ndim < 2 or lips.ndim < 2 or eyes.shape[-2:] != (2, 2) or lips.shape[-2:] != (4, 2) or eyes.shape[:-2] != lips.shape[:-2]:
        raise ValueError(f"eyes (...,2,2) and lips (...,4,2); got {eyes.shape} and {lips.shape}")
    (Ho, Wo), (Hc, Wc) = out_hw, crop_hw
    if not (1 <= Hc <= Ho and 1 <= Wc <= Wo):
        raise ValueError(f"crop {crop_hw} must lie in [1, out {out_hw}]")
    if not (np.isfinite(eyes).all() and np.isfinite(lips).all()):
        raise ValueError("non-finite landmark")
    return eyes, lips


def affine(eyes, lips, out_hw=(96, 96), crop_hw=(88, 88)):
    """eyes (...,2,2), lips (...,4,2) -> A (...,2,3) float64: sx = A00 j + A01 i + A02, sy = A10 j + A11 i + A12."""
    eyes, lips = _check(eyes, lips, out_hw, crop_hw)
    (Ho, Wo), (Hc, Wc) = out_hw, crop_hw
    offx, offy = 0.5 - float(Wo - Wc) / 2.0, 0.5 - float(Ho - Hc) / 2.0
    with np.errstate(all="ignore"):
        xl, yl, xr, yr = eyes[..., 0, 0], eyes[..., 0, 1], eyes[..., 1, 0], eyes[..., 1, 1]
        dx, dy = xr - xl, yr - yl
        dist = np.sqrt(dx * dx + dy * dy)
        if not (dist > 0.0).all():
            raise ValueError("dist == 0: the two eye corners coincide")
        s = SPAN / dist
        a, b = s * (dx / dist), s * (dy / dist)
        cx, cy = (xl + xr) / 2.0, (yl + yr) / 2.0
        ux, uy = lips[..., 0] - cx[..., None], lips[..., 1] - cy[..., None]
        qx = (a[..., None] * ux + b[..., None] * uy) + TX
        qy = (a[..., None] * uy - b[..., None] * ux) + TY
        qx0, qy0 = qx.min(-1), qy.min(-1)
        w, h = (qx.max(-1) - qx0) + 1.0, (qy.max(-1) - qy0) + 1.0
        kx, ky = w / float(Wc), h / float(Hc)
        n2 = a * a + b * b

        def source(j, i):
            """ROI pixel (j, i) -> its aligned point by the pixel-centre rule -> p = c + R^T (q - t) / (a a + b b)."""
            gx, gy = ((qx0 + (j + offx) * kx) - 0.5) - TX, ((qy0 + (i + offy) * ky) - 0.5) - TY
            return cx + (a * gx - b * gy) / n2, cy + (b * gx + a * gy) / n2

        # the matrix is read off the composed map at three ROI pixels: the origin and one step along each axis
        (ox, oy), (jx, jy), (ix, iy) = source(0.0, 0.0), source(1.0, 0.0), source(0.0, 1.0)
        A = np.empty(eyes.shape[:-2] + (2, 3), np.float64)
        A[..., 0, 0], A[..., 0, 1], A[..., 0, 2] = jx - ox, ix - ox, ox
        A[..., 1, 0], A[..., 1, 1], A[..., 1, 2] = jy - oy, iy - oy, oy
    if not np.isfinite(A).all():
        raise ValueError("a matrix with a non-finite entry")
    return A


def aligned_points(eyes, lips, out_hw=(96, 96), crop_hw=(88, 88), M=None):
    """The aligned-face point (ax, ay) that ROI pixel (i, j) shows by cv2.resize's pixel-centre rule on the lip box, straight from the
    rule (not through ``affine``'s matrix): -> ax (..., Wo), ay (..., Ho).  M: the source -> aligned matrix (default: ``forward``)."""
    eyes, lips = _check(eyes, lips, out_hw, crop_hw)
    (Ho, Wo), (Hc, Wc) = out_hw, crop_hw
    M = forward(eyes) if M is None else M
    q = np.einsum("...rc,...kc->...kr", M[..., :2], lips) + M[..., None, :, 2]
    x0, y0 = q[..., 0].min(-1), q[..., 1].min(-1)
    w, h = q[..., 0].max(-1) - x0 + 1.0, q[..., 1].max(-1) - y0 + 1.0
    j, i = np.arange(Wo, dtype=np.float64), np.arange(Ho, dtype=np.float64)
    ax = x0[..., None] + (j - (Wo - Wc) / 2.0 + 0.5) * (w / Wc)[..., None] - 0.5
    ay = y0[..., None] + (i - (Ho - Hc) / 2.0 + 0.5) * (h / Hc)[..., None] - 0.5
    return ax, ay


def forward(eyes):
    """The forward map source -> aligned face of ``affine`` as a 2 x 3 matrix (dx / dist form)."""
    eyes = np.asarray(eyes, dtype=np.float64)
    xl, yl, xr, yr = eyes[..., 0, 0], eyes[..., 0, 1], eyes[..., 1, 0], eyes[..., 1, 1]
    dx, dy = xr - xl, yr - yl
    dist = np.sqrt(dx * dx + dy * dy)
    s = SPAN / dist
    a, b = s * (dx / dist), s * (dy / dist)
    cx, cy = (xl + xr) / 2.0, (yl + yr) / 2.0
    M = np.empty(eyes.shape[:-2] + (2, 3), np.float64)
    M[..., 0, 0], M[..., 0, 1], M[..., 0, 2] = a, b, TX - (a * cx + b * cy)
    M[..., 1, 0], M[..., 1, 1], M[..., 1, 2] = -b, a, TY - (a * cy - b * cx)
    return M


def reference_matrix(eyes):
    """RTFSNet_file.py:32-56 restated: angle by arctan2, scale from the desired eye distance, cv2.getRotationMatrix2D's formula about the
    eyes' midpoint, then the translation that puts the midpoint at (0.5 W, 0.35 H).  eyes (...,2,2) -> M (...,2,3), source -> aligned."""
    eyes = np.asarray(eyes, dtype=np.float64)
    left, right = eyes[..., 0, :], eyes[..., 1, :]
    dY, dX = right[..., 1] - left[..., 1], right[..., 0] - left[..., 0]
    angle = np.degrees(np.arctan2(dY, dX))
    desired_right_x = 1.0 - EYE[0]
    dist = np.sqrt(dX ** 2 + dY ** 2)
    scale = (desired_right_x - EYE[0]) * FACE / dist
    cx, cy = (left[..., 0] + right[..., 0]) / 2.0, (left[..., 1] + right[..., 1]) / 2.0
    alpha, beta = scale * np.cos(np.radians(angle)), scale * np.sin(np.radians(angle))  # getRotationMatrix2D(center, angle, scale)
    M = np.empty(eyes.shape[:-2] + (2, 3), np.float64)
    M[..., 0, 0], M[..., 0, 1], M[..., 0, 2] = alpha, beta, (1.0 - alpha) * cx - beta * cy
    M[..., 1, 0], M[..., 1, 1], M[..., 1, 2] = -beta, alpha, beta * cx + (1.0 - alpha) * cy
    M[..., 0, 2] += FACE * 0.5 - cx
    M[..., 1, 2] += FACE * EYE[1] - cy
    return M


def gray(frames, order):
    """uint8 (..., H, W, 3) | (..., H, W) -> float64 grey planes: OpenCV's 8-bit BGR2GRAY fixed point."""
    f = np.asarray(frames)
    if order == "gray":
        return f.astype(np.float64)
    c = f.astype(np.int64)
    B, G, R = (c[..., 0], c[..., 1], c[..., 2]) if order == "bgr" else (c[..., 2], c[..., 1], c[..., 0])
    return ((1868 * B + 9617 * G + 4899 * R + 8192) >> 14).astype(np.float64)


def _clamp(s, n):
    hi = float(n) + 1.0
    return np.where(~(s >= -2.0), -2.0, np.where(s > hi, hi, s))


def roi(frame, A, out_hw=(96, 96), order="bgr"):
    """One frame uint8 (H,W,3) | (H,W) and one map A (2,3) -> uint8 (Ho,Wo).  A plane without channels is grey whatever ``order`` says."""
    g = gray(frame, order if np.ndim(frame) == 3 else "gray")
    H, W = g.shape
    Ho, Wo = out_hw
    A = np.asarray(A, dtype=np.float64)
    j, i = np.arange(Wo, dtype=np.float64)[None, :], np.arange(Ho, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        sx = _clamp((A[0, 0] * j + A[0, 1] * i) + A[0, 2], W)
        sy = _clamp((A[1, 0] * j + A[1, 1] * i) + A[1, 2], H)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)

    def tap(y, x):
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        return np.where(ok, g[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0)

    p00, p01, p10, p11 = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
    gx, gy = 1.0 - fx, 1.0 - fy
    v = gy * (gx * p00 + fx * p01) + fy * (gx * p10 + fx * p11)
    return np.clip(np.rint(v), 0.0, 255.0).astype(np.uint8)


def rois(frames, A, out_hw=(96, 96), order="bgr"):
    """frames uint8 (n,H,W,3) | (n,H,W), A (n,2,3) | (n,K,2,3) -> uint8 (n,Ho,Wo) | (n,K,Ho,Wo)."""
    A = np.asarray(A, dtype=np.float64)
    n = len(frames)
    if A.ndim == 3:
        return np.stack([roi(frames[t], A[t], out_hw, order) for t in range(n)]) if n else np.zeros((0, *out_hw), np.uint8)
    return np.stack([np.stack([roi(frames[t], A[t, k], out_hw, order) for k in range(A.shape[1])]) for t in range(n)])
