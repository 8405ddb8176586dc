"""numpy restatement of the reference's reconstruction filters and of ImageBlock::put, written
from the reference's lines (not from the product or the oracle, which knows only the tent):

  ReconstructionFilter::configure   src/libcore/rfilter.cpp:37-55
  evalDiscretized                   include/mitsuba/core/rfilter.h:76-77
  the plugins' constructors / eval  src/rfilters/{box,tent,gaussian,mitchell,catmullrom,lanczos}.cpp
  ImageBlock::put                   include/mitsuba/render/imageblock.h:144-189

Everything is float32 like the reference's SINGLE_PRECISION build, one rounding per operation;
expf / sinf are taken as the correctly rounded float32 value of the float64 function.
"""
import numpy as np

f = np.float32
RES = 31          # MTS_FILTER_RESOLUTION (rfilter.h:28)
BLOCK = 32        # the render blocks (mitsuba.cpp:144)
KINDS = ("box", "tent", "gaussian", "mitchell", "catmullrom", "lanczos")


def _expf(x):
    return f(np.exp(np.float64(x)))


def _sinf(x):
    return f(np.sin(np.float64(x)))


def _cubic(x, B, C):
    """mitchell.cpp:55-69 / catmullrom.cpp:40-55: int * float products convert the int first"""
    x = abs(x)
    x2 = f(x * x)
    x3 = f(x2 * x)
    sixth = f(1) / f(6)
    if x < 1:
        return f(sixth * f(f(f(f(f(12) - f(f(9) * B)) - f(f(6) * C)) * x3)
                           + f(f(f(f(-18) + f(f(12) * B)) + f(f(6) * C)) * x2)
                           + f(f(6) - f(f(2) * B))))
    if x < 2:
        return f(sixth * f(f(f(f(f(f(-B) - f(f(6) * C)) * x3) + f(f(f(f(6) * B) + f(f(30) * C)) * x2))
                             + f(f(f(f(-12) * B) - f(f(48) * C)) * x))
                           + f(f(f(8) * B) + f(f(24) * C))))
    return f(0)


def configure(kind, radius=None, stddev=None, B=None, C=None, lobes=None):
    """-> (lut float32[32], scale, radius, border) of plugin `kind` with its parameters (None:
    the plugin's default)"""
    stddev = f(0.5 if stddev is None else stddev)
    B = f(f(1) / f(3) if B is None else B)
    C = f(f(1) / f(3) if C is None else C)
    if kind == "box":
        r = f(f(0.5 if radius is None else radius) + f(1e-5))        # box.cpp:38
        ev = lambda x: f(1) if abs(x) <= r else f(0)                 # noqa: E731  box.cpp:46-48
    elif kind == "tent":
        r = f(1)                                                     # tent.cpp:34
        ev = lambda x: max(f(0), f(f(1) - abs(f(x / r))))            # noqa: E731  tent.cpp:42-44
    elif kind == "gaussian":
        r = f(f(4) * stddev)                                         # gaussian.cpp:35-38
        alpha = f(f(-1) / f(f(f(2) * stddev) * stddev))

        def ev(x):                                                   # gaussian.cpp:52-57
            return max(f(0), f(_expf(f(f(alpha * x) * x)) - _expf(f(f(alpha * r) * r))))
    elif kind == "mitchell":
        r = f(2)                                                     # mitchell.cpp:35
        ev = lambda x: _cubic(x, B, C)                               # noqa: E731
    elif kind == "catmullrom":
        r = f(2)                                                     # catmullrom.cpp:32
        ev = lambda x: _cubic(x, f(0), f(0.5))                       # noqa: E731
    elif kind == "lanczos":
        r = f(3 if lobes is None else int(lobes))                    # lanczos.cpp:35

        def ev(x):                                                   # lanczos.cpp:43-55
            x = abs(x)
            if x < f(1e-4):                                          # Epsilon, constants.h:28
                return f(1)
            if x > r:
                return f(0)
            x1 = f(f(np.pi) * x)                                     # M_PI_FLT, constants.h:63,80
            x2 = f(x1 / r)
            return f(f(_sinf(x1) * _sinf(x2)) / f(x1 * x2))
    else:
        raise ValueError(kind)
    vals = np.zeros(RES + 1, f)
    total = f(0)
    for i in range(RES):                                             # rfilter.cpp:42-46
        vals[i] = ev(f(f(r * f(i)) / f(RES)))
        total = f(total + vals[i])
    scale = f(f(RES) / r)                                            # :49
    border = int(np.ceil(f(r - f(0.5))))                             # :50
    total = f(total * f(f(f(2) * r) / f(RES)))                       # :51
    norm = f(f(1) / total)
    vals[:RES] = vals[:RES] * norm                                   # :53-54 (vals[RES] = 0, :48)
    return vals, scale, r, border


def put(pos, rgb, flt):
    """ImageBlock::put of every sample into the block of its pixel (offset = the block's corner,
    border = the filter's; imageblock.h:158-186), the blocks' interiors and borders then added
    into one film cropped to the image (Film::put of a block, renderproc.cpp:142-145).

    pos (H, W, n, 2), rgb (H, W, n, 3): sample j of pixel (x, y), lying in that pixel.  The
    weights are the float32 LUT entries and their float32 product; the sums are float64.
    -> (film (H, W, 4) float64 RGBW, mag (H, W, 4) float64 = sum |w * v|, cnt (H, W) terms)"""
    lut, scale, radius, border = flt
    H, W, n = pos.shape[:3]
    py, px = [a.ravel() for a in np.broadcast_arrays(np.arange(H)[:, None, None], np.arange(W)[None, :, None],
                                                     np.zeros((1, 1, n), int))[:2]]
    p = np.ascontiguousarray(pos, f).reshape(-1, 2)
    v = np.ascontiguousarray(rgb, f).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(v).all(axis=1) & (v >= 0).all(axis=1)    # imageblock.h:147-151
    cx, cy = (px // BLOCK) * BLOCK, (py // BLOCK) * BLOCK            # m_offset
    sx = np.minimum(BLOCK, W - cx) + 2 * border                      # the block bitmap's size
    sy = np.minimum(BLOCK, H - cy) + 2 * border
    ox, oy = (cx - border).astype(f), (cy - border).astype(f)
    rx = ((p[:, 0] - f(0.5)) - ox).astype(f)                         # :158-160
    ry = ((p[:, 1] - f(0.5)) - oy).astype(f)
    x0 = np.maximum(np.ceil(rx - radius).astype(np.int64), 0)        # :163-166
    y0 = np.maximum(np.ceil(ry - radius).astype(np.int64), 0)
    x1 = np.minimum(np.floor(rx + radius).astype(np.int64), sx - 1)
    y1 = np.minimum(np.floor(ry + radius).astype(np.int64), sy - 1)
    val = np.concatenate([np.where(valid[:, None], v, 0), np.ones((len(v), 1), f)], axis=1).astype(np.float64)
    film = np.zeros((H * W, 4))
    mag = np.zeros((H * W, 4))
    cnt = np.zeros(H * W, np.int64)
    span = 2 * int(np.ceil(radius)) + 2
    for dy in range(span):
        yy = y0 + dy
        wy = lut[np.minimum(np.abs((yy.astype(f) - ry) * scale).astype(np.int64), RES)]   # :171-172
        gy = yy + (cy - border)
        for dx in range(span):
            xx = x0 + dx
            wx = lut[np.minimum(np.abs((xx.astype(f) - rx) * scale).astype(np.int64), RES)]
            gx = xx + (cx - border)
            ok = valid & (xx <= x1) & (yy <= y1) & (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)
            w = (wx * wy).astype(f).astype(np.float64)               # :181
            idx = (gy * W + gx)[ok]
            term = w[ok, None] * val[ok]
            for c in range(4):
                film[:, c] += np.bincount(idx, weights=term[:, c], minlength=H * W)
                mag[:, c] += np.bincount(idx, weights=np.abs(term[:, c]), minlength=H * W)
            cnt += np.bincount(idx, minlength=H * W)
    return film.reshape(H, W, 4), mag.reshape(H, W, 4), cnt.reshape(H, W)


def bound(mag, cnt):
    """the fp32 summation bound of a pixel's n terms (each product rounded once, then n - 1
    additions in any order): n * 2^-24 * sum |w * v|"""
    return cnt[..., None] * 2.0 ** -24 * mag
