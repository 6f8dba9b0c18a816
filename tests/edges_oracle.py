"""Oracle of packed edge maps (include/cvlm.h: cvlm_edge_pack): the float32 restatement of the align_corners=False bilinear
value v, written operation by operation with an explicit .astype(float32) behind each -- one rounding per written operation, nothing
fused --, then the threshold, numpy.packbits, the areas and the intersections with a second set of packed planes.  `plain` is the same
definition as a double loop over output pixels in Python scalars of numpy.float32; the test files hold the two against each other,
against torch.nn.functional.interpolate and against the library's host and device entries."""
import numpy as np

f32 = np.float32
MARGIN = 2.0 ** -21     # |v - F.interpolate| on operands in [0, 1]: at most nine roundings of <= 2^-25 each differ, with a factor of two


def taps(n_in: int, n_out: int):
    """(i0, i1, l) of every output index along one axis: s = f32(n_in) / f32(n_out); f = max(s * (o + 0.5) - 0.5, 0), the product
    rounded before the subtraction; i0 = int(f) capped at n_in - 1; i1 = i0 + (i0 < n_in - 1); l = f - i0."""
    s = f32(n_in) / f32(n_out)
    assert s.dtype == f32
    o = np.arange(n_out, dtype=np.int64).astype(f32)
    half = (o + f32(0.5)).astype(f32)
    prod = (s * half).astype(f32)
    f = (prod - f32(0.5)).astype(f32)
    f = np.where(f < f32(0), f32(0), f).astype(f32)
    i0 = np.where(f >= f32(n_in - 1), n_in - 1, f.astype(np.int64)).astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l = (f - i0.astype(f32)).astype(f32)
    return i0, i1, l


def lerp(l, a, b):
    """(1 - l) * a + l * b, each of the four operations rounded to float32."""
    wa = (f32(1) - l).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        pa = (wa * a).astype(f32)
        pb = (l * b).astype(f32)
        return (pa + pb).astype(f32)


def value(prob: np.ndarray, hout: int, wout: int) -> np.ndarray:
    """prob f32 (..., hin, win) -> v f32 (..., hout, wout)."""
    prob = np.asarray(prob)
    assert prob.dtype == f32
    hin, win = prob.shape[-2:]
    y0, y1, ly = taps(hin, hout)
    x0, x1, lx = taps(win, wout)
    top = lerp(lx, prob[..., y0, :][..., x0], prob[..., y0, :][..., x1])
    bot = lerp(lx, prob[..., y1, :][..., x0], prob[..., y1, :][..., x1])
    return lerp(ly[:, None], top, bot)


def plain(plane: np.ndarray, hout: int, wout: int) -> np.ndarray:
    """One plane, one output pixel at a time, in numpy.float32 scalars."""
    hin, win = plane.shape
    sy, sx = f32(hin) / f32(hout), f32(win) / f32(wout)

    def tap(s, o, n):
        f = f32(f32(s * f32(f32(o) + f32(0.5))) - f32(0.5))
        f = f32(0) if f < 0 else f
        i0 = n - 1 if f >= f32(n - 1) else int(f)
        return i0, i0 + (1 if i0 < n - 1 else 0), f32(f - f32(i0))

    def mix(l, a, b):
        return f32(f32(f32(f32(1) - l) * a) + f32(l * b))
    out = np.empty((hout, wout), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(hout):
            y0, y1, ly = tap(sy, y, hin)
            for x in range(wout):
                x0, x1, lx = tap(sx, x, win)
                out[y, x] = mix(ly, mix(lx, plane[y0, x0], plane[y0, x1]), mix(lx, plane[y1, x0], plane[y1, x1]))
    return out


def above(v: np.ndarray, threshold: float) -> np.ndarray:
    """v > float32(threshold): NaN compares false, +inf is set."""
    with np.errstate(invalid="ignore"):
        return v > f32(threshold)


def pack(planes: np.ndarray) -> np.ndarray:
    """bool (P, H, W) -> uint8 (P, H * W / 8) in numpy.packbits' order."""
    P = planes.shape[0]
    return np.packbits(planes.reshape(P, -1), axis=1)


def popcount(bits: np.ndarray) -> np.ndarray:
    """uint8 (P, n) -> int32 (P,) set bits."""
    return np.unpackbits(bits, axis=1).sum(axis=1).astype(np.int32)


def edge_pack(prob: np.ndarray, hout: int, wout: int, threshold: float, with_bits=None) -> dict:
    """What cvlm_edge_pack answers for prob f32 (P, hin, win): bits uint8 (P, hout * wout / 8), area int32 (P,) and, with
    with_bits uint8 like bits, with_inter int32 (P,) = popcount(bits & with_bits)."""
    assert prob.ndim == 3 and wout % 32 == 0
    bits = pack(above(value(prob, hout, wout), threshold))
    out = dict(bits=bits, area=popcount(bits))
    if with_bits is not None:
        assert with_bits.shape == bits.shape and with_bits.dtype == np.uint8
        out["with_inter"] = popcount(bits & with_bits)
    return out


def operator_cases() -> dict:
    """name -> (prob f32 (P, hin, win), hout, wout, thresholds): the shapes and values a resize-threshold-pack can go wrong at."""
    rng = np.random.default_rng(17)
    T = (0.25, 0.5, 0.9)
    c = {}
    c["one_pixel"] = (np.array([[[0.1]], [[0.6]], [[0.95]]], f32), 1, 32, T)                     # hin = win = 1: x1 / y1 clamp
    c["one_row"] = (rng.random((3, 1, 8)).astype(f32), 1, 32, T)
    c["one_column"] = (rng.random((3, 8, 1)).astype(f32), 8, 32, T)
    c["identity"] = (rng.random((3, 32, 32)).astype(f32), 32, 32, T)                             # scale 1: equals prob > t
    at_t = rng.random((2, 32, 32)).astype(f32)
    at_t[:, ::3, ::2] = f32(0.5)                                                                  # values exactly t: none is set
    c["identity_at_threshold"] = (at_t, 32, 32, (0.5,))
    c["two_by_two"] = (np.array([[[0.0, 1.0], [1.0, 0.0]], [[0.2, 0.7], [0.4, 0.95]]], f32), 8, 32, T)
    c["odd_up_a"] = (rng.random((2, 37, 53)).astype(f32), 101, 96, T)                            # non-integer scales
    c["odd_up_b"] = (rng.random((2, 53, 37)).astype(f32), 67, 160, T)
    c["down"] = (rng.random((2, 100, 100)).astype(f32), 32, 32, T)                               # the same formula shrinks
    special = rng.random((5, 12, 16)).astype(f32)
    special[0, 5, 7] = np.nan
    special[1, 3, 4], special[1, 8, 9] = np.inf, -np.inf
    special[2, ::2, ::3] = -special[2, ::2, ::3] - f32(0.5)
    special[3, 2:6, 3:9] = f32(1e-41)                                                             # float32 denormals
    special[3, 7, 7] = f32(-1e-43)
    special[4, 0, 0], special[4, 11, 15], special[4, 6, 0] = np.nan, np.nan, np.inf               # at the corners and an edge
    c["special_values"] = (special, 48, 64, T)
    yy, xx = np.mgrid[0:16, 0:16]
    c["checkerboard"] = (((yy + xx) & 1).astype(f32)[None], 64, 64, T)                            # every source cell holds a crossing
    ramp = np.empty((3, 4, 40), f32)
    ramp[0] = np.linspace(0.0, 1.0, 40, dtype=f32)                                                # rises through t along x
    ramp[1] = np.linspace(1.0, 0.0, 40, dtype=f32)
    ramp[2] = (np.arange(40) >= 8).astype(f32)            # a step between source pixels 7 and 8: crosses at the seam of words 0 / 1 at 4 x
    c["ramp"] = (ramp, 4, 160, (0.5, 0.2, 0.8))
    return c
