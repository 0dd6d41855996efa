"""Line-by-line numpy restatements of the reference's interpolator (src/nrf.c:442-496) and of the frame loop of its movie
tool (c/gradual-noise.c:54-112), for the tests of fsea_interp_* and nrf_interpolator_*.  tests/test_interp_host.py pins
both to tests/golden/interp_golden.npz, which was recorded from builds of the reference's own sources."""
import math

import numpy as np


def cast_u8(v):
    """x86-64's (uint8_t)(double) per element: cvttsd2si to int32 (0x80000000 for NaN and out of range), the low byte."""
    v = np.asarray(v, dtype=np.float64)
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    t = np.trunc(np.where(ok, v, 0.0)).astype(np.int64)
    return np.where(ok, t & 0xff, 0).astype(np.uint8)


def blend_frames(a, b, weights):
    """nrf_interpolator_get_buffer for every t of weights: (len(weights), n) of a's dtype (uint8 or float64)."""
    a, b = np.asarray(a), np.asarray(b)
    out = np.empty((len(weights), a.size), dtype=a.dtype)
    with np.errstate(all="ignore"):
        va, vb = (a / 256.0, b / 256.0) if a.dtype == np.uint8 else (a, b)
        for f, t in enumerate(np.asarray(weights, dtype=np.float64)):
            v = va * (1.0 - t) + vb * t
            out[f] = cast_u8(v * 256.0) if a.dtype == np.uint8 else v
    return out


class Interpolator:
    """The state machine of nrf_interpolator_process, its `else` without braces included."""

    def __init__(self, step):
        self.step, self.t, self.a, self.b = step, -1.0, None, None

    def process(self, block):
        if self.t < 0.0:
            self.a, self.b, self.t = np.zeros_like(block), block.copy(), 0.0
        elif self.t >= 1.0:
            self.a, self.b, self.t = self.b, block.copy(), 0.0
        else:
            self.t += self.step

    def get_buffer(self):
        return blend_frames(self.a, self.b, [self.t])[0]


def block_scale(width, height, iq_size):
    ws, hs = width / float(iq_size), height / float(iq_size)
    return ws if ws > hs else hs


def scatter_tables(width, height, iq_size):
    """put_block / put_pixel in one dimension each: the sample that wrote pixel column / row p last, -1 for none."""
    scale = block_scale(width, height, iq_size)
    tabs = []
    for side in (width, height):
        tab = np.full(side, -1, dtype=np.int32)
        for x in range(iq_size):
            d = 0
            while d < scale:
                p = int(x * scale + d)
                if p < side:
                    tab[p] = x
                d += 1
        tabs.append(tab)
    return tabs


def scatter_image(colours, width, height):
    """The tool's two nested loops as they stand: colours (iq_size, iq_size) -> (height, width), 0 where nothing lands."""
    iq_size = colours.shape[0]
    scale = block_scale(width, height, iq_size)
    img = np.zeros((height, width), dtype=np.uint8)
    for y in range(iq_size):
        for x in range(iq_size):
            dy = 0
            while dy < scale:
                dx = 0
                while dx < scale:
                    px, py = int(x * scale + dx), int(y * scale + dy)
                    if not (px >= width or py >= height):
                        img[py, px] = colours[y, x]
                    dx += 1
                dy += 1
    return img


def colours(a, b, w, iq_size, flip=True):
    """The (iq_size, iq_size) colours of one frame: lerp of the I bytes with the already eased weight w, clamp, (int)."""
    n = iq_size * iq_size
    ai = np.asarray(a, dtype=np.uint8)[0:2 * n:2].astype(np.int64)
    bi = np.asarray(b, dtype=np.uint8)[0:2 * n:2].astype(np.int64)
    if flip:
        ai, bi = (ai + 128) % 256, (bi + 128) % 256
    with np.errstate(all="ignore"):
        pwr = ai.astype(np.float64) * (1.0 - w) + bi.astype(np.float64) * w
        c = np.where(pwr < 0, 0.0, np.where(pwr > 255, 255.0, pwr))    # the tool's clamp: a NaN passes
        return cast_u8(np.where(np.isnan(c), np.nan, np.trunc(c))).reshape(iq_size, iq_size)


def image_frames(a, b, weights, width, height, iq_size, flip=True):
    col, row = scatter_tables(width, height, iq_size)
    assert col.min() >= 0 and row.min() >= 0
    return np.stack([colours(a, b, w, iq_size, flip)[row][:, col] for w in weights])


def sine_ease_in_out(p):
    return 0.5 * (1 - math.cos(p * math.pi))


def pair_weights(step):
    """(t values, eased weights) of the frames of one pair of captures: t += step from 0 until t >= 1.0."""
    ts, t = [], 0.0
    while True:
        ts.append(t)
        t += step
        if t >= 1.0:
            break
    return ts, [sine_ease_in_out(t) for t in ts], t
