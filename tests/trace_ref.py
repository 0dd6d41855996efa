"""Numpy restatement of the frame loop of the reference's single-sample tool (c/single-sample.c:126-149), for the tests of
fsea_trace_* and fsea-single-sample, in two forms: the literal loop (pixel_inc hit by hit, in the tool's order) and the
order-free one the kernels rest on (per-pixel hit counts h of a frame, then v + p min(h, (254 - v) / p)).
tests/test_trace_host.py pins both to tests/golden/trace_golden.npz, recorded from a build of the reference's own source.

Where the tool reads past its buffer (a size that is no multiple of the step, an odd step on the last frame) the rule here
is the one of include/fsea.h: a point exists only where both its bytes lie inside the data."""
import numpy as np



def draw_lines_counts(x1, y1, x2, y2, stride):
    """The tool's draw_line, one iteration of its loop for all segments at once (as tests/test_iq_draw_host.py has it, with
    the pixels collected and counted once at the end); returns the hits per pixel."""
    x1, y1, x2, y2 = (np.asarray(v, dtype=np.int64).copy() for v in (x1, y1, x2, y2))
    dx, dy = np.abs(x2 - x1), np.abs(y2 - y1)
    sx, sy = np.where(x1 < x2, 1, -1), np.where(y1 < y2, 1, -1)
    err = np.where(dx > dy, dx // 2, -(dy // 2))                # (dx > dy ? dx : -dy) / 2, C truncation
    x, y = x1, y1
    pixels = []
    while x.size:
        pixels.append(y * stride + x)
        go = ~((x == x2) & (y == y2))
        x, y, x2, y2, dx, dy, sx, sy, err = (v[go] for v in (x, y, x2, y2, dx, dy, sx, sy, err))
        e2 = err.copy()
        mx, my = e2 > -dx, e2 < dy
        err = err - dy * mx + dx * my
        x = x + sx * mx
        y = y + sy * my
    return np.bincount(np.concatenate(pixels), minlength=stride * stride)


def geometry(width, height, m):
    side = 256 * m
    return side, (width - side) // 2, (height - side) // 2


def frame_points(data, f, frame_bytes, flip=True):
    """The points (x, y) of frame f: bytes (2k, 2k + 1) from f * frame_bytes on, 2k < frame_bytes, both inside the data."""
    j = f * frame_bytes
    n = min((frame_bytes + 1) // 2, max(0, (len(data) - j) // 2))
    b = np.asarray(data[j:j + 2 * n], dtype=np.uint8).astype(np.int64)
    if flip:
        b = (b + 128) % 256
    return b[0::2], b[1::2]


def n_frames_of(size, frame_bytes):
    """The tool's j = 0, S, 2 S, ... < size."""
    return -(-size // frame_bytes)


def literal_frames(data, frame_bytes, n_frames, width=1920, height=1080, m=4, p=4, f=0, flip=True, canvas=None):
    """The tool's loops as they stand, one pixel_inc call per hit.  Returns (frames, canvas)."""
    side, ox, oy = geometry(width, height, m)
    canvas = np.zeros((height, width), dtype=np.uint8) if canvas is None else canvas.copy()
    out = np.empty((n_frames, height, width), dtype=np.uint8)
    img = canvas.astype(np.int64)
    for n in range(n_frames):
        if f > 0:
            img = np.maximum(img - f, 0)
        xs, ys = frame_points(data, n, frame_bytes, flip)
        for k in range(1, len(xs)):
            x1, y1, x2, y2 = int(xs[k - 1]) * m, int(ys[k - 1]) * m, int(xs[k]) * m, int(ys[k]) * m
            dx, dy = abs(x2 - x1), abs(y2 - y1)
            sx, sy = (1 if x1 < x2 else -1), (1 if y1 < y2 else -1)
            err = (dx if dx > dy else -dy)
            err = -(-err // 2) if err < 0 else err // 2             # C's division truncates
            while True:
                if not (x1 == 0 or y1 == 0 or x1 == width - 1 or y1 == height - 1):
                    v = img[y1 + oy, x1 + ox]
                    if not v + p >= 255:
                        img[y1 + oy, x1 + ox] = v + p
                if x1 == x2 and y1 == y2:
                    break
                e2 = err
                if e2 > -dx:
                    err -= dy
                    x1 += sx
                if e2 < dy:
                    err += dx
                    y1 += sy
        out[n] = img
    return out, img.astype(np.uint8)


def frame_hits(data, n, frame_bytes, width, height, m, flip=True):
    """Hits per pixel of the IQ square in frame n, (side, side) int64, the skipped borders left out."""
    side = 256 * m
    xs, ys = frame_points(data, n, frame_bytes, flip)
    if len(xs) < 2:
        return np.zeros((side, side), dtype=np.int64)
    h = draw_lines_counts(xs[:-1] * m, ys[:-1] * m, xs[1:] * m, ys[1:] * m, side).reshape(side, side)
    h[0, :] = 0
    h[:, 0] = 0
    if width - 1 < side:
        h[:, width - 1] = 0
    if height - 1 < side:
        h[height - 1, :] = 0
    return h


def frames(data, frame_bytes, n_frames, width=1920, height=1080, m=4, p=4, f=0, flip=True, canvas=None):
    """The order-free form.  Returns (frames, canvas)."""
    side, ox, oy = geometry(width, height, m)
    img = (np.zeros((height, width), dtype=np.int64) if canvas is None else canvas.astype(np.int64))
    out = np.empty((n_frames, height, width), dtype=np.uint8)
    for n in range(n_frames):
        img = np.maximum(img - f, 0)
        h = frame_hits(data, n, frame_bytes, width, height, m, flip)
        sq = img[oy:oy + side, ox:ox + side]
        sq += p * np.minimum(h, (254 - sq) // p)
        out[n] = img
    return out, img.astype(np.uint8)
