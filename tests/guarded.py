"""Guard bands round a device buffer: `guard` bytes of `fill` in front of and behind a payload of exactly nbytes, in one
fsea.DeviceBuffer.  A kernel that stores outside the buffer it was given dirties a band; one whose result depends on bytes
behind its input gives another result when the bands hold another fill.  dirty_bytes() is the comparison itself, plain numpy
(tests/test_guarded_host.py); Guarded needs a GPU (tests/test_gpu_bounds.py)."""
import numpy as np

GUARD = 1 << 16     # the band width of the FFT tests (tests/test_gpu_parity.py, tests/test_gpu_anysize.py)
FILL = 0xA5


def dirty_bytes(back, guard, nbytes, fill):
    """back: the guard + nbytes + guard bytes of a guarded buffer as they came back.  [] where both bands still hold `fill`,
    otherwise one (band, first, last, count) per dirtied band: band is "front" or "back"; first and last are the offsets of
    the first and last dirtied byte from the payload's edge (front: -1 is the byte just before the payload, -guard the
    band's first; back: 0 is the byte just behind the payload, guard - 1 the band's last); count is how many differ."""
    back = np.asarray(back, dtype=np.uint8).ravel()
    assert back.size == 2 * guard + nbytes, (back.size, guard, nbytes)
    found = []
    for band, lo, origin in (("front", 0, guard), ("back", guard + nbytes, guard + nbytes)):
        bad = np.flatnonzero(back[lo:lo + guard] != fill)
        if bad.size:
            found.append((band, int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin, int(bad.size)))
    return found


def describe(found):
    return "; ".join("%s band: %d bytes changed, offsets %d..%d from the payload's edge" % (b, c, f, l) for b, f, l, c in found)


class Guarded:
    """guard + nbytes + guard bytes of device memory, all `fill` (the payload too: an element the kernel should have written
    and did not shows as well).  .addr is the payload's address, 16-byte aligned; with nbytes == 0 the bands touch and
    .addr is still a pointer to hand to a call that must write nothing."""

    def __init__(self, nbytes, fill=FILL, guard=GUARD):
        from frequensea_amd import fsea
        assert guard > 0 and guard % 16 == 0 and nbytes >= 0
        self.nbytes, self.fill, self.guard = int(nbytes), fill, guard
        self.buf = fsea.DeviceBuffer(2 * guard + self.nbytes)
        self.buf.upload(np.full(2 * guard + self.nbytes, fill, np.uint8))
        self.addr = self.buf.ptr.value + guard
        assert self.addr % 16 == 0

    def upload(self, arr, byte_offset=0):
        """The bytes of a host array into the payload (from byte_offset of it on); returns self."""
        from frequensea_amd import fsea
        arr = np.ascontiguousarray(arr)
        assert 0 <= byte_offset and byte_offset + arr.nbytes <= self.nbytes, (byte_offset, arr.nbytes, self.nbytes)
        if arr.nbytes:
            fsea._check(fsea.hip_lib().fsea_copy_to_device(self.buf.device, self.addr + byte_offset, arr.ctypes.data, arr.nbytes))
        return self

    def payload(self, dtype, shape):
        """The payload (its first prod(shape) elements) as a new host array."""
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes, (out.nbytes, self.nbytes)
        if out.nbytes:
            out = self.buf.download(dtype, shape, byte_offset=self.guard)
        return out

    def dirty(self):
        back = self.buf.download(np.uint8, (2 * self.guard + self.nbytes,))
        return dirty_bytes(back, self.guard, self.nbytes, self.fill)

    def check(self, what=""):
        found = self.dirty()
        assert not found, "%s: %s" % (what, describe(found))

    def free(self):
        self.buf.free()
