"""CPU tier: the guard-band comparison of tests/guarded.py names the band, the offsets and the count of what changed, and
reports clean when nothing did -- the checker of tests/test_gpu_bounds.py has teeth."""
import numpy as np
import pytest

from tests.guarded import FILL, GUARD, describe, dirty_bytes

SMALL = 64


def banded(guard, nbytes, fill=FILL):
    back = np.full(2 * guard + nbytes, fill, np.uint8)
    back[guard:guard + nbytes] = np.arange(nbytes, dtype=np.uint8)     # the payload may hold anything, `fill` included
    return back


@pytest.mark.parametrize("guard", [SMALL, GUARD])
@pytest.mark.parametrize("nbytes", [0, 1, 24, 4097])
def test_clean_bands_report_nothing(guard, nbytes):
    assert dirty_bytes(banded(guard, nbytes), guard, nbytes, FILL) == []


@pytest.mark.parametrize("guard", [SMALL, GUARD])
@pytest.mark.parametrize("nbytes", [0, 24, 4097])
@pytest.mark.parametrize("where", ["front last", "back first", "back last"])
def test_one_changed_byte_is_named_by_band_and_offset(guard, nbytes, where):
    index, band, offset = {"front last": (guard - 1, "front", -1),
                           "back first": (guard + nbytes, "back", 0),
                           "back last": (2 * guard + nbytes - 1, "back", guard - 1)}[where]
    back = banded(guard, nbytes)
    back[index] ^= 0x01
    assert dirty_bytes(back, guard, nbytes, FILL) == [(band, offset, offset, 1)]
    assert band in describe(dirty_bytes(back, guard, nbytes, FILL))


@pytest.mark.parametrize("nbytes", [0, 24])
def test_first_byte_of_the_front_band_and_a_run_in_the_back_band(nbytes):
    back = banded(SMALL, nbytes)
    back[0] = 0
    back[SMALL + nbytes:SMALL + nbytes + 8] = 0          # one complex64 behind the payload
    back[SMALL + nbytes + 3] = FILL                      # a byte that happens to equal the fill is not counted
    assert dirty_bytes(back, SMALL, nbytes, FILL) == [("front", -SMALL, -SMALL, 1), ("back", 0, 7, 7)]


def test_the_payload_is_not_looked_at_and_another_fill_is_honoured():
    back = banded(SMALL, 100, fill=0x00)
    assert dirty_bytes(back, SMALL, 100, 0x00) == []
    assert dirty_bytes(back, SMALL, 100, 0xFF) == [("front", -SMALL, -1, SMALL), ("back", 0, SMALL - 1, SMALL)]
    with pytest.raises(AssertionError):
        dirty_bytes(back[:-1], SMALL, 100, 0x00)         # a buffer of another size is a mistake of the caller's
