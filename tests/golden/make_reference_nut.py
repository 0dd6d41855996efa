"""Regenerates tests/golden/reference_nut.json in the build container only: needs oracle/_ref/libnut_ref.so, which
oracle/Makefile builds from the reference's own src/nut.c.  Records what that build returns for the fixed nut_buffer script
of tests/test_host_api.py (_drive_nut) and for nut_buffer_get_f64 on u8 data (tests/test_oracle.py), so that both tests
compare with the reference also where it cannot be built.

  python tests/golden/make_reference_nut.py [out.json]
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_nut.json")
REF_NUT = os.path.join(ROOT, "oracle", "_ref", "libnut_ref.so")


def main():
    import numpy as np
    from frequensea_amd import nrf
    from tests.test_host_api import _drive_nut
    if not os.path.exists(REF_NUT):
        sys.exit("needs %s (make -C oracle with the reference present)" % REF_NUT)
    L = nrf.bind_nut(ctypes.CDLL(REF_NUT))
    data = np.arange(256, dtype=np.uint8)
    buf = L.nut_buffer_new_u8(128, 2, data.ctypes.data)
    get_f64 = [[k, L.nut_buffer_get_f64(buf, k)] for k in (0, 1, 128, 255)]
    L.nut_buffer_free(buf)
    rec = {"note": "returned by oracle/_ref/libnut_ref.so (the reference's src/nut.c): drive_nut = tests/test_host_api.py "
                   "_drive_nut; get_f64_u8 = [index, nut_buffer_get_f64] on a u8 buffer of 0..255",
           "drive_nut": json.loads(json.dumps(_drive_nut(L))), "get_f64_u8": get_f64}
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as fp:
        json.dump(rec, fp, indent=None, sort_keys=True)
        fp.write("\n")


if __name__ == "__main__":
    main()
