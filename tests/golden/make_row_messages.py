"""Writes tests/golden/row_messages.json: code and fsea_last_error_string() of every case of tests/test_row_messages.py.

The table is a record of the library BEFORE fsea_persist, fsea_cfar and fsea_events got their shared checks
(csrc/fsea_rows.h): run this against a libfsea_hip.so built from that commit's csrc/, never to bless what a changed check
says.  The fsea_oscfar_* entries are a record of commit 510f74d, the last one before fsea_cfar and fsea_oscfar got their
shared scaffold (csrc/fsea_cfar_shared.h); they were added with that commit's csrc/ built, and the other entries came out
byte for byte as they were.  From the repository root:  python -m tests.golden.make_row_messages
"""
import json

from tests import test_row_messages as T

if __name__ == "__main__":
    table = {case[0]: T.call(case) for case in T.CASES}
    with open(T.TABLE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(table), T.TABLE))
