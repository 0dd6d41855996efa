"""Writes tests/golden/job_messages.json: code and fsea_last_error_string() of every case of tests/test_job_messages.py.

The table is a record of the library BEFORE the objects' checks were shared (csrc/fsea_jobs.h): the fsea_extract_* and
fsea_measure_* entries from before the two got their shared checks, the fsea_audio_* entries from the commit that added the
object, before its placement check and host form moved there.  Run this against a libfsea_hip.so built from such a commit's
csrc/, never to bless what a changed check says.  From the repository root:  python -m tests.golden.make_job_messages
"""
import json

from tests import test_job_messages as T

if __name__ == "__main__":
    table = {case[0]: T.call(case) for case in T.CASES}
    with open(T.TABLE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(table), T.TABLE))
