"""Writes tests/golden/spectra_messages.json: code and fsea_last_error_string() of every case of tests/test_spectra_host.py.

The table records what a caller of fsea_spectra_* saw when the object was added: the codes, the texts and, through the cases
that break two rules at once, the order of the checks.  Run this to record a new case, never to bless what a changed check
says.  From the repository root:  python -m tests.golden.make_spectra_messages
"""
import json

from tests import test_spectra_host as T

if __name__ == "__main__":
    table = {case[0]: T.call(case) for case in T.CASES}
    with open(T.TABLE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(table), T.TABLE))
