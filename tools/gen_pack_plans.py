#!/usr/bin/env python
"""Record tests/golden/pack_plans.json: the packed-weight plan of every case of tests/pack_plan_cases.py as a KNOWN-GOOD build of the
library answers it.  Needs no GPU (the size queries and rsis_conv_pack_job_fill launch nothing).

    RSIS_HIP_LIB=<librsis_hip.so of the parent commit> python tools/gen_pack_plans.py

The file is a characterisation of the parent's behaviour: tests/test_pack_plan_host.py asserts that the current build reproduces it.
Never regenerate it from the code under test -- the script refuses to run without RSIS_HIP_LIB for that reason.  RSIS_CONV_F2 must be
unset (it switches the layout of the strided 3x3 forward)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    if not os.environ.get("RSIS_HIP_LIB"):
        sys.exit("set RSIS_HIP_LIB to a build of the parent commit's library")
    if os.environ.get("RSIS_CONV_F2") is not None:
        sys.exit("unset RSIS_CONV_F2")
    import pack_plan_cases as P
    from rsis_amd import _lib
    plans = P.record_all(_lib.lib(), _lib.PackJob)
    out = os.path.join(ROOT, "tests", "golden", "pack_plans.json")
    with open(out, "w") as f:
        json.dump({"cases": [list(c) for c in P.CASES], "plans": plans}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d plans to %s" % (len(plans), out))


if __name__ == "__main__":
    main()
