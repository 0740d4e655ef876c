"""CPU characterisation test of the packed-weight plan of api.hip: for every case of pack_plan_cases.py, under every dtype and in both
directions, rsis_conv_pack_job_fill and the two size queries must answer exactly what tests/golden/pack_plans.json holds -- recorded
from a build of the commit BEFORE the plan became one function (tools/gen_pack_plans.py), never from the code under test -- and a plan
must never write more bytes than the size query of its direction allots."""
import json
import os

import pytest

import pack_plan_cases as P
from rsis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_IDS = [P.plan_id(case[0], dn, dgrad) for case in P.CASES for dn, _dt in P.DTYPES for dgrad in (0, 1)]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pack_plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plans():
    assert os.environ.get("RSIS_CONV_F2") is None, "RSIS_CONV_F2 switches the layout of the strided 3x3 forward: run with it unset"
    return P.record_all(_lib.lib(), _lib.PackJob)


def test_golden_covers_the_case_table(golden):
    assert golden["cases"] == [list(c) for c in P.CASES]
    assert sorted(golden["plans"]) == sorted(PLAN_IDS) and len(PLAN_IDS) == len(P.CASES) * 6


def test_case_table_holds_what_it_claims(golden):
    """the edges the table names are really in the recorded values: accepted, refused, and the one plan smaller than its buffer"""
    g = golden["plans"]
    assert g["s2_two_segs/f32/dgrad"]["imode"] == 1 and g["repack3_3x3_s2/f32/dgrad"]["imode"] == 4
    assert g["wino_64_64/f32_wino/fwd"]["imode"] == 7 and g["wino_64_64/f32_wino/dgrad"]["imode"] == 8
    assert g["wino_subset/f32_wino/fwd"]["blocks"] == -1 and g["wino_subset/f32_wino/dgrad"]["blocks"] > 0
    assert g["wino_dgrad_two_segs/f32_wino/dgrad"]["imode"] == 8 and g["wino_dgrad_two_segs/f32_wino/fwd"]["imode"] == 2
    for d in ("fwd", "dgrad"):
        assert g["lstm_hid32_ks3/bf16/" + d]["blocks"] > 0 and g["lstm_hid32_ks1/bf16/" + d]["blocks"] == -1
        assert g["lstm_hid32_ks1/f32/" + d]["blocks"] > 0
        for dn, _dt in P.DTYPES:
            for name in ("cout_not_4_hid", "segment_past_ctot", "nseg_0", "nseg_4", "weight_2_31_elements"):
                assert g["%s/%s/%s" % (name, dn, d)]["blocks"] == -1


@pytest.mark.parametrize("pid", PLAN_IDS)
def test_plan_reproduces_the_recorded_one(pid, golden, plans):
    assert plans[pid] == golden["plans"][pid]


@pytest.mark.parametrize("pid", PLAN_IDS)
def test_plan_fits_its_size_query(pid, plans):
    """an accepted plan writes no more than the size query of its direction returns, and exactly that much everywhere but the
    3x3 / stride 2 data gradient (whose query has no segment list and leaves room for either of its two layouts)"""
    p = plans[pid]
    if p["blocks"] < 0:
        assert (p["imode"], p["krows"], p["ldw"]) == (-7, -7, -7), "a refused job must be left as it was"
        return
    dgrad = pid.endswith("/dgrad")
    room = p["bytes_dgrad"] if dgrad else p["bytes_fwd"]
    wrote = P.written_bytes(p["imode"], p["krows"], p["ldw"])
    assert 0 < wrote <= room
    case = next(c for c in P.CASES if pid.startswith(c[0] + "/"))
    s2_dgrad = dgrad and case[3:6] == (3, 2, 1)
    assert wrote == room or s2_dgrad, (wrote, room)
