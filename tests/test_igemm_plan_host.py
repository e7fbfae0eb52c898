"""The launch decisions of the implicit-GEMM passes (csrc/igemm.hip: tile, loop structure, splits), asked of denet_conv_plan - which
launches nothing and needs no device - against tests/golden/igemm_plan.json: what the build before the plan functions existed ran
for the same inputs (the fixture's `meta` says how it was recorded). Every case twice: with the table of measured configurations
cleared, and with the committed denet_amd/tuned/gfx950.json imported."""
import ctypes
import json
import os

import pytest

from denet_amd import lib as dlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "igemm_plan.json")
TUNED = os.path.join(ROOT, "denet_amd", "tuned", "gfx950.json")
SWITCHES = ("DENET_IGEMM_NBUF", "DENET_IGEMM_TILE", "DENET_WGRAD_BLOCKS", "DENET_DGRAD_T_NBUF", "DENET_DGRAD_T_TILE")


def _export(L):
    n = L.denet_tune_export(None, 0)
    buf = (ctypes.c_int * (14 * max(n, 1)))()
    assert L.denet_tune_export(buf, n) == n
    return buf, n


def _plan(L, case):
    v = [ctypes.c_int() for _ in range(4)]
    rc = L.denet_conv_plan(case["pass"], *case["geom"], case["batch"], case["ws"], *[ctypes.byref(x) for x in v])
    assert rc == 0, (case, rc, L.denet_last_error())
    return [x.value for x in v]


@pytest.fixture(scope="module")
def plans():
    """{state: [plan of every case]} for the two states of the table; the process's own table is put back afterwards"""
    forced = [s for s in SWITCHES if os.environ.get(s)]
    assert not forced, "the recorded decisions are those without a forcing switch: unset %s" % forced
    with open(FIXTURE) as f:
        cases = json.load(f)["cases"]
    with open(TUNED) as f:
        rec = json.load(f)["kernels"]
    L = dlib.load()
    saved, n_saved = _export(L)
    try:
        assert L.denet_tune_clear() == 0
        cleared = [_plan(L, c) for c in cases]
        flat = (ctypes.c_int * (14 * len(rec)))(*[v for r in rec for v in r])
        assert L.denet_tune_import(flat, len(rec)) == 0
        tuned = [_plan(L, c) for c in cases]
    finally:
        assert L.denet_tune_clear() == 0
        assert L.denet_tune_import(saved, n_saved) == 0
    assert _export(L)[1] == n_saved
    return cases, rec, {"cleared": cleared, "tuned": tuned}


@pytest.mark.parametrize("state", ["cleared", "tuned"])
def test_every_recorded_decision(plans, state):
    cases, _, got = plans
    assert len(cases) >= 1500
    wrong = [(c["pass"], c["geom"], c["batch"], c["ws"], c[state], g) for c, g in zip(cases, got[state]) if g != c[state]]
    assert not wrong, "%d of %d plans differ from the recorded launches (pass, geom, batch, ws, recorded, plan): %s" % (
        len(wrong), len(cases), wrong[:5])


def test_fixture_covers_what_it_should(plans):
    """every mode 0-4 record of the tuned file is a case, every pass code and every instantiated tile / loop structure occurs, and
    the tuned table changes some answers (the second state is not a copy of the first)"""
    cases, rec, _ = plans
    have = {(c["pass"], tuple(c["geom"][:10]), c["batch"]) for c in cases}
    for r in rec:
        mode, key = r[0], r[1:11]
        if mode <= 2:
            assert (mode, tuple(key), 1) in have, r
        else:                                            # N of the key is the member count; the geometry has N = 1
            assert (mode, (1,) + tuple(key[1:]), key[0]) in have, r
    assert {c["pass"] for c in cases} == set(range(7))
    shapes = {(c["pass"] in (2, 4), tuple(c[s][:3])) for c in cases for s in ("cleared", "tuned")}
    for bm, bn in ((128, 128), (128, 64)):
        assert {(False, (bm, bn, nbuf)) for nbuf in (1, 2)} <= shapes
    for bm, bn in ((128, 128), (64, 64), (64, 128)):
        assert (True, (bm, bn, 1)) in shapes
    assert any(c["cleared"] != c["tuned"] for c in cases)
    assert any(c["pass"] == 2 and c["cleared"][3] > 1 for c in cases) and any(c["pass"] == 2 and c["ws"] and c["cleared"][3] == 1 for c in cases)


def test_plan_refuses_what_the_passes_refuse():
    L = dlib.load()
    v = [ctypes.c_int() for _ in range(4)]
    out = [ctypes.byref(x) for x in v]
    assert L.denet_conv_plan(0, 1, 8, 8, 32, 33, 3, 3, 3, 1, 1, 8, 8, 1, 0, *out) == -1000
    assert b"multiple of 32" in L.denet_last_error()
    assert L.denet_conv_plan(7, 2, 8, 8, 32, 32, 3, 3, 3, 1, 1, 8, 8, 1, 0, *out) == -1000
    assert L.denet_conv_plan(1, 2, 9, 9, 32, 32, 3, 3, 3, 2, 1, 5, 5, 1, 0, *out) == -1000      # H, W no multiple of the stride
    assert L.denet_conv_plan(0, 2, 8, 8, 32, 32, 3, 3, 3, 1, 1, 8, 8, 1, 0, None, None, None, None) == -1000
