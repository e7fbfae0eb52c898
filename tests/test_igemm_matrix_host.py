"""The case table of tests/igemm_matrix.py, without a device: every row's record makes denet_conv_plan answer the instantiation the
row is there for, and the table as a whole reaches what tests/test_igemm_matrix_gpu.py claims to run - all 27 instantiations of
csrc/igemm.hip's kernel text, each loop structure at the reduction lengths where its prologue and tail loops change shape, each tile
at its row and column tails. An edit of the table that loses one of these fails here."""
import ctypes
import os

import pytest

import igemm_matrix as M
from denet_amd import lib as dlib

SWITCHES = ("DENET_IGEMM_NBUF", "DENET_IGEMM_TILE", "DENET_WGRAD_BLOCKS", "DENET_DGRAD_T_NBUF", "DENET_DGRAD_T_TILE")


def _export(L):
    n = L.denet_tune_export(None, 0)
    buf = (ctypes.c_int * (14 * max(n, 1)))()
    assert L.denet_tune_export(buf, n) == n
    return buf, n


@pytest.fixture(scope="module")
def plans():
    """{(row id, record): plan} of every in-process row with the table holding that one record; the process's table is put back"""
    forced = [s for s in SWITCHES if os.environ.get(s)]
    assert not forced, "the table's rows are planned without a forcing switch: unset %s" % forced
    L = dlib.load()
    saved, n_saved = _export(L)
    got = {}
    try:
        for case in M.CASES:
            if case.switch is not None:
                continue
            for rec in case.records or [None]:
                assert L.denet_tune_clear() == 0
                if rec is not None:
                    M.import_record(L, *M.record_key(case), *rec)
                got[(case.id, rec)] = M.plan(L, case)
    finally:
        assert L.denet_tune_clear() == 0
        assert L.denet_tune_import(saved, n_saved) == 0
    assert _export(L)[1] == n_saved
    return got


def test_every_row_plans_what_it_is_there_for(plans):
    assert len(plans) >= 400
    wrong = [(k, M.intended(M.BY_ID[k[0]], k[1]), v) for k, v in plans.items() if v != M.intended(M.BY_ID[k[0]], k[1])]
    assert not wrong, "%d of %d (row, record): intended, plan: %s" % (len(wrong), len(plans), wrong[:5])


def _launches():
    """(row, mode, bm, bn, nbuf, splits) of every launch of the table, the child-process rows included"""
    for case in M.CASES:
        for rec in case.records or [None]:
            bm, bn, nbuf, splits = M.intended(case, rec)
            yield case, M.KERNEL_MODE[case.code], bm, bn, nbuf, splits


def test_the_table_reaches_all_27_instantiations():
    here = {(m, bm, bn, nb) for c, m, bm, bn, nb, _ in _launches() if c.switch is None}
    child = {(m, bm, bn, nb) for c, m, bm, bn, nb, _ in _launches() if c.switch is not None}
    assert here | child == M.INSTANTIATIONS
    # MODE_DGRAD_T reads no record: its rule reaches two instantiations in this process, the other four are child-process cases
    assert {k for k in here if k[0] == 3} == {(3, 128, 64, 1), (3, 128, 64, 2)}
    assert child - here == {(3, 128, 128, 1), (3, 128, 128, 2), (3, 128, 128, 3), (3, 128, 64, 3)}
    assert {c.switch for c in M.CASES if c.switch} == set(M.DGRAD_T_CHILDREN)
    # the batched products run the three-buffer loop as well, on both of their passes
    assert (128, 128, 3, 16) in [M.intended(M.BY_ID["gemm_b_fwd"], r) for r in M.BY_ID["gemm_b_fwd"].records]
    assert (128, 128, 3, 1) in [M.intended(M.BY_ID["wgrad_b"], r) for r in M.BY_ID["wgrad_b"].records]


def test_every_loop_structure_meets_the_reduction_lengths_where_it_changes_shape():
    """the pipelined loop's prologue depends on nsteps > 1 and nsteps > NBUF - 1, its four tail loops on nsteps against NBUF - 1:
    1 ... 5 chunks take every combination for NBUF = 2 and 3, 9 or more reach the steady state; a parity class without a tap has 0"""
    seen = {}
    for case, mode, bm, bn, nbuf, splits in _launches():
        seen.setdefault((mode, nbuf), set()).update(M.steps(case, splits if mode == 2 else 1))
    assert set(seen) == {(m, nb) for m in range(4) for nb in (1, 2, 3)}
    for (mode, nbuf), st in seen.items():
        assert {1, 2, 3, 4, 5} <= st and max(st) >= 9, (mode, nbuf, sorted(st))
        if mode in (1, 3):
            assert 0 in st, (mode, nbuf)


def test_every_tile_meets_its_row_and_column_tails():
    rows_of, cols_of = {}, {}
    for case, mode, bm, bn, nbuf, splits in _launches():
        rows, cols = M.rows_cols(case)
        rows_of.setdefault((mode, bm, bn), set()).add(rows)
        cols_of.setdefault((mode, bm, bn), set()).add(cols)
    assert set(rows_of) == {(m, bm, bn) for m, tl in M.TILES.items() for bm, bn in tl}
    for (mode, bm, bn), rows in rows_of.items():
        assert any(r > bm and r % bm for r in rows), ("no partial row tile behind a full one", mode, bm, bn)
        # (the 128 x 128 filter-gradient tile is chosen from 128 rows on: it always has a full tile)
        assert any(r < bm for r in rows) or (mode, bm, bn) == (2, 128, 128), ("no launch with fewer rows than a tile", mode, bm, bn)
        assert any(c % bn for c in cols_of[(mode, bm, bn)]), ("no partial last column tile", mode, bm, bn)


def test_every_filter_gradient_tile_meets_short_slices_and_partial_chunks():
    slices, partial = {}, {}
    for case, mode, bm, bn, nbuf, splits in _launches():
        if mode != 2:
            continue
        st = M.steps(case, splits)
        assert sum(st) == -(-M.npix(case) // M.BK) and min(st) > 0
        slices.setdefault((bm, bn, nbuf), []).append(st)
        partial.setdefault((bm, bn, nbuf), set()).add(M.npix(case) % M.BK)
    assert set(slices) == {(bm, bn, nb) for bm, bn in M.TILES[2] for nb in (1, 2, 3)}
    for key, sts in slices.items():
        assert any(len(st) > 1 and st[-1] < st[0] for st in sts), ("no shorter last slice", key)
        assert any(len(st) == 1 for st in sts)
        assert partial[key] - {0}, ("no partial last chunk", key)
