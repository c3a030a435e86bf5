"""fedrann_amd.graph.expand_rows, the numpy model fdr_graph_expand is held to, against a brute force of the definition
that shares nothing with it (tests/_expand_rows.py: Python's sort and sets), on the symmetrise tests' graphs
(tests/_graph_rows.py), whose three distance levels leave the fan cut among ties to the index; the argument checks of
Context.graph_expand and RescoreRows.refine's block cut, which need no GPU."""
import re

import numpy as np
import pytest

import _expand_rows as er
import _graph_rows as gr
from fedrann_amd import _lib
from fedrann_amd.graph import expand_bound, expand_rows

FANS = (1, 2, 63, 64, 65, 128)
SIZES = (1, 2, 65, 700)  # 700: above the longest drawn row (300)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_expand_rows_is_the_definition(n, shuffled):
    graph = gr.drawn(n, seed=10 * n + shuffled, shuffled=shuffled)
    for fan in FANS:
        got = expand_rows(*graph, fan)
        er.same(got, er.brute(graph, fan))
        assert got[0].dtype == np.int64 and got[1].dtype == np.int32
        for r in range(n):
            row = got[1][got[0][r]:got[0][r + 1]]
            assert np.all(row[1:] > row[:-1]) and row.size <= fan + fan * fan


def test_the_pieces_of_the_walk_change_nothing():
    graph = gr.drawn(700, seed=3, shuffled=True)
    whole = expand_rows(*graph, 64)
    for piece in (1, 1000, 1 << 30):
        er.same(expand_rows(*graph, 64, piece_entries=piece), whole)


def test_self_entries_and_the_subnormal_decide_the_cut():
    graph = gr.asymmetric()
    for fan in (1, 2, 3):
        er.same(expand_rows(*graph, fan), er.brute(graph, fan))
    one = expand_rows(*graph, 1)
    # row 0: its own entry at 0.0 is ahead of (3, the smallest subnormal) and (1, 0.5): the fan of 1 is the row itself
    assert one[1][one[0][0]:one[0][1]].tolist() == [0]
    # row 3 lists 0 at 0.0; row 0's fan of 1 is 0
    assert one[1][one[0][3]:one[0][4]].tolist() == [0]
    two = expand_rows(*graph, 2)
    assert two[1][two[0][0]:two[0][1]].tolist() == [0, 3]  # 0.0 before the subnormal before 0.5: 1 is cut
    assert two[0][5] == two[0][4]  # the empty row stays empty


def test_sub_ranges_are_slices_of_the_whole():
    graph = gr.drawn(65, seed=5, shuffled=True)
    ip, ix = expand_rows(*graph, 64)
    for lo, hi in ((0, 65), (0, 1), (3, 40), (64, 65), (17, 17), (0, 0), (65, 65)):
        got = expand_rows(*graph, 64, lo, hi)
        er.same(got, (ip[lo:hi + 1] - ip[lo], ix[ip[lo]:ip[hi]]))
        er.same(got, er.brute(graph, 64, lo, hi))
    empty = expand_rows(*graph, 64, 17, 17)
    assert empty[0].tolist() == [0] and empty[1].size == 0


def test_a_row_reached_only_through_itself_is_not_listed_and_a_listed_self_stays():
    graph = gr.from_rows([[(1, 0.5)], [(0, 0.25), (2, 0.5)], [(2, 0.0), (0, 0.5)]])
    ip, ix = expand_rows(*graph, 2)
    assert ix[ip[0]:ip[1]].tolist() == [1, 2]  # 0 -> 1 -> 0: row 0 does not list itself, so 0 is left out
    assert ix[ip[1]:ip[2]].tolist() == [0, 2]  # 1 -> 0 -> 1 and 1 -> 2 -> 2
    assert ix[ip[2]:ip[3]].tolist() == [0, 1, 2]  # row 2 lists itself: it stays; 2 -> 0 -> 1
    er.same((ip, ix), er.brute(graph, 2))


def test_a_duplicated_index_takes_two_fan_places_and_comes_out_once():
    graph = gr.from_rows([[(1, 0.0), (1, 0.0), (2, 0.25)], [(3, 0.0)], [(4, 0.0)], [], []])
    two = expand_rows(*graph, 2)
    assert two[1][two[0][0]:two[0][1]].tolist() == [1, 3]  # both places of the fan are row 1's: 2 is cut
    three = expand_rows(*graph, 3)
    assert three[1][three[0][0]:three[0][1]].tolist() == [1, 2, 3, 4]
    for fan in (1, 2, 3):
        er.same(expand_rows(*graph, fan), er.brute(graph, fan))


def test_every_refusal_carries_its_message():
    good = gr.drawn(65, seed=7, shuffled=True, lengths=(5, 63))
    ip = good[0]

    def edited(fn):
        out = tuple(a.copy() for a in good)
        fn(*out)
        return out
    bad_far = edited(lambda _, ix, ds: ix.__setitem__(int(ip[60]), 65))
    for lo, hi in ((0, 65), (0, 3), (9, 9)):  # the whole graph is checked, whatever the range
        with pytest.raises(ValueError, match=re.escape("row 60: an index outside [0, n)")):
            expand_rows(*bad_far, 5, lo, hi)
    with pytest.raises(ValueError, match=re.escape("row 2: an index outside [0, n)")):
        expand_rows(*edited(lambda _, ix, ds: ix.__setitem__(int(ip[2]) + 1, -1)), 5)
    for v in (-0.5, -0.0, np.nan):
        with pytest.raises(ValueError, match="row 4: a distance that is negative or NaN"):
            expand_rows(*edited(lambda _, ix, ds: ds.__setitem__(int(ip[4]), v)), 5)

    def several(_, ix, ds):
        ds[int(ip[4])] = np.nan
        ix[int(ip[4]) + 1] = 99
        ix[int(ip[30])] = -2
    with pytest.raises(ValueError, match="row 4: an index outside"):  # the smallest (row, rule)
        expand_rows(*edited(several), 5)
    for fan in (0, -1, 129, 2.0, True, None):
        with pytest.raises(ValueError, match="fan"):
            expand_rows(*good, fan)
        with pytest.raises(ValueError, match="fan"):
            _lib.check_graph_expand(good, fan)
    for lo, hi in ((-1, 3), (4, 3), (0, 66), (66, 66)):
        with pytest.raises(ValueError, match="no range of the n = 65 rows"):
            expand_rows(*good, 5, lo, hi)
        with pytest.raises(ValueError, match="no range of the n = 65 rows"):
            _lib.check_graph_expand(good, 5, lo, hi)
    for cap in (0, 2 ** 31, 1.5, True):
        with pytest.raises(ValueError, match="max_entries"):
            _lib.check_graph_expand(good, 5, max_entries=cap)
    with pytest.raises(ValueError, match="int32"):
        _lib.check_graph_expand((good[0], good[1].astype(np.int64), good[2]), 5)
    with pytest.raises(ValueError, match="at least one row|1 <= n"):
        _lib.check_graph_expand((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)), 5)
    n, _, _, _, fan, lo, hi = _lib.check_graph_expand(good, np.int64(5), 2)
    assert (n, fan, lo, hi) == (65, 5, 2, 65)


def test_the_block_cut_by_the_row_pointer_alone():
    graph = gr.drawn(700, seed=9)
    for fan in (1, 20, 128):
        bound = expand_bound(graph[0], fan)
        got = np.diff(expand_rows(*graph, fan)[0])
        assert np.all(got <= bound) and bound.dtype == np.int64
        assert _lib.expand_pieces(bound, int(bound.sum())) == [(0, 700)]
        cap = max(int(bound.max()), int(bound.sum()) // 7)
        pieces = _lib.expand_pieces(bound, cap)
        assert pieces == _lib.radius_pieces(bound, cap) and len(pieces) > 1
        assert _lib.expand_pieces(bound, int(bound.max()) - 1) is None
    assert _lib.expand_pieces(np.zeros(0, np.int64), 5) == [(0, 0)]


def test_the_new_entries_are_declared_and_bound():
    import os
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "fedrann_hip.h")).read()
    for name in ("fdr_graph_expand", "fdr_graph_expand_fetch", "fdr_rescore_rows_refine"):
        assert re.search(r"\bint %s\(fdr_ctx \*ctx," % name, hdr) and name in _lib.SYMBOLS
