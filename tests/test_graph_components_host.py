"""fedrann_amd.graph.component_labels, the numpy model of fdr_graph_components, against a brute force that shares nothing
with it (tests/_component_rows.py) and against scipy on the brute force's pairs: both modes, the bounds None, 0.25 and
0.0, rows sorted and shuffled; what the test graphs offer; asymmetric distances, the subnormal, one-way pairs and self
entries; every refusal of the model and of _lib.check_graph_components.  No GPU."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import _component_rows as cr
import _graph_rows as gr
from fedrann_amd import _lib
from fedrann_amd.graph import component_labels, symmetrize_rows

# n = 1000: (C, largest, singletons, components of 3 - 49 rows) of the uncut graphs, and of the mutual ones at bound 0.0
UNION_1000 = {3: (258, 623, 192, 27), 4: (238, 683, 185, 19)}
MUTUAL_1000 = {3: (229, 641, 165, 25), 4: (206, 720, 161, 16)}
MUTUAL_1000_AT_0 = {3: (545, 51, 77), 4: (526, 87, 63)}  # (C, largest, components of 3 - 49 rows)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("bound", cr.BOUNDS)
@pytest.mark.parametrize("mode", cr.COMPONENT_MODES)
@pytest.mark.parametrize("n", [1, 2, 65, 1000])
def test_the_model_is_the_brute_force(n, mode, bound, shuffled):
    graph = cr.graph_for(mode, n, seed=3, shuffled=shuffled)
    want = cr.brute_components(graph, mode, bound)
    got = component_labels(*graph, mode, bound)
    cr.equal(got, want)
    assert got[1].sum() == n and np.all(got[1] >= 1) and got[0][0] == 0
    # the partition of scipy on the joined pairs
    pairs = np.array(cr.joined_pairs(graph, mode, bound), np.int64).reshape(-1, 2)
    links = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    count, names = connected_components(links, directed=False)
    assert count == got[1].size
    cr.equal(got, cr.by_smallest_row(names.tolist()))


@pytest.mark.parametrize("seed", [3, 4])
def test_the_graphs_have_large_middling_and_single_components(seed):
    union = cr.graph_for("union", 1000, seed)
    sizes = cr.brute_components(union, "union")[1]
    assert cr.is_rich(sizes) and cr.profile(sizes) == UNION_1000[seed]
    cut = cr.brute_components(union, "union", 0.25)[1]
    assert cr.profile(cut)[1] == {3: 124, 4: 299}[seed]  # the cut takes the large component apart
    for shuffled in (False, True):
        mutual = cr.graph_for("mutual", 1000, seed, shuffled)
        sizes = cr.brute_components(mutual, "mutual")[1]
        assert cr.is_rich(sizes) and cr.profile(sizes) == MUTUAL_1000[seed]
        sizes = cr.brute_components(mutual, "mutual", 0.0)[1]
        assert cr.is_rich(sizes)
        assert (cr.profile(sizes)[0], cr.profile(sizes)[1], cr.profile(sizes)[3]) == MUTUAL_1000_AT_0[seed]
    # without the reciprocated entries there is next to nothing mutual
    plain = gr.drawn(1000, seed, lengths=cr.MUTUAL_LENGTHS)
    assert cr.profile(cr.brute_components(plain, "mutual")[1])[1] <= 2


@pytest.mark.parametrize("mode", cr.COMPONENT_MODES)
def test_the_order_of_a_rows_entries_does_not_show(mode):
    graph = cr.graph_for(mode, 1000, seed=4)
    for bound in cr.BOUNDS:
        want = component_labels(*graph, mode, bound)
        for seed in (1, 2):
            cr.equal(component_labels(*cr.shuffle_rows(graph, seed), mode, bound), want)


def _labels(graph, mode, bound=None):
    got = component_labels(*graph, mode, bound)
    cr.equal(got, cr.brute_components(graph, mode, bound))
    return got[0].tolist()


def test_asymmetric_distances_the_subnormal_one_way_pairs_and_self_entries():
    graph = gr.asymmetric()
    # 0 <-> 1 at 0.5 / 0.25, 0 <-> 3 at the subnormal / 0.0, 1 <-> 2 at 0.75 / 0.125, 2 -> 4 one way at 0.5
    assert _labels(graph, "union") == [0, 0, 0, 0, 0]
    assert _labels(graph, "mutual") == [0, 0, 0, 0, 1]  # the one-way pair joins nothing
    # a bound between a pair's two directions joins it: the minimum decides
    assert _labels(graph, "mutual", 0.3) == [0, 0, 0, 0, 1]
    assert _labels(graph, "mutual", 0.2) == [0, 1, 1, 0, 2]  # below both of 0 <-> 1
    assert _labels(graph, "mutual", 0.125) == [0, 1, 1, 0, 2]  # inclusive
    assert _labels(graph, "mutual", 0.1) == [0, 1, 2, 0, 3]
    assert _labels(graph, "union", 0.3) == [0, 0, 0, 0, 1]  # 2 -> 4 sits at 0.5
    assert _labels(graph, "union", 0.5) == [0, 0, 0, 0, 0]
    # 0.0 and the smallest subnormal are different distances
    assert _labels(graph, "mutual", 0.0) == [0, 1, 2, 0, 3]  # 3 -> 0 at 0.0
    one_way = gr.from_rows([[(1, 0.5), (0, 0.0), (3, gr.TINY)], [(0, 0.25), (2, 0.75)],
                            [(2, 0.375), (1, 0.125), (4, 0.5)], [], []])  # 0 -> 3 only, at the subnormal
    assert _labels(one_way, "union", 0.0) == [0, 1, 2, 3, 4]
    assert _labels(one_way, "union", gr.TINY) == [0, 1, 2, 0, 3]
    assert _labels(one_way, "mutual") == [0, 0, 0, 1, 2]
    # self entries change nothing
    bare = gr.from_rows([[(1, 0.5), (3, gr.TINY)], [(0, 0.25), (2, 0.75)], [(1, 0.125), (4, 0.5)], [(0, 0.0)], []])
    for mode in cr.COMPONENT_MODES:
        for bound in (None, 0.3, 0.0):
            assert _labels(bare, mode, bound) == _labels(graph, mode, bound)
    lone = gr.from_rows([[(0, 0.0)], [(1, 0.25)]])
    assert _labels(lone, "union") == _labels(lone, "mutual") == [0, 1]


def _edited(graph, fn):
    out = tuple(a.copy() for a in graph)
    fn(*out)
    return out


def test_refusals_of_the_model_and_of_the_argument_checks():
    good = gr.drawn(65, seed=31, shuffled=True, lengths=(5, 63, 64, 65))
    ip = good[0]

    def refused(graph, match):
        for mode in cr.COMPONENT_MODES:
            for bound in (None, 0.0):
                with pytest.raises(ValueError, match=match):
                    component_labels(*graph, mode, bound)
        with pytest.raises(ValueError, match=match):  # the same words as the symmetrise's
            symmetrize_rows(*graph, "union")

    def index(r, j, v):
        return lambda _, ix, ds: ix.__setitem__(int(ip[r]) + j, v)

    def distance(r, j, v):
        return lambda _, ix, ds: ds.__setitem__(int(ip[r]) + j, v)

    def twice(r, a, b):
        return lambda _, ix, ds: ix.__setitem__(int(ip[r]) + b, ix[int(ip[r]) + a])
    refused(_edited(good, index(7, 2, -3)), "row 7: an index outside")
    refused(_edited(good, index(64, 0, 65)), "row 64: an index outside")
    refused(_edited(good, distance(0, 0, -0.5)), "row 0: a distance that is negative or NaN")
    refused(_edited(good, distance(9, 1, np.nan)), "row 9: a distance that is negative or NaN")
    refused(_edited(good, distance(3, 1, -0.0)), "row 3: a distance that is negative or NaN")
    refused(_edited(good, twice(12, 0, 3)), "row 12: an index listed twice")
    several = _edited(_edited(_edited(good, twice(5, 0, 2)), distance(5, 1, np.nan)), index(40, 0, -2))
    refused(several, "row 5: a distance")  # the smallest (row, rule)
    refused(_edited(several, index(5, 3, 99)), "row 5: an index outside")
    refused(_edited(several, index(4, 0, 99)), "row 4: an index outside")
    # the mode and the bound, by the model and by the checks that need no GPU
    for call in (lambda m, b: component_labels(*good, m, b), lambda m, b: _lib.check_graph_components(good, m, b)):
        with pytest.raises(ValueError, match="union or mutual"):
            call("transpose", None)
        for mode in ("both", None, 0):
            with pytest.raises(ValueError, match="mode must be one of"):
                call(mode, None)
        for bound in (-1.0, -0.0, float("nan"), np.float32(-1e-30), float("-inf"), "0.5", True, [0.5]):
            with pytest.raises(ValueError, match="max_distance"):
                call("union", bound)
        for bound in (None, 0, 0.0, 0.5, np.float32(0.25), gr.TINY, float("inf"), 1e300):
            call("mutual", bound)
    with pytest.raises(ValueError, match="a graph is"):
        _lib.check_graph_components(good[:1])
    with pytest.raises(ValueError, match="need 1 <= n"):
        _lib.check_graph_components((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))
    code, n, _, _, _, bound = _lib.check_graph_components(good, "mutual", gr.TINY)
    assert (code, n) == (1, 65) and bound.dtype == np.float32 and int(bound.view(np.uint32)) == 1
    assert int(_lib.check_graph_components(good)[5].view(np.uint32)) == 0x7f800000
