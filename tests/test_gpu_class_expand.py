"""expand_classes_kernel (fedrann_amd/csrc/dedup_classes.inc) on made-up lists, path by path, against the numpy model of
tests/_class_model.py (itself checked against the oracle in tests/test_class_model.py, without a GPU).

The kernel rebuilds every row's list from its unique row's list in one of five ways: the inner list as it is (`fast`), a
concatenation of the classes' members (`concat`), a bitonic sort of 32, 64 or 128 keys, or K selection rounds over K * K
keys in LDS (`select`); queries per wave, idle lanes, waves per workgroup and the per-query ballot mask all depend on k.
fdr_knn_classes_dev builds the class tables from any rows and fdr_knn_expand_dev expands caller-supplied lists without
looking at the rows, so the lists here are synthetic: every unique row gets a list built for one stratum, the model's
path_of counts the queries per stratum BEFORE the GPU call (a floor per reachable stratum and for waves that mix fast
and slow queries), and indices and distance bits must equal the model's on every row, in every form of the call.

Two small end-to-end cases with real lists follow: one-hot and few-hot rows through the host API in both modes, and
through fdr_knn_dev on query blocks, with the class-member bit of the path codes checked against the model's classes."""
import numpy as np
import pytest

import _class_lists as L
import _class_model as M
from _class_lists import D, KS, N
from _guarded import guarded
from _paths_rows import _normalize
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

T_BASES = (0, 1 << 20)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _forms(k):
    qw4 = L.queries_per_wave(k)
    return [(0, N), (1, N - 2), (N // 2 + 3, 1), (37, 5 * qw4 + 1)]


@pytest.mark.parametrize("k", KS)
def test_expand_synthetic_lists(ctx, k):
    import torch
    dev, dp = _dev(), ctx.padded_dim(D)
    T = L.target_rows(k, dp, seed=k)
    cls_of_row, members, reps = M.classes_of(T)
    nu = len(members)
    pair = np.flatnonzero(T[:, 0] == 0)  # the two rows that differ in the sign of a zero alone: equal floats, two classes
    assert pair.size == 2 and np.array_equal(T[pair[0]], T[pair[1]]) and cls_of_row[pair[0]] != cls_of_row[pair[1]]
    ids, bits = L.lists(members, k, seed=1000 + k)
    paths_u = M.path_of(members, ids, bits, k)
    paths_q = paths_u[cls_of_row]
    cu, cq, mixed = L.condition(k, paths_u, paths_q)
    print("k = %d: %d rows in %d classes; lists per stratum %s; queries per stratum %s; mixed %s"
          % (k, N, nu, cu, cq, mixed))
    want = {tb: M.expand(members, cls_of_row, ids, bits, 0, N, k, tb) for tb in T_BASES}

    Td = torch.from_numpy(T).to(dev)
    zero = torch.zeros((N,), dtype=torch.uint8, device=dev)
    ctx.set_dedup_mode("force")
    try:
        ws = guarded(ctx.knn_workspace_bytes(N, N, D, k), "ones", dev)
        assert ctx.knn_classes_dev(Td.data_ptr(), zero.data_ptr(), N, D, k, N, ws.ptr, ws.nbytes) == nu
        ws.check("classes: workspace")
        # the lists: two [nu, k] arrays, and one packed [nu, 2k] buffer (a row's ids, then its distance bits)
        gu_i, gu_d, packed = (guarded(nu * k * 4, "ones", dev), guarded(nu * k * 4, "ones", dev),
                              guarded(nu * 2 * k * 4, "ones", dev))
        ids_d, bits_d = torch.from_numpy(ids).to(dev), torch.from_numpy(bits.view(np.int32)).to(dev)
        gu_i.view(torch.int32, (nu, k)).copy_(ids_d)
        gu_d.view(torch.int32, (nu, k)).copy_(bits_d)
        pk = packed.view(torch.int32, (nu, 2 * k))
        pk[:, :k], pk[:, k:] = ids_d, bits_d
        exchange = {"two arrays": ((gu_i, gu_d), gu_i.ptr, gu_d.ptr, 0),
                    "packed": ((packed,), packed.ptr, packed.ptr + 4 * k, 2 * k)}
        before = {g: g.payload() for g in (gu_i, gu_d, packed)}
        for form, (bufs, p_idx, p_dist, stride) in exchange.items():
            for q0, nq in _forms(k):
                for tb in T_BASES:
                    gi, gd = guarded(nq * k * 4, "ones", dev), guarded(nq * k * 4, "ones", dev)
                    ctx.knn_expand_dev(q0, nq, tb, p_idx, p_dist, gi.ptr, gd.ptr, u_row_stride=stride)
                    torch.cuda.synchronize(dev)
                    tag = "k = %d, rows [%d, +%d), t_base = %d, lists as %s" % (k, q0, nq, tb, form)
                    for g, what in ((ws, "workspace"), (gi, "indices"), (gd, "distances")) + tuple(
                            (b, "exchange buffer") for b in bufs):
                        g.check("%s: %s" % (tag, what))
                    got_i = gi.view(torch.int32, (nq, k)).cpu().numpy()
                    got_b = gd.view(torch.int32, (nq, k)).cpu().numpy().view(np.uint32)
                    wi, wb = want[tb][0][q0:q0 + nq], want[tb][1][q0:q0 + nq]
                    bad = np.flatnonzero(np.any(got_i != wi, axis=1) | np.any(got_b != wb, axis=1))
                    if bad.size:
                        r = int(bad[0])
                        by = {s: int(np.sum(paths_q[q0 + bad] == s)) for s in M.STRATA if np.any(paths_q[q0 + bad] == s)}
                        raise AssertionError(
                            "%s: %d rows differ from the model, per stratum %s; the first is row %d (stratum %s, list of "
                            "unique row %d):\n  got  %s %s\n  want %s %s" % (
                                tag, bad.size, by, q0 + r, paths_q[q0 + r], cls_of_row[q0 + r], got_i[r].tolist(),
                                got_b[r].tolist(), wi[r].tolist(), wb[r].tolist()))
        for g, was in before.items():
            assert np.array_equal(g.payload(), was), "k = %d: the expansion wrote into the exchange buffer" % k
    finally:
        ctx.set_dedup_mode("auto")


# ---- end to end, real lists: one-hot and few-hot rows ----------------------------------------------------------------
HOT_N, HOT_D = 4000, 32
_hot = {}


def _hot_case(oracle):
    """The rows, their classes by the oracle's normalised rows, and per k the oracle's answer over all rows and the
    strata of the real unique-row lists (the oracle over the unique rows): made once, read-only."""
    if not _hot:
        E = M.hot_rows(HOT_N, HOT_D, seed=11)
        Eh, _, zero = oracle.normalize(E)
        cls_of_row, members, reps = M.classes_of(Eh)
        per_k = {}
        for k in (3, 20, 33, 64):
            iu, du = oracle.knn_normalized(Eh[reps], zero[reps], Eh[reps], zero[reps], k)
            per_k[k] = (oracle.knn_normalized(Eh, zero, Eh, zero, k), M.path_of(members, iu, du, k, cls_of_row))
        for a in (E, cls_of_row):
            a.setflags(write=False)
        _hot.update(E=E, cls_of_row=cls_of_row, members=members, per_k=per_k)
    return _hot


# The tie strata the real lists of these rows populate, per k.  A one-hot or two-hot query meets the two-hot rows that
# share a component with it on one plateau (1 - 1/sqrt(2), 1/2): classes of one to three rows, so n is about 2k -- a
# sort32 at k = 3, sort64 / sort128 at k = 20, sort128 at k = 33; from k = 33 the lists reach the plateau at 1, where
# the one-hot classes of hundreds of rows come first (early representatives) and n passes 128.
HOT_TIES = {3: ("sort32",), 20: ("sort64", "sort128"), 33: ("sort128", "select"), 64: ("select",)}


def _assert_hot_strata(k, paths):
    c = M.counts(paths)
    print("hot rows, k = %d: queries per stratum %s" % (k, c))
    for s in ("fast", "concat") + HOT_TIES[k]:
        assert c[s] > 0, (k, s, c)
    assert all(c[s] == 0 for s in M.STRATA if s not in M.reachable(k)), (k, c)


@pytest.mark.parametrize("mode", ["exact", "prefilter"])
@pytest.mark.parametrize("k", [3, 20, 33, 64])
def test_hot_rows_host_api(ctx, oracle, k, mode):
    case = _hot_case(oracle)
    (wi, wd), paths = case["per_k"][k]
    _assert_hot_strata(k, paths)
    ctx.set_dedup_mode("force")
    ctx.set_knn_mode(mode)
    try:
        gi, gd = ctx.knn(case["E"], k)
        ut, uq = ctx.last_unique()
    finally:
        ctx.set_knn_mode("auto")
        ctx.set_dedup_mode("auto")
    assert ut == uq == len(case["members"]), (ut, uq, len(case["members"]))
    bad = np.flatnonzero(np.any(gi != wi, axis=1) | np.any(gd.view(np.uint32) != wd.view(np.uint32), axis=1))
    assert bad.size == 0, "k = %d, %s mode: %d rows differ from the oracle, per stratum %s; the first is row %d (%s)" % (
        k, mode, bad.size, M.counts(paths[bad]), int(bad[0]), paths[bad[0]])


@pytest.mark.parametrize("k", [3, 20, 33, 64])
def test_hot_rows_rank_form(ctx, oracle, k):
    """fdr_knn_dev on query blocks of the rows (only the blocks' unique rows are searched: the expansion finds a row's
    list through the unique-query numbering), then all pairs: the class-member bit of every row's path code"""
    import torch
    from fedrann_amd.distributed import HipEngine
    case = _hot_case(oracle)
    (wi, wd), paths = case["per_k"][k]
    size = np.array([len(m) for m in case["members"]])
    engine = HipEngine(ctx, _dev())
    Ehat, zero = _normalize(ctx, torch.from_numpy(np.array(case["E"])).to(_dev()))
    ctx.set_dedup_mode("force")
    try:
        for q0, nq in ((0, 2048), (2048, 1951), (0, HOT_N)):  # (an aligned block, a ragged one, all pairs)
            gi, gd = engine.knn(Ehat[q0:q0 + nq], zero[q0:q0 + nq], nq, Ehat, zero, HOT_N, HOT_D, k)
            gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
            ut, uq = ctx.last_unique()
            assert ut == size.size and uq == np.unique(case["cls_of_row"][q0:q0 + nq]).size, (q0, nq, ut, uq)
            bad = np.flatnonzero(np.any(gi != wi[q0:q0 + nq], axis=1) |
                                 np.any(gd.view(np.uint32) != wd[q0:q0 + nq].view(np.uint32), axis=1))
            assert bad.size == 0, "k = %d, rows [%d, +%d): %d rows differ from the oracle, per stratum %s; the first is " \
                "row %d (%s)" % (k, q0, nq, bad.size, M.counts(paths[q0 + bad]), q0 + int(bad[0]), paths[q0 + bad[0]])
        codes = ctx.last_query_paths(HOT_N)
    finally:
        ctx.set_dedup_mode("auto")
    member = (codes & _lib.PATH_CLASS_MEMBER) != 0
    assert np.array_equal(member, size[case["cls_of_row"]] > 1), "k = %d: %d rows with a wrong class-member bit" % (
        k, int(np.sum(member != (size[case["cls_of_row"]] > 1))))
    valid = (_lib.PATH_CERTIFIED, _lib.PATH_RANGE, _lib.PATH_EXACT, _lib.PATH_ZERO, _lib.PATH_RANGE_OVERFLOW)
    assert np.all(np.isin(codes & 0x7F, valid)), np.unique(codes & 0x7F)
