"""Every dense k-NN route in a poisoned, guarded workspace.

fdr_knn_dev and the three-call class API carve their scratch out of one caller-supplied arena that knn_workspace.inc
lays out anew per call, per route, mode and shape: every region starts with what an earlier call left there.  Each
case here runs ONE call in one context once per fill of tests/_guarded.py -- zeros, every word 1 (a counter that reads
"one entry there", a key that beats every real key), 0xFF bytes (NaN, key ~0, -1, a stage-list entry 0xffff) and the
bytes a different call (the case's PARTNER, named in its table) left -- with

  - the workspace of exactly fdr_knn_workspace_bytes bytes and both outputs from guarded(): canaries in front, behind
    and in the round-up tail; the outputs pre-filled with 0xFF;
  - the rows placed by poisoned_rows(): NaN rows that count as real targets on both sides, in the same allocation;

and asserts, per fill: indices and distance BITS equal to the zeros run; path codes and the whole trace equal (stale
data must not move a row between certified, range, overflow and exact either); all canaries intact.  The zeros run
equals the CPU oracle over ALL targets on every query row (computed once per case), and shows from its trace and path
codes that the intended route, shape and strata ran.  Sizes: the smallest at which each kernel runs -- 3001 targets, a
query block [1111, 1888) at t_base = 5 (no multiple of 32 or 256, ragged at both ends), modes forced by the context's
setters; the wide route from 8192 targets.  A refused call (workspace one byte short) writes nothing at all."""
import contextlib

import numpy as np
import pytest

import _live_rows as LR
from _dense_rows import mixed
from _guarded import FILLS, guarded, poisoned_rows
from _paths_rows import RESERVED, _normalize, _paths_input
from _strata import stratified_rows
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

N, Q0, NQ, T_BASE = 3001, 1111, 777, 5
PAD = 192  # hostile rows on each side: more than the four tiles a stage may fetch ahead, and a partial tile
RANK, ALL = (Q0, NQ), (0, N)

_inputs = {}  # (kind, n, d) -> (E on the host, Ehat and zero flags on the device between hostile rows): made once, read-only


def _dev():
    import torch
    return torch.device("cuda", 0)


def _paths_rows(n, d):
    """_paths_input's rows with two lonely and two all-zero rows moved into the query block (its 8 + 4 special rows land
    there by chance only): the exact and zero strata are populated whatever the shuffle."""
    # two plateaus of 200 members; d = 100 leaves 94 free dimensions = 188 distinct members q +- e_j per centre, so
    # three plateaus of 150 there (every plateau still wider than the longest list, K' = 62)
    plateau = (2, 200) if 2 * (d - RESERVED - 2) >= 200 else (3, 150)
    E = _paths_input(n, d, seed=d, plateau=plateau, overflow=1).cpu().numpy()
    lonely = np.flatnonzero((np.abs(E[:, :d - RESERVED]).sum(1) == 0) & (np.abs(E).sum(1) > 0))
    zero = np.flatnonzero(np.abs(E).sum(1) == 0)
    assert lonely.size == RESERVED and zero.size == 8
    for slot, row in zip((Q0 + 1, Q0 + 300, Q0 + NQ - 2, Q0 + 31), (lonely[0], lonely[1], zero[0], zero[1])):
        E[[slot, row]] = E[[row, slot]]
    return E


def _live_rows(n, d):
    """Mask classes (tests/_live_rows.py) cut to d columns, shuffled, with 320 all-zero rows side by side inside the
    query block: in the queries' scan order they fill a whole 256-row block of mask 0; 3001 targets end in a tile of
    25 rows, 777 queries in a block of 9."""
    rng = np.random.default_rng(100 + d)
    E, _ = LR.signed_classes(rng, sizes=(470, 510, 530, 490, 521), lonely=160, zeros=0, shuffle=True)
    assert E.shape[0] == n - 320
    E = np.concatenate([E[:Q0 + 100], np.zeros((320, LR.D), np.float32), E[Q0 + 100:]])
    return np.ascontiguousarray(E[:, :d])


def _dup_rows(n, d):
    from test_gpu_parity import _rows_with_duplicate_classes
    return _rows_with_duplicate_classes(np.random.default_rng(n + d), n, d, 400)


_MAKERS = {"paths": _paths_rows, "live": _live_rows, "dup": _dup_rows,
           "dense": lambda n, d: mixed(n, d, 7 * d + 1, 128)[0]}


def _input(ctx, kind, n, d):
    import torch
    key = (kind, n, d)
    if key not in _inputs:
        E = np.ascontiguousarray(_MAKERS[kind](n, d), dtype=np.float32)
        E.setflags(write=False)
        Ehat, zero = _normalize(ctx, torch.from_numpy(E.copy()).to(_dev()))
        _inputs[key] = (E,) + poisoned_rows(Ehat, zero, PAD, PAD)
    return _inputs[key]


@contextlib.contextmanager
def _modes(ctx, mode="auto", dedup="off", live="auto", skip="auto"):
    ctx.set_knn_mode(mode)
    ctx.set_dedup_mode(dedup)
    ctx.set_live_chunks(live)
    ctx.set_live_skip(skip)
    try:
        yield
    finally:
        ctx.set_live_skip("auto")
        ctx.set_live_chunks("auto")
        ctx.set_dedup_mode("auto")
        ctx.set_knn_mode("auto")


class Call:
    """One fdr_knn_dev call: rows [q0, q0 + nq) of input (kind, n, d) against all its rows, under `modes`."""

    def __init__(self, kind, n, d, k, form, t_base=T_BASE, **modes):
        self.kind, self.n, self.d, self.k, (self.q0, self.nq), self.t_base, self.modes = kind, n, d, k, form, t_base, modes

    def __repr__(self):
        return "%s n=%d d=%d k=%d q=[%d,+%d) %s" % (self.kind, self.n, self.d, self.k, self.q0, self.nq, self.modes)

    def need(self, ctx):
        with _modes(ctx, **self.modes):
            return ctx.knn_workspace_bytes(self.nq, self.n, self.d, self.k)

    def run(self, ctx, ws, ws_bytes=None, outputs=None):
        """The call in workspace `ws` (a Guarded, or None: a null pointer); (idx, dist, paths, trace, unique) on the host,
        after the synchronise and the canary checks of workspace and outputs."""
        import torch
        _, Ehat, zero = _input(ctx, self.kind, self.n, self.d)
        nq, k, same = self.nq, self.k, self.nq == self.n
        gi, gd = outputs or (guarded(nq * k * 4, "ones", _dev()), guarded(nq * k * 4, "ones", _dev()))
        with _modes(ctx, **self.modes):
            # (all-pairs: the queries ARE the targets, the same pointers)
            ctx.knn_dev(Ehat[self.q0].data_ptr(), zero[self.q0:].data_ptr() if not same else zero.data_ptr(), nq,
                        Ehat.data_ptr(), zero.data_ptr(), self.n, self.t_base, self.d, k, gi.ptr, gd.ptr,
                        ws.ptr if ws else 0, (ws.nbytes if ws else 0) if ws_bytes is None else ws_bytes)
            torch.cuda.synchronize(_dev())
            paths, trace, unique = ctx.last_query_paths(nq), ctx.last_knn_trace(), ctx.last_unique()
        for g, what in ((ws, "workspace"), (gi, "indices"), (gd, "distances")):
            if g:
                g.check("%r: %s" % (self, what))
        return gi.view(torch.int32, (nq, k)).cpu().numpy(), gd.view(torch.float32, (nq, k)).cpu().numpy(), paths, trace, unique


# The partners ("prev"): a call of another route or shape whose workspace is at least as large, run first in the same
# buffer.  PARTNER, for every call on 3001 targets: d = 500, k = 50 in prefilter mode with the class layer forced and
# all 3001 rows as queries -- fp16 rows, 32-key lists, counters, range sets, class tables and sort scratch over every
# region of the smaller calls (for those that force the class layer themselves: an inner search of 2993 unique rows
# where theirs has 400).  PARTNER_WIDE, for the wide route's 300 queries on 8200 targets: the FAST route's prefilter +
# classes over the same 8200 targets at d = 100, k = 50.
PARTNER = Call("paths", N, 500, 50, ALL, mode="prefilter", dedup="force")
PARTNER_WIDE = Call("dense", 8200, 100, 50, (0, 8200), mode="prefilter", dedup="force")


def _workspace(ctx, call, partner, fill):
    """A guarded workspace of exactly call.need bytes holding `fill`; "prev": what `partner` left in its first bytes."""
    need = call.need(ctx)
    if fill != "prev":
        return guarded(need, fill, _dev())
    room = partner.need(ctx)
    assert room >= need, (partner, room, call, need)
    ws = guarded(room, "ones", _dev())
    partner.run(ctx, ws)
    return ws.shrink(need)


def _same(got, base, tag):
    """(a) indices and distance bits, (b) path codes and the whole trace, unique-row counts: equal to the zeros run"""
    assert np.array_equal(got[0], base[0]), "%s: %d indices differ" % (tag, int((got[0] != base[0]).sum()))
    assert np.array_equal(got[1].view(np.uint32), base[1].view(np.uint32)), "%s: %d distances differ in their bits" % (
        tag, int((got[1].view(np.uint32) != base[1].view(np.uint32)).sum()))
    assert np.array_equal(got[2], base[2]), "%s: %d path codes differ" % (tag, int((got[2] != base[2]).sum()))
    assert got[3] == base[3], (tag, {key: (v, base[3][key]) for key, v in got[3].items() if v != base[3][key]})
    assert got[4] == base[4], (tag, got[4], base[4])


def _oracle_all(oracle, call, E):
    """(d) the CPU oracle on ALL query rows of the call, over all targets"""
    Eh, _, z = oracle.normalize(E)
    q = slice(call.q0, call.q0 + call.nq)
    return oracle.knn_normalized(Eh[q], z[q], Eh, z, call.k, t_base=call.t_base)


def _poison_case(ctx, oracle, call, partner, expect, f64=False, fills=FILLS):
    E = _input(ctx, call.kind, call.n, call.d)[0]
    base = None
    for fill in fills:
        got = call.run(ctx, _workspace(ctx, call, partner, fill))
        tag = "%r in a workspace of %s" % (call, fill)
        if base is not None:
            _same(got, base, tag)
            continue
        base = got
        expect(got)
        wi, wd = _oracle_all(oracle, call, E)
        assert np.array_equal(got[0], wi), tag
        assert np.array_equal(got[1].view(np.uint32), wd.view(np.uint32)), tag
        if f64:  # (e) dense rows: the float64 bound derived in test_gpu_wide_dense._assert_f64
            from test_gpu_wide_dense import _assert_f64
            full_i, full_d = np.zeros((call.n, call.k), np.int32), np.zeros((call.n, call.k), np.float32)
            full_i[call.q0:call.q0 + call.nq], full_d[call.q0:call.q0 + call.nq] = got[0], got[1]
            _assert_f64(E, call.q0 + np.arange(call.nq), full_i, full_d, call.k, t_base=call.t_base)
    return base


# ---- 1. exact mode, FAST route ------------------------------------------------------------------------------------
def _ran_exact(call):
    def expect(got):
        _, _, paths, tr, _ = got
        assert tr["kind"] == "exact" and tr["exact_calls"] == 1 and tr["exact_queries"] == call.nq, tr
        assert tr["dp"] == (128 if call.d <= 128 else 256 if call.d <= 256 else 512) and tr["pass_launches"] == 0, tr
        assert np.all(paths == _lib.PATH_EXACT)
    return expect


@pytest.mark.parametrize("d,k", [(100, 20), (100, 64), (200, 50), (500, 20)])
def test_exact_mode(ctx, oracle, d, k):
    call = Call("paths", N, d, k, RANK, mode="exact")
    _poison_case(ctx, oracle, call, PARTNER, _ran_exact(call))


# ---- 2. prefilter mode forced: the 16-key and 32-key list forms of the small-size candidate shapes -----------------
def _ran_prefilter(call, live=0):
    def expect(got):
        _, _, paths, tr, _ = got
        assert tr["kind"] == "prefilter" and tr["pass_live"] == live and tr["queries"] == call.nq, tr
        assert tr["pass_list_keys"] == (16 if tr["kp"] <= 32 else 32) == (16 if call.k == 20 else 32), tr
        _, counts, _ = stratified_rows(paths, per=1)
        print(call, counts, {key: tr[key] for key in ("pass_waves", "pass_units", "pass_segments", "uncertified",
                                                     "range_queries", "range_overflow", "exact_calls")})
        for stratum in ("certified", "range", "overflow", "zero"):
            assert counts[stratum] > 0, (stratum, counts)
        assert counts["exact"] > counts["overflow"], counts  # (the lonely rows: FDR_PATH_EXACT itself)
        assert tr["exact_fallback"] == "chunked" and tr["exact_queries"] == tr["uncertified"] + tr["range_overflow"], tr
        assert counts["overflow"] == tr["range_overflow"] and counts["zero"] == tr["zero_queries"], (counts, tr)
    return expect


@pytest.mark.parametrize("d,k", [(100, 20), (100, 50), (200, 20), (200, 50), (500, 20), (500, 50)])
def test_prefilter_mode(ctx, oracle, d, k):
    call = Call("paths", N, d, k, RANK, mode="prefilter")
    _poison_case(ctx, oracle, call, PARTNER, _ran_prefilter(call))


# ---- 3. the live-chunk pass forced: blocked copy with its over-fetch, stage lists, per-block mask tables -------------
def _ran_live(call, skip):
    def expect(got):
        _, _, paths, tr, _ = got
        assert tr["kind"] == "prefilter" and tr["pass_live"] == 1 and tr["pass_waves"] == 8 and tr["pass_units"] == 8, tr
        assert tr["skip_live"] == (skip == "auto") and tr["zero_queries"] >= 320, tr
        items = [tr["pass_live_items_%d" % nl] for nl in range(2, 7)]
        print(call, "NL items", items, "dense", tr["pass_live_dense_items"], "stages walked / skipped",
              tr["skip_stages_walked"], tr["skip_stages_skipped"])
        # the block of all-zero queries (mask 0, run as NL = 2) and at least one block of real chunks on an NL kernel
        assert items[0] >= tr["pass_segments"] and sum(items) >= 2 * tr["pass_segments"], (items, tr)
        # (how many stages the switch saves depends on the segments the device's plan cuts; off, it saves none)
        assert tr["skip_stages_walked"] > 0 and (skip == "auto" or tr["skip_stages_skipped"] == 0), tr
        assert np.any((paths & 0x7F) == _lib.PATH_CERTIFIED) and np.any((paths & 0x7F) == _lib.PATH_ZERO)
    return expect


@pytest.mark.parametrize("skip", ["auto", "off"])
@pytest.mark.parametrize("d", [64, 100])
def test_live_chunk_pass(ctx, oracle, d, skip):
    call = Call("live", N, d, 20, RANK, mode="prefilter", live="force", skip=skip)
    _poison_case(ctx, oracle, call, PARTNER, _ran_live(call, skip))


# ---- 4. the class layer forced over the three groups above; k = 7: nine queries share a wave of the expansion -------
CLASS_MODES = {"exact": dict(mode="exact"), "prefilter": dict(mode="prefilter"),
               "live": dict(mode="prefilter", live="force")}


def _ran_classes(call, group):
    def expect(got):
        _, _, paths, tr, (ut, uq) = got
        assert call.k <= ut < call.n // 2 and 0 < uq <= ut and (uq == ut or call.nq < call.n), (ut, uq)
        assert tr["targets"] == ut and tr["queries"] == uq, tr  # the inner call searched the unique rows
        assert tr["kind"] == ("exact" if group == "exact" else "prefilter") and tr["pass_live"] == (group == "live"), tr
        assert np.any(paths & _lib.PATH_CLASS_MEMBER)
    return expect


@pytest.mark.parametrize("k", [20, 7])
@pytest.mark.parametrize("group,d", [("exact", 100), ("prefilter", 200), ("live", 100)])
def test_class_layer(ctx, oracle, group, d, k):
    for form in (RANK, ALL):
        call = Call("dup", N, d, k, form, dedup="force", **CLASS_MODES[group])
        _poison_case(ctx, oracle, call, PARTNER, _ran_classes(call, group))


# ---- 5. the WIDE route: the exact fp32 MFMA pass alone, from 8192 targets --------------------------------------------
@pytest.mark.parametrize("d,k", [(1000, 20), (100, 100), (600, 128)])
def test_wide_route(ctx, oracle, d, k):
    from test_gpu_wide_knn import _assert_mfma_trace
    call = Call("dense", 8200, d, k, (7900, 300))

    def expect(got):
        _assert_mfma_trace(ctx, call.nq, ctx.padded_dim(d), k)
        assert got[3]["queries"] == 300 and got[3]["targets"] == 8200, got[3]
    _poison_case(ctx, oracle, call, PARTNER_WIDE, expect, f64=True)


# ---- 6. the GENERIC route: no scratch at all -------------------------------------------------------------------------
def test_generic_route(ctx, oracle):
    """d = 1500 on 700 targets: a null workspace once, a poisoned one once -- the outputs' canaries and the hostile
    neighbours of the rows are what applies here."""
    call = Call("dense", 700, 1500, 20, (211, 333))
    E = _input(ctx, call.kind, call.n, call.d)[0]
    base = call.run(ctx, None)
    assert base[3]["kind"] == "generic" and base[3]["generic"] == 1 and np.all(base[2] == _lib.PATH_GENERIC), base[3]
    wi, wd = _oracle_all(oracle, call, E)
    assert np.array_equal(base[0], wi) and np.array_equal(base[1].view(np.uint32), wd.view(np.uint32))
    from test_gpu_wide_dense import _assert_f64
    full_i, full_d = np.zeros((call.n, call.k), np.int32), np.zeros((call.n, call.k), np.float32)
    full_i[211:211 + 333], full_d[211:211 + 333] = base[0], base[1]
    _assert_f64(E, 211 + np.arange(333), full_i, full_d, call.k, t_base=call.t_base)
    assert call.need(ctx) == 256
    _same(call.run(ctx, guarded(256, "ones", _dev())), base, "generic, a workspace of 0xFF bytes")


# ---- 7. the three-call class API ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [20, 7])
def test_three_call_class_api(ctx, k):
    """fdr_knn_classes_dev, fdr_knn_unique_dev in two ranges, fdr_knn_expand_dev from a packed [n_unique, 2k] buffer
    (indices, then distance bits: u_row_stride = 2k), workspace, shares, exchange buffer and outputs from guarded():
    the bits of the forced class layer's all-pairs call (test_class_layer checks those against the oracle)."""
    import torch
    d, nq_max, dev = 100, (N + 1) // 2, _dev()
    want = Call("dup", N, d, k, ALL, mode="prefilter", dedup="force")
    wi, wd = want.run(ctx, guarded(want.need(ctx), "zeros", dev))[:2]
    _, Ehat, zero = _input(ctx, "dup", N, d)
    modes = dict(mode="prefilter", dedup="force")
    with _modes(ctx, **modes):
        need = ctx.knn_workspace_bytes(nq_max, N, d, k)
    sizes = []
    for fill in FILLS:
        if fill == "prev":
            ws = guarded(PARTNER.need(ctx), "ones", dev)
            assert ws.nbytes >= need
            PARTNER.run(ctx, ws)
            ws.shrink(need)
        else:
            ws = guarded(need, fill, dev)
        with _modes(ctx, **modes):
            nu = ctx.knn_classes_dev(Ehat.data_ptr(), zero.data_ptr(), N, d, k, nq_max, ws.ptr, ws.nbytes)
            ws.check("classes: workspace")
            assert k <= nu < N // 2, nu
            packed = guarded(nu * 2 * k * 4, "ones", dev)
            pk = packed.view(torch.int32, (nu, 2 * k))
            cut = nu // 2 + 1
            for lo, hi in ((0, cut), (cut, nu)):
                gi, gd = guarded((hi - lo) * k * 4, "ones", dev), guarded((hi - lo) * k * 4, "ones", dev)
                ctx.knn_unique_dev(lo, hi, gi.ptr, gd.ptr)
                for g, what in ((ws, "workspace"), (gi, "indices"), (gd, "distances")):
                    g.check("unique rows [%d, %d): %s" % (lo, hi, what))
                tr = ctx.last_knn_trace()
                assert tr["kind"] == "prefilter" and tr["queries"] == hi - lo and tr["targets"] == nu, tr
                pk[lo:hi, :k] = gi.view(torch.int32, (hi - lo, k))
                pk[lo:hi, k:] = gd.view(torch.int32, (hi - lo, k))
            packed.check("exchange buffer")
            before = packed.payload()
            for q0, nq in (ALL, RANK):
                gi, gd = guarded(nq * k * 4, "ones", dev), guarded(nq * k * 4, "ones", dev)
                ctx.knn_expand_dev(q0, nq, T_BASE, packed.ptr, packed.ptr + 4 * k, gi.ptr, gd.ptr, u_row_stride=2 * k)
                for g, what in ((ws, "workspace"), (packed, "exchange buffer"), (gi, "indices"), (gd, "distances")):
                    g.check("expand [%d, +%d), workspace of %s: %s" % (q0, nq, fill, what))
                tag = "rows [%d, +%d) in a workspace of %s" % (q0, nq, fill)
                assert np.array_equal(gi.view(torch.int32, (nq, k)).cpu().numpy(), wi[q0:q0 + nq]), tag
                assert np.array_equal(gd.view(torch.int32, (nq, k)).cpu().numpy(), wd[q0:q0 + nq].view(np.int32)), tag
            assert np.array_equal(packed.payload(), before)  # (the expansion only reads the exchange buffer)
        sizes.append(nu)
    assert len(set(sizes)) == 1, sizes


# ---- 8. a refused call writes nothing ----------------------------------------------------------------------------------
REFUSED = [Call("paths", N, 100, 20, RANK, mode="exact"), Call("paths", N, 200, 50, RANK, mode="prefilter"),
           Call("dup", N, 100, 20, RANK, mode="prefilter", dedup="force"), Call("dense", 8200, 600, 128, (7900, 300))]


@pytest.mark.parametrize("call", REFUSED, ids=["exact", "prefilter", "classes", "wide"])
def test_refused_call_writes_nothing(ctx, call):
    """workspace_bytes one byte short: an argument error before any launch -- workspace and outputs keep their fill"""
    ws = guarded(call.need(ctx), "word1", _dev())
    gi, gd = guarded(call.nq * call.k * 4, "ones", _dev()), guarded(call.nq * call.k * 4, "ones", _dev())
    was = [g.payload() for g in (ws, gi, gd)]
    assert np.all(was[0].view(np.uint32) == 1) and np.all(was[1] == 0xFF)
    with pytest.raises(_lib.FedrannHipError, match="workspace"):
        call.run(ctx, ws, ws_bytes=ws.nbytes - 1, outputs=(gi, gd))
    for g, w, what in zip((ws, gi, gd), was, ("workspace", "indices", "distances")):
        g.check(what)
        assert np.array_equal(g.payload(), w), what


# ---- the helper itself ---------------------------------------------------------------------------------------------------
def test_guard_check_sees_one_byte():
    """one byte written by torch into the front guard, the round-up tail or the back guard makes check raise"""
    dev = _dev()
    g = guarded(1001, "ones", dev)
    g.check("untouched")
    assert g.ptr % 256 == 0 and g.ptr - g.t.data_ptr() == 4096 and g.nbytes == 1001 and np.all(g.payload() == 0xFF)
    for off, where in ((4095, -1), (4096 + 1001, 1001), (4096 + 1023, 1023), (4096 + 1024, 1024), (g.t.numel() - 1, 5119)):
        g = guarded(1001, "word1", dev)
        g.t[off] += 1
        with pytest.raises(AssertionError, match="first at offset %d$" % where):
            g.check("one byte")
    g = guarded(1001, "zeros", dev)
    g.t[4096 + 1000] = 7  # (the payload's last byte is the call's to write)
    g.check("payload")
