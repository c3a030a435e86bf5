"""Every way a query row can take through the prefilter mode, on every candidate-pass kernel variant, at the size where
the planner picks that variant by itself (release library, no development knobs).

The certificate argument says the fp16 candidate pass + certificate, the range pass over a tie plateau (four-wave and
ping-pong range kernels, one or several 32 768-query chunks), the range overflow and the uncertified rows (exact
kernel, in chunks or for the whole call) and the all-zero closed form all return the canonical bits.  Each is its own
hand-written kernel, chosen by padded dimension, list width K' and the number of unique queries against the CU count,
so each case here:

  - builds an input whose size is computed from the device's CU count (prefilter_shape / knn_plan_compute thresholds)
    and whose rows are made to take the rare ways (_paths_input),
  - asserts from fdr_last_knn_trace that the intended variant ran and that the target strata are non-empty,
  - compares ALL rows bit for bit with exact mode in the same context (class layer off and forced),
  - compares rows drawn per stratum (tests/_strata.py) with the CPU oracle over all targets,

in the all-pairs form and in the rank form (a query block inside a larger target set, with a non-zero t_base)."""
import zlib

import numpy as np
import pytest

from _guarded import knn_dev_guarded
from _paths_rows import CASES, MIX, RESERVED, _normalize, _paths_input
from _strata import stratified_rows
from fedrann_amd import _lib

pytestmark = pytest.mark.gpu

PER = 32      # oracle rows per stratum


def _knn(ctx, Ehat, zero, q0, nq, d, k, t_base, mode, dedup):
    """fdr_knn_dev of rows [q0, q0 + nq) against all rows: (idx, dist, paths, trace) on the host."""
    ctx.set_knn_mode(mode)
    ctx.set_dedup_mode(dedup)
    # (workspace and outputs hold 0xFF bytes between canaries, checked after the synchronise: tests/_guarded.py)
    idx, dst, ws = knn_dev_guarded(ctx, Ehat, zero, q0, nq, t_base, d, k)
    paths = ctx.last_query_paths(nq)
    trace = ctx.last_knn_trace()
    del ws
    return idx.cpu().numpy(), dst.cpu().numpy(), paths, trace


def _variant(trace):
    return {key: trace[key] for key in ("dp", "pass_waves", "pass_wps", "pass_units", "pass_list_keys", "pass_pingpong")}


def _check_form(ctx, oracle, E, q0, nq, k, t_base, want, fallback):
    """One form (all-pairs: q0 = 0, nq = n; rank: a block of the rows): prefilter mode with the class layer off and
    forced against exact mode on every row, per-stratum rows against the oracle.  Returns the runs' reports."""
    n, d = E.shape
    Ehat, zero = _normalize(ctx, E)
    ref_i, ref_d, ref_p, ref_t = _knn(ctx, Ehat, zero, q0, nq, d, k, t_base, "exact", "off")
    assert ref_t["kind"] == "exact" and ref_t["exact_queries"] == nq and np.all(ref_p == _lib.PATH_EXACT)
    report, rows = {}, []
    for dedup in ("off", "force"):
        got_i, got_d, paths, tr = _knn(ctx, Ehat, zero, q0, nq, d, k, t_base, "prefilter", dedup)
        tag = "%s/%s" % ("all-pairs" if nq == n else "rank", dedup)
        assert tr["kind"] == "prefilter", (tag, tr)
        assert _variant(tr) == want, (tag, _variant(tr), want)
        assert tr["exact_fallback"] == fallback, (tag, tr)
        picked, counts, _ = stratified_rows(paths, per=PER, seed=3)
        report[tag] = {"rows": nq, "unique_queries": tr["queries"], "counts": counts,
                       "trace": {key: tr[key] for key in ("pass_launches", "pass_queues", "pass_segments", "uncertified",
                                                          "range_queries", "range_chunks", "range_pp_chunks",
                                                          "range_overflow", "exact_calls", "exact_queries")}}
        print(tag, report[tag])
        if dedup == "force":  # (the all-zero rows form one class; every other row is its own)
            assert tr["queries"] == nq - int(zero[q0:q0 + nq].sum().item()) + (1 if zero[q0:q0 + nq].any() else 0)
        else:
            assert tr["queries"] == nq
        # the path codes agree with the trace's counts
        code = paths & 0x7F
        if fallback == "whole":
            assert np.all(code == _lib.PATH_EXACT), (tag, counts)
            assert tr["exact_calls"] == 1 and tr["exact_queries"] == tr["queries"]
        else:
            assert counts["certified"] > 0 and counts["range"] > 0 and counts["overflow"] > 0, (tag, counts)
            assert counts["exact"] > counts["overflow"], (tag, counts)  # (the lonely rows: FDR_PATH_EXACT itself)
            assert tr["exact_queries"] == tr["uncertified"] + tr["range_overflow"], (tag, tr)
            assert tr["exact_calls"] == -(-tr["exact_queries"] // 16384), (tag, tr)
            if dedup == "off":
                assert counts["range"] == tr["range_queries"] - tr["range_overflow"], (tag, counts, tr)
                assert counts["overflow"] == tr["range_overflow"] and counts["zero"] == tr["zero_queries"]
        assert tr["range_overflow"] > 0 and tr["range_chunks"] == -(-tr["range_queries"] // 32768), (tag, tr)
        # every row, bit for bit, against exact mode
        assert np.array_equal(got_i, ref_i), tag
        assert np.array_equal(got_d.view(np.uint32), ref_d.view(np.uint32)), tag
        rows.append(picked)
        report[tag]["_trace"] = tr
    # rows of every stratum (of both runs), and the block's edges, against the CPU oracle over ALL targets
    rows = np.unique(np.concatenate(rows))
    Eh_host, _, z_host = oracle.normalize(E.cpu().numpy())
    wi, wd = oracle.knn_normalized(Eh_host[q0 + rows], z_host[q0 + rows], Eh_host, z_host, k, t_base=t_base)
    assert np.array_equal(ref_i[rows], wi)
    assert np.array_equal(ref_d[rows].view(np.uint32), wd.view(np.uint32))
    return report


@pytest.mark.parametrize("name,d,k,scale,mix,shape,one_launch,fallback", CASES, ids=[c[0] for c in CASES])
def test_prefilter_paths_per_variant(ctx, oracle, name, d, k, scale, mix, shape, one_launch, fallback):
    import torch
    cus = ctx.device_info()["cus"]
    n = int(scale * 512 * cus)
    if mix == "whole":
        plateau, overflow = (0, 0), -(-(n // 2 + 2048) // 1100)
    else:
        plateau, overflow = MIX[mix]
    dp = ctx.padded_dim(d)
    want = dict(zip(("pass_waves", "pass_wps", "pass_units", "pass_list_keys", "pass_pingpong"), shape), dp=dp)
    E = _paths_input(n, d, seed=zlib.crc32(name.encode()) % 1000, plateau=plateau, overflow=overflow)
    rep = _check_form(ctx, oracle, E, 0, n, k, 0, want, fallback)
    # the rank form: the same rows as a query block between 4096 further target rows on each side, row numbers from
    # t_base = 2^20 (a later rank's block of the targets)
    g = torch.Generator(device=E.device)
    g.manual_seed(7)
    pad = torch.zeros((4096, d), dtype=torch.float32, device=E.device)  # (off the reserved dimensions, like E's rows)
    pad[:, :d - RESERVED] = torch.randn((4096, 24), device=E.device, generator=g) @ \
        torch.randn((24, d - RESERVED), device=E.device, generator=g)
    T = torch.cat([pad[:2048], E, pad[2048:]]).contiguous()
    del E
    rep.update(_check_form(ctx, oracle, T, 2048, n, k, 1 << 20, want, fallback))
    for tag, r in rep.items():
        tr = r["_trace"]
        assert (tr["pass_launches"] == 1) == one_launch and (tr["pass_queues"] == 1) == one_launch, (tag, tr)
        if mix == "heavy":  # a ping-pong range chunk, then a four-wave one under 4096; the exact kernel in chunks
            assert tr["range_chunks"] == 2 and tr["range_pp_chunks"] == 1, (tag, tr)
            assert tr["range_queries"] - 32768 < 4096 and tr["exact_calls"] >= 2, (tag, tr)
        elif mix == "mixed":  # one four-wave range chunk, one exact chunk
            assert tr["range_chunks"] == 1 and tr["range_pp_chunks"] == 0 and tr["exact_calls"] == 1, (tag, tr)
        else:  # every range chunk of 4096 queries or more: the ping-pong range kernel
            assert tr["range_chunks"] >= 2 and tr["range_pp_chunks"] >= 2, (tag, tr)


def test_trace_of_exact_generic_and_failed_calls(ctx):
    """The trace after an exact-mode call and after a generic-kernel call; a call that fails its argument checks
    leaves a cleared trace and no path codes (every entry point resets both first)."""
    rng = np.random.default_rng(5)
    E = rng.standard_normal((3000, 100)).astype(np.float32)
    ctx.set_dedup_mode("off")
    ctx.set_knn_mode("exact")
    ctx.knn(E, 10)
    tr = ctx.last_knn_trace()
    assert tr["kind"] == "exact" and tr["dp"] == 128 and tr["k"] == 10 and tr["queries"] == 3000 == tr["targets"]
    assert tr["exact_calls"] == 1 and tr["exact_queries"] == 3000 and tr["exact_waves"] in (4, 8)
    assert tr["pass_launches"] == 0 and tr["range_queries"] == 0 and tr["exact_fallback"] == "none"
    assert tr["generic"] == 0 and np.all(ctx.last_query_paths(3000) == _lib.PATH_EXACT)
    ctx.set_knn_mode("auto")
    ctx.knn(rng.standard_normal((500, 700)).astype(np.float32), 12)  # d > 512: the generic kernel
    tr = ctx.last_knn_trace()
    assert tr["kind"] == "generic" and tr["generic"] == 1 and tr["dp"] == 1024 and tr["exact_calls"] == 0
    assert np.all(ctx.last_query_paths(500) == _lib.PATH_GENERIC)
    with pytest.raises(_lib.FedrannHipError):
        ctx.knn(E, 0)  # k = 0
    tr = ctx.last_knn_trace()
    assert tr["kind"] == "none" and all(v == 0 for key, v in tr.items() if key not in ("kind", "exact_fallback"))
    with pytest.raises(_lib.FedrannHipError, match="recorded codes for 0"):
        ctx.last_query_paths(3000)
    ctx.set_dedup_mode("auto")
