"""The dense index's radius search without a GPU: the threshold margin against the float64-free model of the fp16
range pass (tests/_dense_radius_model.py), the argument checks of _lib.check_dense_radius and the command line's
refusals of --radius."""
import os

import numpy as np
import pytest

import _dense_radius_model as dmodel
from fedrann_amd import __main__ as cli
from fedrann_amd import _lib

SETS = [("%s-%d" % s, s) for s in dmodel.ADVERSARIAL] + [("mixed-100", None)]


@pytest.fixture(scope="module")
def margin_figures(oracle):
    """Per set: (radii, hits, hits whose fp16 distance is above r, hits outside {d~ <= r + M})."""
    out = {}
    for name, spec in SETS:
        E = dmodel.mixed() if spec is None else dmodel.adversarial(*spec)
        D, Dt = dmodel.exact_dists(oracle, E), dmodel.approx_dists(oracle, E)
        live = dmodel.scanned(oracle, E)[:, None]
        rows = []
        for r in dmodel.radii(D, Dt):
            hit = (D <= r) & live
            th = np.float32(r + dmodel.MARGIN)  # (float32 + float32: the library's sum)
            rows.append((float(r), int(hit.sum()), int((hit & (Dt > r)).sum()), int((hit & ~(Dt <= th)).sum())))
        out[name] = rows
    return out


def test_margin_is_the_librarys():
    """The model's margin is radius_margin() of csrc/knn_plan.inc, read from the source: the same constants, the same
    float32 sum."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fedrann_amd", "csrc",
                            "knn_plan.inc")).read()
    eps = re.search(r"#define FDR_PREFILTER_EPS ([0-9.eE+-]+)f\b", src).group(1)
    body = re.search(r"static float radius_margin\(\) \{ return (.+?); \}", src).group(1)
    m = re.fullmatch(r"FDR_PREFILTER_EPS \+ ([0-9.eE+-]+)f", body)
    assert m, body
    assert dmodel.MARGIN == np.float32(np.float32(float(eps)) + np.float32(float(m.group(1))))
    assert float(eps) == dmodel.cmodel.PREFILTER_EPS and float(dmodel.MARGIN) < 0.00105 + 1.0e-6 + 1.2e-7


@pytest.mark.parametrize("name", [s[0] for s in SETS])
def test_candidates_with_the_margin_hold_every_hit(margin_figures, name):
    for r, hits, above, lost in margin_figures[name]:
        print("%s r = %.9g: %d hits, %d with d~ > r, %d outside d~ <= r + M" % (name, r, hits, above, lost))
        assert hits > 0 and lost == 0


def test_the_margin_is_needed(margin_figures):
    """At least one (set, radius) has an oracle hit with d~ > r: a pass that admitted d~ <= r would lose it, so the GPU
    parity test on these sets and radii fails without the margin.  The worst pair's gap is far above what the order
    of the float32 accumulation can move (d 2^-24 <= 3e-5)."""
    needed = [(name, r, above) for name, rows in margin_figures.items() for r, _, above, _ in rows if above > 0]
    print(needed)
    assert needed
    assert any(name.startswith("fp16_midpoints") for name, _, _ in needed)


def test_worst_pair_gap_exceeds_accumulation_noise(oracle):
    E = dmodel.adversarial("fp16_midpoints", 128)
    D, Dt = dmodel.exact_dists(oracle, E), dmodel.approx_dists(oracle, E)
    q, t, r = dmodel.worst_pair(D, Dt)
    assert float(Dt[q, t]) - float(r) > 1.0e-4 and float(Dt[q, t]) <= float(r) + float(dmodel.MARGIN)


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_check_dense_radius_accepts_and_returns():
    r, lo, hi, cap = _lib.check_dense_radius(10, 128, 0.25)
    assert (r, lo, hi, cap) == (np.float32(0.25), 0, 10, 1 << 26) and isinstance(r, np.float32)
    assert _lib.check_dense_radius(10, 512, 0, 3, 3, 1)[1:] == (3, 3, 1)
    assert _lib.check_dense_radius(10, 1, np.nextafter(np.float32(1), np.float32(0)))[0] < 1


@pytest.mark.parametrize("kw", [
    dict(radius=1.0), dict(radius=-0.0001), dict(radius=float("nan")), dict(radius="0.5"), dict(radius=True),
    dict(radius=0.5, n=0), dict(radius=0.5, n=2 ** 31), dict(radius=0.5, d=0), dict(radius=0.5, d=513),
    dict(radius=0.5, lo=-1), dict(radius=0.5, lo=4, hi=3), dict(radius=0.5, hi=11), dict(radius=0.5, lo=1.5),
    dict(radius=0.5, max_hits=0), dict(radius=0.5, max_hits=2 ** 31), dict(radius=0.5, max_hits=1.0),
])
def test_check_dense_radius_refuses(kw):
    a = dict(n=10, d=128, lo=0, hi=None, max_hits=1 << 26)
    a.update(kw)
    with pytest.raises(ValueError):
        _lib.check_dense_radius(a["n"], a["d"], a["radius"], a["lo"], a["hi"], a["max_hits"])


def test_symbols_are_bound():
    for s in ("build", "embed", "radius_search", "radius_query", "radius_fetch", "info", "free"):
        assert "fdr_dense_index_" + s in _lib.SYMBOLS
    assert hasattr(_lib.Context, "dense_index") and hasattr(_lib.Context, "dense_index_from_csr")
    for m in ("radius_search", "radius_query", "info", "close", "__enter__", "__exit__"):
        assert hasattr(_lib.DenseIndex, m)


# ---- the command line's refusals, each before the output directory exists ---------------------------------------------
@pytest.mark.parametrize("extra,needle", [
    (["--radius", "1.0"], "--radius must be in [0, 1)"),
    (["--radius", "-0.1"], "--radius must be in [0, 1)"),
    (["--radius", "nan"], "--radius must be in [0, 1)"),
    (["--radius", "0.1", "--no-projection"], "--no-projection-radius"),
    (["--radius", "0.1", "--devices", "0,1"], "one GPU"),
    (["--radius", "0.1", "-n", "513"], "<= 512"),
])
def test_cli_refuses_radius_before_any_work(tmp_path, extra, needle):
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        cli.main(["--feature-matrix", "fm.npz", "--kmer-counts", "c.npy", "-o", str(out)] + extra)
    assert needle in str(e.value)
    assert not os.path.exists(out)


def test_cli_keeps_the_sparse_radius_messages(tmp_path):
    out = tmp_path / "out"
    with pytest.raises(SystemExit) as e:
        cli.main(["--feature-matrix", "fm.npz", "--kmer-counts", "c.npy", "-o", str(out), "--no-projection-radius", "0.5"])
    assert str(e.value) == "--no-projection-radius needs --no-projection (the projected search has no radius form)"
    assert not os.path.exists(out)
