"""Development: which (query block, target unit) pairs of the live-chunk candidate pass share no chunk at all?

    python devtools/live_skip_stats.py [--segments N] [reads ...]        (default 1 segment; 100000 1000000)

The rows are live_chunk_stats.py's: the benchmark's reads embedded and normalised by the CPU oracle, duplicate rows
dropped, in the shipped scan order (non-empty chunks, chunk mask).  A query block is 256 consecutive rows and its mask
the OR of its rows' masks; a target unit is a 32-row tile or a 128-row stage counted from its segment's first row
(`--segments N`: N equal segments cut at tile boundaries, as knn_plan cuts them), its mask the OR of its rows'.  Where
the two masks are disjoint every similarity of the pair is exactly 0 and the pass need not visit the unit (the first
unit of a segment is always visited).  Printed, per unit size: the disjoint share of all pairs; the same weighted with
the cost model of docs/experiments.md A-22 -- a block of NL live chunks pays 0.23 + 0.09 NL of a dense visit per unit,
NL < 2 runs as 2, blocks of seven or eight live chunks run the dense kernel (cost 1, nothing skipped) --; and the
disjoint share by the block's own NL.  docs/experiments.md A-26.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from live_chunk_stats import D, NC, chunk_masks, popcount  # noqa: E402
from fedrann_amd.precompute import build_precompute_matrix  # noqa: E402
from fedrann_amd.synth import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

DISJOINT = (np.arange(256)[:, None] & np.arange(256)[None, :]) == 0  # [block mask value, unit mask value]


def or_blocks(masks, block):
    pad = (-masks.size) % block
    return np.bitwise_or.reduce(np.concatenate([masks, np.zeros(pad, dtype=np.int64)]).reshape(-1, block), axis=1)


def unit_masks(masks, unit, segments):
    """per segment: the masks of its units of `unit` rows, counted from the segment's first row"""
    tiles = -(-masks.size // 32)
    cuts = [32 * (tiles * g // segments) for g in range(segments)] + [masks.size]
    return [or_blocks(masks[b:e], unit) for b, e in zip(cuts, cuts[1:]) if e > b]


def block_cost(nl):
    return np.where(nl > 6, 1.0, 0.23 + 0.09 * np.maximum(nl, 2))


def report(masks, unit, segments):
    bm = or_blocks(masks, 256)
    nl = popcount(bm)
    segs = unit_masks(masks, unit, segments)
    units = sum(u.size for u in segs)
    hist = sum(np.bincount(u[1:], minlength=256) for u in segs)  # (unit 0 of a segment is always visited)
    per_value = (DISJOINT * hist[None, :]).sum(1)                # units a block of each mask value leaves out
    skipped = np.where(nl > 6, 0, per_value[bm])                 # ... per block; the dense group leaves none out
    cost = block_cost(nl)
    print("  %3d-row units, %d segment(s): %d blocks x %d units; disjoint pairs %.4f; weighted by 0.23 + 0.09 NL: %.4f"
          % (unit, segments, bm.size, units, skipped.sum() / (bm.size * units),
             (cost * skipped).sum() / (cost.sum() * units)))
    by_nl = ["%d: %.4f (%d)" % (n, skipped[nl == n].sum() / max(1, (nl == n).sum() * units), (nl == n).sum())
             for n in range(NC + 1)]
    print("      disjoint share by the block's NL (blocks): " + "  ".join(by_nl))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--segments", type=int, default=1)
    ap.add_argument("reads", type=int, nargs="*", default=[100_000, 1_000_000])
    a = ap.parse_args()
    for R in a.reads:
        t0 = time.time()
        s = synth(R, seed=602)
        P = build_precompute_matrix(s["counts"], D)
        E = O.embed(s["indptr"], s["indices"], (P.indptr, P.indices, P.data), s["n_features"], D)
        del s
        Eh, _, _ = O.normalize(E)
        del E
        v = np.ascontiguousarray(Eh).view(np.dtype((np.void, 4 * D))).ravel()
        _, first = np.unique(v, return_index=True)
        first.sort()  # the unique rows in row order
        m = chunk_masks(Eh[first])
        m = m[np.argsort((popcount(m) << 32) | m, kind="stable")]
        print("reads %d: %d unique rows, shipped order  (%.0f s)" % (R, first.size, time.time() - t0))
        for unit in (32, 128):
            report(m, unit, a.segments)


if __name__ == "__main__":
    main()
